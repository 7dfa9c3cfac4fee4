"""gpv_plan_loglik_rep / gpv_plan_loglik_rep_nu (gpv_rep_kernel.hpp) on the GPU: value, gradient and expected Fisher information of
the cond.yz='z' log-likelihood summed over R replicates of the data, from one pass over the conditioning sets.

Truth: the truth helpers of the one-column entries, unchanged.  For R columns a row is the sum over the columns of
tests/_grad_truth.py's rows_f64 followed by R times the information row of tests/_fisher_truth.py (tests/_grad_nu_truth.py for the
general smoothness).  Tolerances are the project's (tests/test_gpu_loglik_grad.py, tests/_parity.py): per row
|row_terms[k] - truth_k|_inf <= 1e-8 max(|truth_k|_inf, 1); totals within 1e-8 sum_k |term_k|.  Every test that adjudicates rows
first asserts the float64 truth against the long-double row truth (summed the same way) on picked rows, within the _F64_VS_LD of
tests/test_gpu_loglik_fisher.py (1e-12; the general smoothness: the mpmath adjudicator of tests/test_gpu_loglik_grad_nu.py).

Inputs are those of tests/test_gpu_loglik_grad.py::_setup (seeded uniform locations, tau = 0.1, range 0.25 sqrt(d / 2)); the
replicates are default_rng(seed).standard_normal((n, R)).  Uploads go through the C entry with ldz = n + 5 and NaN in the padding
rows, which must not be read.

  test_buckets_and_edges        buckets 16 / 32 / 64 filled exactly and past an edge, m = 0, packed records and d = 9, the four
                                closed forms and nu = 0.8 through the _nu entry; R = 1 (one chunk, mostly padding; against
                                gpv_plan_loglik_fisher on the same column), R = 17 (three chunks of 8, the last one ragged),
                                R = 3 at (10, 2)
  test_more_than_one_set_per_wavefront   n = 40 000, R = 5: the grid cap gives every wavefront 9 or 10 sets; twice, bitwise
  test_exact_at_full_conditioning        m = n - 1, R = 4: the sum of the dense multivariate normals
  test_coincident_points, test_nan_coordinate      failure semantics
  test_state_*                  the plan's data column and last evaluation stay intact; a second upload replaces the first;
                                R = 0 releases; the refusals
  test_estimation_replicates    L-BFGS-B and Fisher scoring on n x R data against Nelder-Mead; the R-fold information"""
import ctypes as C
import functools

import numpy as np
import pytest

import _fisher_truth as F
import _grad_nu_truth as N
import _grad_truth as T
import test_gpu_loglik_grad as B

pytestmark = pytest.mark.gpu

TOL = B.TOL
TAU = B.TAU
SEED = 11
_F64_VS_LD = 1e-12
SHAPES = [(0, 2), (10, 2), (15, 2), (31, 2), (40, 3), (63, 2), (15, 9)]
FAMILIES = B.FAMILIES + ("nu0.8",)
CASES = [(m, d, R) for (m, d) in SHAPES for R in (1, 17)] + [(10, 2, 3)]


def _family(fam, d):
    return ("matern", [1.3, B._range_rule(d), 0.8]) if fam == "nu0.8" else B._family(fam, d)


@functools.lru_cache(maxsize=None)
def _Z(n, R):
    Z = np.random.default_rng(SEED).standard_normal((n, R))
    Z.setflags(write=False)
    return Z


def _upload(G, plan, Z):
    """gpv_plan_set_replicates with ldz = n + 5 and NaN in the rows the call must not read"""
    from gpvecchia_amd import _lib
    n, R = Z.shape
    buf = np.full((n + 5, R), np.nan, order="F")
    buf[:n] = Z
    _lib.check(_lib.lib().gpv_plan_set_replicates(plan._h, _lib.dptr(buf), n + 5, R), "gpv_plan_set_replicates")
    assert plan.replicates() == R


def _plan(G, va, Z, locs=None, z=None):
    prep = va["U_prep"]
    plan = G.Plan(va["locsord"] if locs is None else locs, prep["revNNarray"], prep["revCond"])
    if z is not None:
        plan.set_data(z)
    _upload(G, plan, Z)
    return plan


def _call(plan, fam, cm, cp, **kw):
    return plan.loglik_replicates(cm, cp, TAU, smoothness_grad=(fam == "nu0.8"), **kw)


def _nu_sum_truth(lo, revNN, Z, cp):
    """N.rows_f64 summed over the columns of Z, then R times N.fisher_rows_f64, from the pieces those two are made of (N._groups,
    N.cov_and_derivs, T._terms, F._half_traces) with the pair functions of a group evaluated ONCE: they cost seconds per call at
    m = 63 and depend on no datum.  test_buckets_and_edges[m10-d2-R3-nu0.8] holds this against the two helpers themselves."""
    lo = np.asarray(lo, dtype=np.float64)
    n, R = Z.shape
    out = np.full((n, N.NCOLS + N.NTRI), np.nan)
    for g, rows, idx in N._groups(revNN):
        C, dC = N.cov_and_derivs(T._dist(lo[idx]), cp)
        eye = np.broadcast_to(np.eye(g), C.shape)
        S, D = C + TAU * eye, list(dC) + [eye + np.zeros_like(C)]
        e = np.zeros(g)
        e[-1] = 1.0
        val = 0.0
        for r in range(R):
            zJ = Z[:, r][idx]
            sol = np.linalg.solve(S, np.stack([np.broadcast_to(e, zJ.shape), zJ], axis=-1))
            ell, dl = T._terms(sol[..., 0], sol[..., 1], zJ, dC + [None])
            val = val + np.stack([ell] + dl, axis=-1)
        Fm = F._half_traces(np.linalg.inv(S), D)
        if g > 1:
            Fm = Fm - F._half_traces(np.linalg.inv(S[..., :-1, :-1]), [d_[..., :-1, :-1] for d_ in D])
        out[rows] = np.concatenate([val, R * F.tri(Fm)], axis=1)
    return out


def _sum_truth(va, Z, fam, d):
    """(n, cols) float64: sum over the columns of the value-and-gradient rows, then R times the information rows"""
    cm, cp = _family(fam, d)
    lo, revNN, R = va["locsord"], va["U_prep"]["revNNarray"], Z.shape[1]
    if fam == "nu0.8":
        return _nu_sum_truth(lo, revNN, Z, cp)
    else:
        val = sum(T.rows_f64(lo, revNN, Z[:, r], cm, cp, TAU) for r in range(R))
        tri = F.rows_f64(lo, revNN, cm, cp, TAU)
    return np.concatenate([val, R * tri], axis=1)


@functools.lru_cache(maxsize=None)
def _truth(m, d, n, fam, R, dup=False):
    locs, z, va = B._setup(m, d, n, dup=dup)
    t = _sum_truth(va, _Z(n, R), fam, d)
    t.setflags(write=False)
    return t


def _row_ld(va, Z, fam, d, k):
    """one row of the same sums in long double (the general smoothness: every pair function from mpmath)"""
    cm, cp = _family(fam, d)
    lo, row, R = va["locsord"], va["U_prep"]["revNNarray"][k], Z.shape[1]
    if fam == "nu0.8":
        per = [N.row_adj(lo, row, Z[:, r], cp, TAU) for r in range(R)]
        return np.concatenate([sum(p[:N.NCOLS] for p in per), R * per[0][N.NCOLS:]])
    val = sum(T.row_ld(lo, row, Z[:, r], cm, cp, TAU) for r in range(R))
    return np.concatenate([val, R * F.row_ld(lo, row, cm, cp, TAU)])


def _row_error(rows, truth):
    return (N if not np.isnan(truth).any() else T).scaled_row_error(rows, truth)


def _check_rows(rows, truth, what):
    err = _row_error(rows, truth)
    print(f"{what}: worst row error {err.max():.3e} (row {int(err.argmax())})")
    assert err.max() <= TOL, (what, float(err.max()), int(err.argmax()))


def _check_totals(ll, grad, info, truth, what):
    tot = np.concatenate([[ll], grad, F.tri(info)])
    want, scale = truth.sum(axis=0), np.abs(truth).sum(axis=0)
    keep = ~np.isnan(want)
    assert np.array_equal(np.isnan(tot), ~keep), (what, tot)
    off = np.abs(tot[keep] - want[keep])                   # (m = 0 has no pairs: its range terms and their scale are exact zeros)
    print(f"{what}: totals off by {(off / np.maximum(scale[keep], 1e-300)).max():.3e} of sum |term|")
    assert np.all(off <= TOL * scale[keep]), (what, tot, want)
    assert np.array_equal(info, info.T, equal_nan=True)


def _adjudicate(va, Z, fam, d, truth, rows, pick, what):
    ld = np.stack([_row_ld(va, Z, fam, d, k) for k in pick]).astype(np.float64)
    f64_err = _row_error(truth[pick], ld).max()
    print(f"{what}: float64 restatement against long double on {len(pick)} rows: {f64_err:.2e}")
    assert f64_err <= _F64_VS_LD                              # the inputs are benign
    _check_rows(rows[pick], ld, what + ", long-double truth")


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("m,d,R", CASES, ids=["m%d-d%d-R%d" % c for c in CASES])
def test_buckets_and_edges(m, d, R, fam):
    G = B._need_gpu()
    n = 200 if m == 63 else 300
    locs, z, va = B._setup(m, d, n)
    cm, cp = _family(fam, d)
    Z = _Z(n, R)
    plan = _plan(G, va, Z)
    ll, grad, info, nfail, rows = _call(plan, fam, cm, cp, row_terms=True)
    assert nfail == 0
    truth = _truth(m, d, n, fam, R)
    assert rows.shape == truth.shape
    _check_rows(rows, truth, "all rows, float64 truth")
    _check_totals(ll, grad, info, truth, "totals")
    # the adjudicator: ragged rows in front and seeded rows (the general smoothness: the short rows in front, mpmath per pair)
    if fam == "nu0.8":                                        # (R mpmath rows per picked row: the shortest ones)
        pick = np.arange(min(m, 1 if R > 3 else 2) + 1)
        if (m, d, R) == (10, 2, 3):                           # the composed bulk truth against the helpers it is composed from
            lo, revNN = va["locsord"], va["U_prep"]["revNNarray"]
            val = sum(N.rows_f64(lo, revNN, Z[:, r], cp, TAU) for r in range(R))
            ref = np.concatenate([val, R * N.fisher_rows_f64(lo, revNN, cp, TAU)], axis=1)
            assert N.scaled_row_error(truth, ref).max() <= 1e-14
    else:
        pick = np.union1d(np.arange(min(m + 1, 8)), np.random.default_rng(5).choice(n, 16, replace=False))
    _adjudicate(va, Z, fam, d, truth, rows, pick, "picked rows")
    # value and gradient alone (fisher = NULL): the same bits
    ll_g, grad_g, none, nfail_g = _call(plan, fam, cm, cp, fisher=False)
    assert none is None and nfail_g == 0 and ll_g == ll and np.array_equal(grad_g, grad, equal_nan=True)
    if R == 1:                                                # gpv_plan_loglik_fisher on the same column: b takes another route
        plan.set_data(Z[:, 0])
        ll1, grad1, info1, nfail1 = plan.loglik_fisher(cm, cp, TAU, smoothness_grad=(fam == "nu0.8"))
        assert nfail1 == 0
        scale = np.abs(truth).sum(axis=0)
        got, one = np.concatenate([[ll], grad, F.tri(info)]), np.concatenate([[ll1], grad1, F.tri(info1)])
        keep = ~np.isnan(one)
        assert np.array_equal(np.isnan(got), ~keep)
        print("R = 1 against gpv_plan_loglik_fisher:", (np.abs(got - one)[keep] / np.maximum(scale[keep], 1e-300)).max())
        assert np.all(np.abs(got - one)[keep] <= TOL * scale[keep])


def test_more_than_one_set_per_wavefront():
    G = B._need_gpu()
    n, m, d, R = 40000, 10, 2, 5
    rng = np.random.default_rng(17)
    locs = rng.random((n, d))
    va = G.vecchia_specify(locs, m, ordering="none", cond_yz="z")
    Z = _Z(n, R)
    cm, cp = _family("nu1.5", d)
    plan = _plan(G, va, Z)
    ll, grad, info, nfail, rows = _call(plan, "nu1.5", cm, cp, row_terms=True)
    assert nfail == 0
    truth = _sum_truth(va, Z, "nu1.5", d)
    _check_rows(rows, truth, "n = 40 000, all rows")
    _check_totals(ll, grad, info, truth, "n = 40 000 totals")
    pick = np.random.default_rng(5).choice(n, 16, replace=False)
    _adjudicate(va, Z, "nu1.5", d, truth, rows, pick, "n = 40 000, picked rows")
    ll2, grad2, info2, _, rows2 = _call(plan, "nu1.5", cm, cp, row_terms=True)
    assert ll2 == ll and np.array_equal(grad2, grad, equal_nan=True) and np.array_equal(info2, info, equal_nan=True)
    assert np.array_equal(rows2, rows, equal_nan=True)


@pytest.mark.parametrize("fam", ("nu1.5", "esqe"))
def test_exact_at_full_conditioning(fam):
    G = B._need_gpu()
    n, R = 40, 4
    locs, z, va = B._setup(n - 1, 2, n)
    cm, cp = _family(fam, 2)
    Z = _Z(n, R)
    ll, grad, info, nfail = _call(_plan(G, va, Z), fam, cm, cp)
    assert nfail == 0
    dense = [T.dense_mvn(locs, Z[:, r], cm, cp, TAU) for r in range(R)]
    ll_d, grad_d = sum(v for v, _ in dense), sum(g for _, g in dense)
    truth = _truth(n - 1, 2, n, fam, R)
    scale = np.abs(truth).sum(axis=0)
    nc = T.ncols(cm)
    keep = ~np.isnan(grad_d)
    assert np.array_equal(np.isnan(grad), ~keep)
    print("dense value off by", abs(ll - ll_d) / scale[0], "gradient", (np.abs(grad - grad_d)[keep] / scale[1:nc][keep]).max())
    assert abs(ll - ll_d) <= TOL * scale[0] and np.all(np.abs(grad - grad_d)[keep] <= TOL * scale[1:nc][keep])
    dinfo = R * F.dense(locs, cm, cp, TAU)
    iscale = F.untri(scale[nc:], F.npar(cm))
    ikeep = ~np.isnan(dinfo)
    assert np.array_equal(np.isnan(info), ~ikeep)
    assert np.all(np.abs(info - dinfo)[ikeep] <= TOL * iscale[ikeep])


@pytest.mark.parametrize("m,d", [(10, 2), (15, 9)], ids=["m10-d2", "m15-d9"])
def test_coincident_points(m, d):
    G = B._need_gpu()
    n, R = 300, 3
    locs, z, va = B._setup(m, d, n, dup=True)
    cm, cp = _family("nu1.5", d)
    Z = _Z(n, R)
    ll, grad, info, nfail, rows = _call(_plan(G, va, Z), "nu1.5", cm, cp, row_terms=True)
    assert nfail == 0
    truth = _truth(m, d, n, "nu1.5", R, dup=True)
    _check_rows(rows, truth, "coincident points, all rows")
    _check_totals(ll, grad, info, truth, "coincident points, totals")
    pick = np.random.default_rng(5).choice(n, 16, replace=False)
    _adjudicate(va, Z, "nu1.5", d, truth, rows, pick, "coincident points")


@pytest.mark.parametrize("m,d", [(10, 2), (15, 9)], ids=["m10-d2", "m15-d9"])
def test_nan_coordinate(m, d):
    G = B._need_gpu()
    n, bad, R = 300, 150, 3
    locs, z, va = B._setup(m, d, n)
    cm, cp = _family("nu1.5", d)
    poisoned = np.array(va["locsord"])
    poisoned[bad, d - 1] = np.nan                           # the LAST coordinate
    ll, grad, info, nfail, rows = _call(_plan(G, va, _Z(n, R), locs=poisoned), "nu1.5", cm, cp, row_terms=True)
    revNN = va["U_prep"]["revNNarray"]
    hit = np.array([bad in T.valid_entries(revNN[k]) for k in range(n)])
    assert hit.sum() >= 1 and nfail == hit.sum()
    assert ll == -np.inf and np.all(np.isnan(grad)) and np.all(np.isnan(info))
    assert np.all(np.isnan(rows[hit]))
    _check_rows(rows[~hit], _truth(m, d, n, "nu1.5", R)[~hit], "rows away from the NaN coordinate")


def test_state_plan_stays_intact():
    G = B._need_gpu()
    n = 300
    locs, z, va = B._setup(10, 2, n)
    cm, cp = _family("nu1.5", 2)
    plan = B._plan(G, va, z)
    plan.eval(cm, cp, TAU, G.GPV_WANT_U | G.GPV_WANT_LOGLIK_Z)
    sums, Lent, stamp = plan.sums(), plan.Lentries(), plan.factor_stamp()
    before = plan.loglik_grad(cm, cp, TAU, row_terms=True)
    _upload(G, plan, _Z(n, 17))
    ll, grad, info, nfail = plan.loglik_replicates(cm, [0.9, 0.2, 2.5], 0.3)           # other parameters than the evaluation's
    assert nfail == 0 and np.isfinite(ll)
    assert np.array_equal(plan.sums(), sums) and np.array_equal(plan.Lentries(), Lent) and plan.factor_stamp() == stamp
    after = plan.loglik_grad(cm, cp, TAU, row_terms=True)                              # the plan's own column
    assert after[0] == before[0] and np.array_equal(after[1], before[1], equal_nan=True) and after[2] == before[2]
    assert np.array_equal(after[3], before[3], equal_nan=True)
    # a second upload with another R replaces the first
    _upload(G, plan, _Z(n, 3))
    ll3, grad3, info3, nfail3, rows3 = plan.loglik_replicates(cm, cp, TAU, row_terms=True)
    truth = _truth(10, 2, n, "nu1.5", 3)
    _check_rows(rows3, truth, "second upload, R = 3")
    _check_totals(ll3, grad3, info3, truth, "second upload, totals")
    # R = 0 releases the replicates; the data column still serves its own entry
    plan.set_replicates(None)
    assert plan.replicates() == 0
    with pytest.raises(G.GpvError) as e:
        plan.loglik_replicates(cm, cp, TAU)
    assert e.value.status == 7                                                         # GPV_ERR_STATE
    again = plan.loglik_grad(cm, cp, TAU)
    assert again[0] == before[0]


def test_state_refusals():
    G = B._need_gpu()
    from gpvecchia_amd import _lib
    n = 300
    locs, z, va = B._setup(10, 2, n)
    cm, cp = _family("nu1.5", 2)
    Z = _Z(n, 3)
    plan = _plan(G, va, Z)

    def status(fn):
        with pytest.raises(G.GpvError) as e:
            fn()
        return e.value.status

    assert status(lambda: plan.loglik_replicates("matern", [1.3, 0.25, 0.8], TAU)) == 4       # GPV_ERR_UNSUPPORTED_NU
    assert status(lambda: plan.loglik_replicates("gauss", [1.3, 0.25, 0.5], TAU)) == 3        # GPV_ERR_COVTYPE
    assert status(lambda: plan.loglik_replicates("matern", [1.3, 0.25], TAU)) == 2            # GPV_ERR_BAD_ARG
    assert status(lambda: plan.loglik_replicates("matern", cp, 0.0)) == 2
    assert status(lambda: plan.loglik_replicates("matern", cp, np.inf)) == 2
    buf = np.zeros((n, 2), order="F")
    L = _lib.lib()
    assert L.gpv_plan_set_replicates(plan._h, _lib.dptr(buf), n, -1) == 2                     # R < 0
    assert L.gpv_plan_set_replicates(plan._h, None, n, 2) == 2
    assert L.gpv_plan_set_replicates(plan._h, _lib.dptr(buf), n - 1, 2) == 2                  # ldz < Nlocs
    assert plan.replicates() == 3                                                             # refused uploads change nothing
    prep = va["U_prep"]
    none = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
    none.set_data(z)
    assert status(lambda: none.loglik_replicates(cm, cp, TAU)) == 7                           # GPV_ERR_STATE: no replicates
    shard = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"], row_begin=0, row_end=150)
    shard.set_replicates(Z)
    assert status(lambda: shard.loglik_replicates(cm, cp, TAU)) == 7                          # a row shard
    sgv = G.vecchia_specify(np.array(locs), 10, ordering="none", cond_yz="SGV")
    assert status(lambda: _plan(G, sgv, Z).loglik_replicates(cm, cp, TAU)) == 7               # latent neighbours
    wide = G.vecchia_specify(np.array(locs), 64, ordering="none", cond_yz="z")
    assert status(lambda: _plan(G, wide, Z).loglik_replicates(cm, cp, TAU)) == 5              # GPV_ERR_UNSUPPORTED_M


@functools.lru_cache(maxsize=None)
def _fields():
    """R = 4 exact draws of a Matern-1.5 field (variance 2, range 0.2) plus noise 0.3 at n = 400, by dense Cholesky on the host"""
    rng = np.random.default_rng(2024)
    n, R = 400, 4
    locs = rng.random((n, 2))
    r = np.sqrt(((locs[:, None, :] - locs[None, :, :]) ** 2).sum(-1))
    c = np.sqrt(3.0) / 0.2
    S = 2.0 * (1 + c * r) * np.exp(-c * r) + 0.3 * np.eye(n)
    return locs, np.linalg.cholesky(S) @ rng.standard_normal((n, R))


def test_estimation_replicates():
    G = B._need_gpu()
    locs, data = _fields()
    R = data.shape[1]
    kw = dict(m=10, cond_yz="z", output_level=0, smoothness=1.5)
    nm = G.vecchia_estimate(data, locs, **kw)
    lb = G.vecchia_estimate(data, locs, method="L-BFGS-B", **kw)
    fs = G.vecchia_estimate(data, locs, method="fisher", **kw)
    reltol = np.sqrt(np.finfo(float).eps)
    print("Nelder-Mead", nm["neg_loglik"], nm["n_evals"], nm["theta_hat"], "L-BFGS-B", lb["neg_loglik"], lb["n_evals"],
          lb["theta_hat"], "fisher", fs["neg_loglik"], fs["n_evals"], fs["theta_hat"], "se", fs["theta_se"])
    assert lb["convergence"] == 0 and fs["convergence"] == 0
    assert lb["neg_loglik"] <= nm["neg_loglik"] + 100 * reltol * abs(nm["neg_loglik"])
    assert fs["neg_loglik"] <= nm["neg_loglik"] + 100 * reltol * abs(nm["neg_loglik"])
    for res in (nm, lb, fs):
        assert res["n_replicates"] == R and res["z"].shape == data.shape and len(res["theta_hat"]) == 3
    # the R-fold information: R times that of one column at theta_hat (the information does not depend on the data)
    va = G.vecchia_specify(locs, 10, cond_yz="z")
    th = fs["theta_hat"]
    _, _, info1 = G.vecchia_likelihood_fisher(fs["z"][:, 0], va, [th[0], th[1], 1.5], th[2])
    sub = np.delete(np.delete(info1, 2, axis=0), 2, axis=1)
    assert np.allclose(fs["fisher_info"], R * sub, rtol=1e-8, atol=0)
    # the objective the three searches share: the summed replicate likelihoods
    per = G.vecchia_likelihood_replicates(fs["z"], va, [th[0], th[1], 1.5], th[2])
    scale = np.abs(per).sum()
    assert abs(-per.sum() - fs["neg_loglik"]) <= TOL * scale
