"""gpv_plan_loglik_grad / _fisher / _rep with covmodel='matern_scaledim' (one range per coordinate) on the GPU.

Truth: tests/_scaledim_truth.py, dense algebra per conditioning set (float64 for whole plans, a long-double Cholesky for picked
rows).  Bar: that of tests/test_gpu_loglik_grad.py and tests/test_gpu_loglik_fisher.py: per row
|row_terms[k] - truth|_inf <= 1e-8 max(|truth_k|_inf, 1); totals within 1e-8 sum_k |term_k|.  The inputs are benign (cond.yz = 'z',
tau = 0.1 on every diagonal): every shape asserts again that the float64 truth stays within 2e-12 of the long-double one on the
rows it picks.

Shapes (n = 300, 200 at m = 63): rows of p = m + 1 = 1, 16, 17, 32, 33, 64 entries -- the three buckets filled exactly and one past
each edge, the plan's first p - 1 rows being the warm-up rows with fewer entries -- in 1, 2 and 3 dimensions, ranges 1 : 50 apart
and equal, the three closed-form smoothnesses, R = 1 and 9 replicates.  Neighbours are the exact ordered nearest neighbours of the
scaled coordinates (oracle.r_side).

  test_rows_and_totals       the three entries on one plan against the truth; the information symmetric and positive definite; the
                             replicate entry with R = 1 and R = 9; every call twice, bitwise
  test_equal_ranges_sum_to_matern   at equal ranges the value, the other derivatives and the sum of the range derivatives are those of
                             gpv_plan_loglik_grad with 'matern' on the same plan (1e-8, two different kernels)
  test_coincident_points     nu = 0.5 with coincident points inside the sets: finite, and the 0 / 0 pair contributes exactly 0
  test_nan_coordinate        failure semantics, as for 'matern'
  test_state_*               the plan's last evaluation stays intact; the refusals; the _nu entries return what the plain ones do
  test_estimation            Fisher scoring on an anisotropic field: converges, not below the isotropic fit, ranges in order
  test_estimation_other_routes   Nelder-Mead, L-BFGS-B, the GLS trend and n x R data with the family"""
import functools

import numpy as np
import pytest

import _fisher_truth as F
import _grad_truth as T
import _scaledim_truth as S

pytestmark = pytest.mark.gpu

TOL = 1e-8
TAU = 0.1
FAM = "matern_scaledim"
_F64_VS_LD = 2e-12
SHAPES = [(0, 2, "far"), (15, 1, "far"), (16, 2, "far"), (31, 3, "far"), (32, 2, "equal"), (63, 3, "far"), (10, 3, "equal")]
NUS = (0.5, 1.5, 2.5)


def _need_gpu():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


def _ranges(dim, kind):
    return np.full(dim, 0.25) if kind == "equal" else np.array([[0.02], [0.02, 1.0], [0.02, 1.0, 0.2]][dim - 1])


def _cp(dim, kind, nu):
    return np.concatenate([[1.3], _ranges(dim, kind), [nu]])


@functools.lru_cache(maxsize=None)
def _setup(m, dim, kind, n, dup=False):
    """Seeded inputs of one plan, shared read-only: locations, data, 9 replicate columns, the product's vecchia.approx"""
    G = _need_gpu()
    from oracle import r_side as R
    rng = np.random.default_rng(31 + m + dim)
    locs = rng.random((n, dim))
    z, Z = rng.standard_normal(n), rng.standard_normal((n, 9))
    if dup:                                            # every third point sits on an earlier one that is no copy itself
        for j in range(2, n, 3):                       # (copies of copies pile up more than m + 1 points at one location)
            src = int(rng.integers(j))
            locs[j] = locs[src - 1 if src % 3 == 2 else src]
    NN = None
    if m > 0:
        NN = R.findOrderedNN(locs / _ranges(dim, kind), m)
        for j in np.where(NN[:, 0] != np.arange(1, n + 1))[0]:      # a coincident earlier point wins the tie: self back in front
            c = int(np.where(NN[j] == j + 1)[0][0])
            NN[j, 0], NN[j, c] = NN[j, c], NN[j, 0]
        NN = np.nan_to_num(NN, nan=0.0).astype(np.int32)
    va = G.vecchia_specify(locs, m, ordering="none", cond_yz="z", NNarray=NN)
    for a in (locs, z, Z, va["locsord"], va["U_prep"]["revNNarray"], va["U_prep"]["revCond"]):
        a.setflags(write=False)
    return locs, z, Z, va


def _plan(G, va, z, locs=None):
    prep = va["U_prep"]
    plan = G.Plan(va["locsord"] if locs is None else locs, prep["revNNarray"], prep["revCond"])
    plan.set_data(z)
    return plan


def _check_rows(rows, truth, what):
    err = T.scaled_row_error(rows, truth)
    print(f"{what}: worst row error {err.max():.3e} (row {int(err.argmax())})")
    assert err.max() <= TOL, (what, float(err.max()), int(err.argmax()))
    return float(err.max())


def _check_totals(tot, truth, what):
    want, scale = truth.sum(axis=0), np.abs(truth).sum(axis=0)
    keep = ~np.isnan(want)
    assert np.array_equal(np.isnan(tot), ~keep), (what, tot)
    off = np.abs(tot[keep] - want[keep])                   # (m = 0 has no pairs: its range terms and their scale are exact zeros)
    print(f"{what}: totals off by {(off / np.maximum(scale[keep], 1e-300)).max():.3e} of sum |term|")
    assert np.all(off <= TOL * scale[keep]), (what, tot, want)


def _check_matrix(info, dim, definite=True):
    """exactly symmetric; NaN exactly in the smoothness row and column; positive definite on the differentiated parameters"""
    assert info.shape == (dim + 3, dim + 3) and np.array_equal(info, info.T, equal_nan=True)
    pos = list(range(dim + 1)) + [dim + 2]
    nan = np.ones(info.shape, bool)
    nan[np.ix_(pos, pos)] = False
    assert np.array_equal(np.isnan(info), nan)
    if definite:
        assert np.linalg.eigvalsh(info[np.ix_(pos, pos)]).min() > 0


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("m,dim,kind", SHAPES, ids=["m%d-d%d-%s" % s for s in SHAPES])
def test_rows_and_totals(m, dim, kind, nu):
    G = _need_gpu()
    n = 200 if m == 63 else 300
    locs, z, Z, va = _setup(m, dim, kind, n)
    cp = _cp(dim, kind, nu)
    revNN = va["U_prep"]["revNNarray"]
    truth = S.full_rows_f64(va["locsord"], revNN, z, cp, TAU)
    nc = S.ncols(dim)
    # the inputs are benign: float64 against long double on the warm-up rows and 12 seeded ones
    pick = np.union1d(np.arange(0, min(m + 1, n), 7), np.random.default_rng(5).choice(n, 12, replace=False))
    ld = np.stack([S.full_row_ld(va["locsord"], revNN[k], z, cp, TAU) for k in pick]).astype(np.float64)
    f64_err = T.scaled_row_error(truth[pick], ld).max()
    print(f"float64 restatement against long double on {len(pick)} rows: {f64_err:.2e}")
    assert f64_err <= _F64_VS_LD
    plan = _plan(G, va, z)
    # value and gradient
    ll, grad, nfail, rows = plan.loglik_grad(FAM, cp, TAU, row_terms=True)
    assert nfail == 0 and rows.shape == (n, nc) and grad.shape == (dim + 3,)
    _check_rows(rows, truth[:, :nc], "grad, all rows")
    _check_rows(rows[pick], ld[:, :nc], "grad, picked rows against long double")
    _check_totals(np.concatenate([[ll], grad]), truth[:, :nc], "grad totals")
    again = plan.loglik_grad(FAM, cp, TAU, row_terms=True)
    assert again[0] == ll and np.array_equal(again[1], grad, equal_nan=True) and np.array_equal(again[3], rows, equal_nan=True)
    # ... with the information
    ll_f, grad_f, info, nfail, rows_f = plan.loglik_fisher(FAM, cp, TAU, row_terms=True)
    assert nfail == 0 and rows_f.shape == truth.shape
    _check_rows(rows_f, truth, "fisher, all rows")
    _check_rows(rows_f[pick], ld, "fisher, picked rows against long double")
    _check_totals(np.concatenate([[ll_f], grad_f, F.tri(info)]), truth, "fisher totals")
    _check_matrix(info, dim, definite=m > 0)               # (m = 0: no pairs, the ranges carry no information)
    again = plan.loglik_fisher(FAM, cp, TAU, row_terms=True)
    assert again[0] == ll_f and np.array_equal(again[2], info, equal_nan=True) and np.array_equal(again[4], rows_f, equal_nan=True)
    # ... over replicates: one column (the plan's data again) and nine
    for R_ in (1, 9):
        Zr = z[:, None] if R_ == 1 else Z
        want = truth if R_ == 1 else S.rep_rows_f64(va["locsord"], revNN, Zr, cp, TAU)
        plan.set_replicates(Zr)
        ll_r, grad_r, info_r, nfail, rows_r = plan.loglik_replicates(FAM, cp, TAU, row_terms=True)
        assert nfail == 0
        _check_rows(rows_r, want, f"replicates R = {R_}, all rows")
        _check_totals(np.concatenate([[ll_r], grad_r, F.tri(info_r)]), want, f"replicates R = {R_} totals")
        _check_matrix(info_r, dim, definite=m > 0)
        again = plan.loglik_replicates(FAM, cp, TAU, row_terms=True)
        assert again[0] == ll_r and np.array_equal(again[2], info_r, equal_nan=True) and np.array_equal(again[4], rows_r, equal_nan=True)


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("m,dim", [(16, 2), (10, 3), (15, 1)], ids=["m16-d2", "m10-d3", "m15-d1"])
def test_equal_ranges_sum_to_matern(m, dim, nu):
    G = _need_gpu()
    n, r = 300, 0.25
    locs, z, Z, va = _setup(m, dim, "equal", n)
    plan = _plan(G, va, z)
    _, _, _, sd = plan.loglik_grad(FAM, _cp(dim, "equal", nu), TAU, row_terms=True)
    _, _, _, iso = plan.loglik_grad("matern", [1.3, r, nu], TAU, row_terms=True)
    folded = np.stack([sd[:, 0], sd[:, 1], sd[:, 2:2 + dim].sum(axis=1), sd[:, dim + 2], sd[:, dim + 3]], axis=1)
    _check_rows(folded, iso, "equal ranges folded onto 'matern'")


@pytest.mark.parametrize("dim", (1, 2, 3))
def test_coincident_points(dim):
    G = _need_gpu()
    n, m = 300, 10
    locs, z, Z, va = _setup(m, dim, "far", n, dup=True)
    cp = _cp(dim, "far", 0.5)
    revNN = va["U_prep"]["revNNarray"]
    x = va["locsord"]
    inside = sum(len(np.unique(x[T.valid_entries(revNN[k])], axis=0)) < len(T.valid_entries(revNN[k])) for k in range(n))
    assert inside >= 50                                       # sets that hold two distinct rows at one location
    truth = S.full_rows_f64(x, revNN, z, cp, TAU)
    plan = _plan(G, va, z)
    ll, grad, info, nfail, rows = plan.loglik_fisher(FAM, cp, TAU, row_terms=True)
    assert nfail == 0 and np.isfinite(ll) and np.all(np.isfinite(np.delete(grad, dim + 1)))
    assert np.all(np.isfinite(np.delete(rows[:, :S.ncols(dim)], dim + 2, axis=1)))
    _check_rows(rows, truth, "coincident points, fisher rows")
    _, _, _, rows_g = plan.loglik_grad(FAM, cp, TAU, row_terms=True)
    _check_rows(rows_g, truth[:, :S.ncols(dim)], "coincident points, grad rows")
    # the 0 / 0 pair alone: two rows at one location, the second conditioning on the first.  Every pair of its block has h = 0,
    # so every range derivative of the row is exactly 0
    two = np.repeat(np.full((1, dim), 0.3), 2, axis=0)
    va2 = G.vecchia_specify(two, 1, ordering="none", cond_yz="z", NNarray=np.array([[1, 0], [2, 1]], dtype=np.int32))
    p2 = _plan(G, va2, np.array([0.4, -0.7]))
    for call in (p2.loglik_grad, p2.loglik_fisher):
        r2 = call(FAM, cp, TAU, row_terms=True)[-1]
        assert np.all(r2[:, 2:2 + dim] == 0.0) and np.all(np.isfinite(r2[:, [0, 1, dim + 3]]))
    _check_rows(p2.loglik_fisher(FAM, cp, TAU, row_terms=True)[-1],
                S.full_rows_f64(two, va2["U_prep"]["revNNarray"], np.array([0.4, -0.7]), cp, TAU), "the coincident pair alone")


@pytest.mark.parametrize("dim", (1, 3))
def test_nan_coordinate(dim):
    G = _need_gpu()
    n, m, bad = 300, 10, 150
    locs, z, Z, va = _setup(m, dim, "far", n)
    cp = _cp(dim, "far", 1.5)
    poisoned = np.array(va["locsord"])
    poisoned[bad, dim - 1] = np.nan                         # the LAST coordinate
    plan = _plan(G, va, z, locs=poisoned)
    revNN = va["U_prep"]["revNNarray"]
    hit = np.array([bad in T.valid_entries(revNN[k]) for k in range(n)])
    truth = S.full_rows_f64(va["locsord"], revNN, z, cp, TAU)
    ll, grad, nfail, rows = plan.loglik_grad(FAM, cp, TAU, row_terms=True)
    assert hit.sum() >= 1 and nfail == hit.sum()
    assert ll == -np.inf and np.all(np.isnan(grad)) and np.all(np.isnan(rows[hit]))
    _check_rows(rows[~hit], truth[~hit][:, :S.ncols(dim)], "grad rows away from the NaN coordinate")
    ll, grad, info, nfail, rows = plan.loglik_fisher(FAM, cp, TAU, row_terms=True)
    assert nfail == hit.sum() and ll == -np.inf and np.all(np.isnan(grad)) and np.all(np.isnan(info)) and np.all(np.isnan(rows[hit]))
    _check_rows(rows[~hit], truth[~hit], "fisher rows away from the NaN coordinate")


def test_state_last_evaluation_stays_intact():
    G = _need_gpu()
    locs, z, Z, va = _setup(16, 2, "far", 300)
    cp = _cp(2, "far", 1.5)
    plan = _plan(G, va, z)
    plan.set_replicates(Z)
    plan.eval(FAM, cp, TAU, G.GPV_WANT_U | G.GPV_WANT_LOGLIK_Z)       # (the evaluation wrote the scaled copy with ITS ranges)
    sums, Lent, stamp = plan.sums(), plan.Lentries(), plan.factor_stamp()
    other = [0.9, 0.3, 0.05, 2.5]
    for call in (lambda: plan.loglik_grad(FAM, other, 0.3), lambda: plan.loglik_fisher(FAM, other, 0.3),
                 lambda: plan.loglik_replicates(FAM, other, 0.3)):
        out = call()
        assert out[-1] == 0 and np.isfinite(out[0])
        assert np.array_equal(plan.sums(), sums) and np.array_equal(plan.Lentries(), Lent) and plan.factor_stamp() == stamp
    # and the next evaluation is not disturbed by the copy the calls left behind
    plan.eval(FAM, cp, TAU, G.GPV_WANT_U | G.GPV_WANT_LOGLIK_Z)
    assert np.array_equal(plan.sums(), sums) and np.array_equal(plan.Lentries(), Lent)


def test_state_refusals_and_nu_entries():
    G = _need_gpu()
    locs, z, Z, va = _setup(16, 2, "far", 300)
    cp = _cp(2, "far", 1.5)
    plan = _plan(G, va, z)
    plan.set_replicates(Z)

    def status(fn):
        with pytest.raises(G.GpvError) as e:
            fn()
        return e.value.status

    calls = (plan.loglik_grad, plan.loglik_fisher, plan.loglik_replicates)
    for call in calls:
        assert status(lambda: call(FAM, [1.3, 0.02, 1.0, 0.8], TAU)) == 4                       # GPV_ERR_UNSUPPORTED_NU
        assert status(lambda: call(FAM, [1.3, 0.02, 1.0, 0.8], TAU, smoothness_grad=True)) == 4  # not differentiated: the same
        assert status(lambda: call(FAM, [1.3, 0.02, 1.5], TAU)) == 2                            # GPV_ERR_BAD_ARG: the count
        assert status(lambda: call(FAM, [1.3, 0.02, 1.0, 0.2, 1.5], TAU)) == 2
        assert status(lambda: call(FAM, [1.3, 0.02, 0.0, 1.5], TAU)) == 2                       # a range of 0
        assert status(lambda: call(FAM, [1.3, 0.02, np.inf, 1.5], TAU)) == 2
        assert status(lambda: call(FAM, cp, 0.0)) == 2
        a, b = call(FAM, cp, TAU, row_terms=True), call(FAM, cp, TAU, row_terms=True, smoothness_grad=True)
        assert a[0] == b[0] and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[1:], b[1:]) if isinstance(x, np.ndarray))
    # more than three coordinates: the kernels' five parameter slots are the limit
    rng = np.random.default_rng(1)
    l5 = rng.random((300, 5))
    va5 = G.vecchia_specify(l5, 10, ordering="none", cond_yz="z", nn_backend="host")
    p5 = _plan(G, va5, z)
    p5.set_replicates(Z)
    cp5 = [1.3, 0.3, 0.3, 0.3, 0.3, 0.3, 1.5]
    for call in (p5.loglik_grad, p5.loglik_fisher, p5.loglik_replicates):
        assert status(lambda: call(FAM, cp5, TAU)) == 7                                         # GPV_ERR_STATE
    p5.eval(FAM, cp5, TAU, G.GPV_WANT_LOGLIK_Z)                                                 # (evaluation takes any dimension <= 8)
    s5 = p5.sums()
    assert s5[6] == 0 and np.isfinite(s5[2]) and np.isfinite(s5[3])                             # no failed row, finite sums
    # the refusals of 'matern' hold for this family as well
    prep = va["U_prep"]
    nodata = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
    assert status(lambda: nodata.loglik_fisher(FAM, cp, TAU)) == 7                              # no data
    shard = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"], row_begin=0, row_end=150)
    shard.set_data(z)
    assert status(lambda: shard.loglik_grad(FAM, cp, TAU)) == 7                                 # a row shard


@functools.lru_cache(maxsize=None)
def _field():
    """n = 1500 in the unit square, Matern 1.5 with ranges (0.05, 0.25), variance 1, nugget 0.05: a dense Cholesky draw"""
    rng = np.random.default_rng(2024)
    n = 1500
    locs = rng.random((n, 2))
    C, _ = S.cov_and_derivs(locs, [1.0, 0.05, 0.25, 1.5])
    data = np.linalg.cholesky(C + 0.05 * np.eye(n)) @ rng.standard_normal(n)
    return locs, data


def test_estimation():
    G = _need_gpu()
    locs, data = _field()
    kw = dict(m=10, cond_yz="z", output_level=0, smoothness=1.5, method="fisher")
    iso = G.vecchia_estimate(data, locs, **kw)
    sd = G.vecchia_estimate(data, locs, covmodel=FAM, **kw)
    reltol = np.sqrt(np.finfo(float).eps)
    print("isotropic", iso["neg_loglik"], iso["theta_hat"], "scaled", sd["neg_loglik"], sd["theta_hat"], "se", sd["theta_se"],
          "evaluations", iso["n_evals"], sd["n_evals"])
    assert sd["convergence"] == 0
    assert len(sd["theta_hat"]) == 4 and len(sd["theta_se"]) == 4              # variance, range_1, range_2, nugget
    assert -sd["neg_loglik"] >= -iso["neg_loglik"] - reltol * abs(iso["neg_loglik"])   # nested models, one plan
    assert sd["theta_hat"][2] > sd["theta_hat"][1]
    assert np.all(np.isfinite(sd["theta_se"])) and np.all(sd["theta_se"] > 0)
    # once more on neighbours chosen in the fitted metric: continues from the estimate and does not get worse on ITS plan
    rn = G.vecchia_estimate(data, locs, covmodel=FAM, reneighbor=True, **kw)
    print("reneighbor", rn["neg_loglik"], rn["theta_hat"])
    assert rn["convergence"] == 0 and rn["theta_hat"][2] > rn["theta_hat"][1] and np.all(np.isfinite(rn["theta_se"]))


def test_estimation_other_routes():
    """The other searches and data layouts of vecchia_estimate take the family: Nelder-Mead with a free smoothness, L-BFGS-B, the
    GLS trend, n x R data.  n = 400: the routes run and agree on the order of the ranges; their accuracy is that of the calls above."""
    G = _need_gpu()
    rng = np.random.default_rng(77)
    n = 400
    locs = rng.random((n, 2))
    C, _ = S.cov_and_derivs(locs, [1.0, 0.05, 0.25, 1.5])
    Lc = np.linalg.cholesky(C + 0.05 * np.eye(n))
    Z = Lc @ rng.standard_normal((n, 3))
    kw = dict(m=10, cond_yz="z", output_level=0, covmodel=FAM)
    fs = G.vecchia_estimate(Z[:, 0], locs, smoothness=1.5, method="fisher", **kw)
    lb = G.vecchia_estimate(Z[:, 0], locs, smoothness=1.5, method="L-BFGS-B", **kw)
    nm = G.vecchia_estimate(Z[:, 0], locs, method="Nelder-Mead", maxit=60, **kw)
    gl = G.vecchia_estimate(Z[:, 0] + 2.0, locs, smoothness=1.5, method="fisher", trend="gls", **kw)
    rp = G.vecchia_estimate(Z, locs, smoothness=1.5, method="fisher", **kw)
    print("fisher", fs["theta_hat"], "L-BFGS-B", lb["theta_hat"], "Nelder-Mead", nm["theta_hat"], "gls", gl["theta_hat"],
          gl["beta_hat"], "replicates", rp["theta_hat"], rp["theta_se"])
    reltol = np.sqrt(np.finfo(float).eps)
    assert fs["convergence"] == 0 and fs["neg_loglik"] <= lb["neg_loglik"] + 100 * reltol * abs(lb["neg_loglik"])   # (test_estimation_fisher's bar)
    assert len(fs["theta_hat"]) == 4 and len(lb["theta_hat"]) == 4 and len(nm["theta_hat"]) == 5 and np.isfinite(nm["neg_loglik"])
    assert gl["convergence"] == 0 and len(gl["theta_hat"]) == 4 and abs(gl["beta_hat"][0] - 2.0) < 1.0 and np.all(np.isfinite(gl["theta_se"]))
    assert rp["convergence"] == 0 and rp["n_replicates"] == 3 and np.all(np.isfinite(rp["theta_se"])) and np.all(rp["theta_se"] > 0)
    for est in (fs, lb, gl, rp):
        assert est["theta_hat"][2] > est["theta_hat"][1]
