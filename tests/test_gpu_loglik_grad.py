"""gpv_plan_loglik_grad (gpv_grad.hip) on the GPU: value and analytic gradient of the cond.yz='z' log-likelihood.

Truth: tests/_grad_truth.py, a numpy restatement of the formula (float64 for whole plans, a hand-written long-double Cholesky
for single rows).  Tolerances: per row |row_terms[k] - truth|_inf <= 1e-8 max(|truth_k|_inf, 1); totals within
1e-8 sum_k |term_k| (the project's flat bar, tests/_parity.py).

Inputs: seeded uniform locations in the unit cube, tau = 0.1, range = 0.25 sqrt(d / 2), exact ordered nearest neighbours from
oracle.r_side (the 40 000-location case takes the product's exact search instead: the oracle's is a quadratic Python loop).
They are benign: on the CPU the float64 restatement stays within _F64_VS_LD of the long-double one, measured over ALL rows of
every (m, d, family) case below (largest figure per family):
    nu0.5 8.9e-14   nu1.5 6.6e-13   nu2.5 3.9e-13   esqe 1.4e-13      coincident points: 4.2e-13      n = 40, m = 39: 2.7e-14
    n = 1000, m = 10 (test_against_existing_path): 6.6e-13
so the float64 truth (numpy's LU solve of each block) uses less than 1e-4 of the 1e-8 bar; every test asserts _F64_VS_LD
again on the rows it adjudicates.

What each case reaches:
  test_buckets_and_edges        row-length buckets 16 / 32 / 64 filled exactly (m = 15, 31, 63) and one past an edge (m = 30 in
                                32, m = 40 in 64, m = 10 in 16), m = 0 (a plan whose row stride, 4, is shorter than the bucket),
                                ragged first rows, packed records (d <= 3) and unpacked coordinates (d = 9), every family
  test_more_than_one_set_per_wavefront   n = 40 000: the grid cap gives every wavefront 9 or 10 sets; twice, bitwise
  test_exact_at_full_conditioning        m = n - 1: the Vecchia density IS the multivariate normal
  test_against_existing_path    value against the fused GPV_WANT_LOGLIK_Z sums, gradient against their central differences
  test_coincident_points        r = 0 pairs off the diagonal: variance derivative 1, range derivative exactly 0
  test_nan_coordinate           failure semantics
  test_state_*                  the plan's last evaluation stays intact; the refusals
  test_estimation               L-BFGS-B on the analytic gradient against Nelder-Mead; the default call unchanged"""
import functools

import numpy as np
import pytest

import _grad_truth as T

pytestmark = pytest.mark.gpu

TOL = 1e-8
TAU = 0.1
SHAPES = [(0, 2), (10, 2), (15, 2), (30, 2), (31, 2), (40, 3), (63, 2), (15, 9)]       # (m, d)
_F64_VS_LD = 2e-12


def _need_gpu():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


def _range_rule(d):
    return 0.25 * np.sqrt(d / 2)


def _family(name, d):
    r = _range_rule(d)
    return {"nu0.5": ("matern", [1.3, r, 0.5]), "nu1.5": ("matern", [1.3, r, 1.5]), "nu2.5": ("matern", [1.3, r, 2.5]),
            "esqe": ("esqe", [0.8, r, 0.5, 0.8 * r])}[name]


FAMILIES = ("nu0.5", "nu1.5", "nu2.5", "esqe")


@functools.lru_cache(maxsize=None)
def _setup(m, d, n, seed=11, dup=False):
    """Seeded inputs of one plan, computed once and shared read-only: locations, data, the product's vecchia.approx."""
    G = _need_gpu()
    from oracle import r_side as R
    rng = np.random.default_rng(seed)
    locs = rng.random((n, d))
    z = rng.standard_normal(n)
    if dup:                                            # every third point sits on an earlier one
        for j in range(2, n, 3):
            locs[j] = locs[rng.integers(j)]
    NN = None
    if m > 0:
        NN = R.findOrderedNN(locs, m)
        for j in np.where(NN[:, 0] != np.arange(1, n + 1))[0]:      # a coincident earlier point wins the tie: self back in front
            c = int(np.where(NN[j] == j + 1)[0][0])
            NN[j, 0], NN[j, c] = NN[j, c], NN[j, 0]
        NN = np.nan_to_num(NN, nan=0.0).astype(np.int32)
    va = G.vecchia_specify(locs, m, ordering="none", cond_yz="z", NNarray=NN)
    for a in (locs, z, va["locsord"], va["U_prep"]["revNNarray"], va["U_prep"]["revCond"]):
        a.setflags(write=False)
    return locs, z, va


def _plan(G, va, z, locs=None):
    prep = va["U_prep"]
    plan = G.Plan(va["locsord"] if locs is None else locs, prep["revNNarray"], prep["revCond"])
    plan.set_data(z)
    return plan


@functools.lru_cache(maxsize=None)
def _truth(m, d, n, fam, dup=False):
    locs, z, va = _setup(m, d, n, dup=dup)
    cm, cp = _family(fam, d)
    t = T.rows_f64(va["locsord"], va["U_prep"]["revNNarray"], z, cm, cp, TAU)
    t.setflags(write=False)
    return t


def _check_rows(rows, truth, what):
    err = T.scaled_row_error(rows, truth)
    print(f"{what}: worst row error {err.max():.3e} (row {int(err.argmax())})")
    assert err.max() <= TOL, (what, float(err.max()), int(err.argmax()))


def _check_totals(ll, grad, truth, what):
    tot = np.concatenate([[ll], grad])
    want, scale = truth.sum(axis=0), np.abs(truth).sum(axis=0)
    keep = ~np.isnan(want)
    assert np.array_equal(np.isnan(tot), ~keep), (what, tot)
    off = np.abs(tot[keep] - want[keep])                   # (m = 0 has no pairs: its range terms and their scale are exact zeros)
    print(f"{what}: totals off by {(off / np.maximum(scale[keep], 1e-300)).max():.3e} of sum |term|")
    assert np.all(off <= TOL * scale[keep]), (what, tot, want)


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("m,d", SHAPES, ids=["m%d-d%d" % s for s in SHAPES])
def test_buckets_and_edges(m, d, fam):
    G = _need_gpu()
    n = 200 if m == 63 else 300
    locs, z, va = _setup(m, d, n)
    cm, cp = _family(fam, d)
    plan = _plan(G, va, z)
    ll, grad, nfail, rows = plan.loglik_grad(cm, cp, TAU, row_terms=True)
    assert nfail == 0
    truth = _truth(m, d, n, fam)
    _check_rows(rows, truth, "all rows, float64 truth")
    _check_totals(ll, grad, truth, "totals")
    # the adjudicator on 64 seeded rows and the ragged rows in front
    pick = np.union1d(np.arange(min(m + 1, n)), np.random.default_rng(5).choice(n, 64, replace=False))
    revNN = va["U_prep"]["revNNarray"]
    ld = np.stack([T.row_ld(va["locsord"], revNN[k], z, cm, cp, TAU) for k in pick])
    f64_err = T.scaled_row_error(truth[pick], ld.astype(np.float64)).max()
    print(f"float64 restatement against long double on these rows: {f64_err:.2e}")
    assert f64_err <= _F64_VS_LD                              # the inputs are benign
    _check_rows(rows[pick], ld.astype(np.float64), "picked rows, long-double truth")


def test_more_than_one_set_per_wavefront():
    G = _need_gpu()
    n, m, d = 40000, 10, 2
    rng = np.random.default_rng(17)
    locs = rng.random((n, d))
    z = rng.standard_normal(n)
    va = G.vecchia_specify(locs, m, ordering="none", cond_yz="z")
    cm, cp = _family("nu1.5", d)
    plan = _plan(G, va, z)
    ll, grad, nfail, rows = plan.loglik_grad(cm, cp, TAU, row_terms=True)
    assert nfail == 0
    truth = T.rows_f64(va["locsord"], va["U_prep"]["revNNarray"], z, cm, cp, TAU)
    _check_rows(rows, truth, "n = 40 000, all rows")
    _check_totals(ll, grad, truth, "n = 40 000 totals")
    ll2, grad2, _, rows2 = plan.loglik_grad(cm, cp, TAU, row_terms=True)
    assert ll2 == ll and np.array_equal(grad2, grad, equal_nan=True) and np.array_equal(rows2, rows, equal_nan=True)


@pytest.mark.parametrize("fam", ("nu1.5", "esqe"))
def test_exact_at_full_conditioning(fam):
    G = _need_gpu()
    n = 40
    locs, z, va = _setup(n - 1, 2, n)
    cm, cp = _family(fam, 2)
    ll, grad, nfail = _plan(G, va, z).loglik_grad(cm, cp, TAU)
    assert nfail == 0
    ll_d, g_d = T.dense_mvn(locs, z, cm, cp, TAU)
    truth = _truth(n - 1, 2, n, fam)
    scale = np.abs(truth).sum(axis=0)                       # the scale of the totals: sum_k |term_k|
    keep = ~np.isnan(g_d)
    assert np.array_equal(np.isnan(grad), ~keep)
    print("dense MVN: value off", abs(ll - ll_d) / scale[0], "gradient off", (np.abs(grad - g_d)[keep] / scale[1:][keep]).max())
    assert abs(ll - ll_d) <= TOL * scale[0]
    assert np.all(np.abs(grad - g_d)[keep] <= TOL * scale[1:][keep])


def test_against_existing_path():
    G = _need_gpu()
    n, m, d = 1000, 10, 2
    locs, z, va = _setup(m, d, n)
    cm, cp = _family("nu1.5", d)
    plan = _plan(G, va, z)
    ll, grad, nfail = plan.loglik_grad(cm, cp, TAU)
    assert nfail == 0

    def existing(cp_, tau_):
        plan.eval(cm, cp_, tau_, G.GPV_WANT_LOGLIK_Z)
        return G.loglik_z_from_sums(plan.sums(), n)

    ll0 = existing(cp, TAU)
    print("value: gradient entry", ll, "existing path", ll0)
    assert abs(ll - ll0) <= 1e-8 * abs(ll0)
    theta = np.array([cp[0], cp[1], TAU])
    g = np.array([grad[0], grad[1], grad[3]])
    h = 1e-6 * theta
    # central differences of a float64 value: truncation 1e-10 relative (measured on the restatement), round-off eps |l| / h
    roundoff = np.finfo(float).eps * abs(ll0) / h / np.abs(g)
    print("round-off bound of the central differences, relative to the components:", roundoff)
    assert roundoff.max() < 1e-7
    for i in range(3):
        tp, tm = theta.copy(), theta.copy()
        tp[i] += h[i]
        tm[i] -= h[i]
        cd = (existing([tp[0], tp[1], 1.5], tp[2]) - existing([tm[0], tm[1], 1.5], tm[2])) / (tp[i] - tm[i])
        print("component", i, "analytic", g[i], "central difference", cd, "relative", abs(cd - g[i]) / abs(g[i]))
        assert abs(cd - g[i]) <= 1e-6 * abs(g[i])


@pytest.mark.parametrize("fam", ("nu1.5", "esqe"))
@pytest.mark.parametrize("m,d", [(10, 2), (15, 9)], ids=["m10-d2", "m15-d9"])
def test_coincident_points(m, d, fam):
    G = _need_gpu()
    n = 300
    locs, z, va = _setup(m, d, n, dup=True)
    cm, cp = _family(fam, d)
    ll, grad, nfail, rows = _plan(G, va, z).loglik_grad(cm, cp, TAU, row_terms=True)
    assert nfail == 0
    truth = _truth(m, d, n, fam, dup=True)
    _check_rows(rows, truth, "coincident points, all rows")
    _check_totals(ll, grad, truth, "coincident points, totals")


@pytest.mark.parametrize("m,d", [(10, 2), (15, 9)], ids=["m10-d2", "m15-d9"])
def test_nan_coordinate(m, d):
    G = _need_gpu()
    n, bad = 300, 150
    locs, z, va = _setup(m, d, n)
    cm, cp = _family("nu1.5", d)
    poisoned = np.array(va["locsord"])
    poisoned[bad, d - 1] = np.nan                           # the LAST coordinate
    ll, grad, nfail, rows = _plan(G, va, z, locs=poisoned).loglik_grad(cm, cp, TAU, row_terms=True)
    revNN = va["U_prep"]["revNNarray"]
    hit = np.array([bad in T.valid_entries(revNN[k]) for k in range(n)])
    assert hit.sum() >= 1 and nfail == hit.sum()
    assert ll == -np.inf and np.all(np.isnan(grad))
    assert np.all(np.isnan(rows[hit]))
    _check_rows(rows[~hit], _truth(m, d, n, "nu1.5")[~hit], "rows away from the NaN coordinate")


def test_state_last_evaluation_stays_intact():
    G = _need_gpu()
    locs, z, va = _setup(10, 2, 300)
    cm, cp = _family("nu1.5", 2)
    plan = _plan(G, va, z)
    plan.eval(cm, cp, TAU, G.GPV_WANT_U | G.GPV_WANT_LOGLIK_Z)
    sums, Lent, stamp = plan.sums(), plan.Lentries(), plan.factor_stamp()
    ll, grad, nfail = plan.loglik_grad(cm, [0.9, 0.2, 2.5], 0.3)      # other parameters than the evaluation's
    assert nfail == 0 and np.isfinite(ll)
    assert np.array_equal(plan.sums(), sums) and np.array_equal(plan.Lentries(), Lent) and plan.factor_stamp() == stamp


def test_state_refusals():
    G = _need_gpu()
    locs, z, va = _setup(10, 2, 300)
    cm, cp = _family("nu1.5", 2)
    plan = _plan(G, va, z)

    def status(fn):
        with pytest.raises(G.GpvError) as e:
            fn()
        return e.value.status

    assert status(lambda: plan.loglik_grad("matern", [1.3, 0.25, 0.8], TAU)) == 4          # GPV_ERR_UNSUPPORTED_NU
    assert status(lambda: plan.loglik_grad("gauss", [1.3, 0.25, 0.5], TAU)) == 3           # GPV_ERR_COVTYPE
    assert status(lambda: plan.loglik_grad("matern", [1.3, 0.25], TAU)) == 2               # GPV_ERR_BAD_ARG
    assert status(lambda: plan.loglik_grad("matern", cp, 0.0)) == 2
    assert status(lambda: plan.loglik_grad("matern", cp, np.inf)) == 2
    prep = va["U_prep"]
    nodata = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
    assert status(lambda: nodata.loglik_grad(cm, cp, TAU)) == 7                            # GPV_ERR_STATE: no data
    shard = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"], row_begin=0, row_end=150)
    shard.set_data(z)
    assert status(lambda: shard.loglik_grad(cm, cp, TAU)) == 7                             # a row shard
    sgv = G.vecchia_specify(np.array(locs), 10, ordering="none", cond_yz="SGV")
    assert status(lambda: _plan(G, sgv, z).loglik_grad(cm, cp, TAU)) == 7                  # latent neighbours
    wide = G.vecchia_specify(np.array(locs), 64, ordering="none", cond_yz="z")
    assert status(lambda: _plan(G, wide, z).loglik_grad(cm, cp, TAU)) == 5                 # GPV_ERR_UNSUPPORTED_M


# vecchia_estimate(data, locs, m=10, cond_yz='z', output_level=0) of _field() as the commit before this feature returns it
# (default method, smoothness searched), recorded from a run of that commit on an MI355X
_PARENT_DEFAULT = dict(theta_hat=[2.2827292751192765, 0.05742624403455391, 3.3663620460950807, 0.3113773110147149],
                       neg_loglik=1449.349041544677, n_evals=301, convergence=1)


@functools.lru_cache(maxsize=None)
def _field():
    """n = 1500 draws of a Matern-1.5 field (variance 2, range 0.2) plus noise 0.3, by dense Cholesky on the host"""
    rng = np.random.default_rng(2024)
    n = 1500
    locs = rng.random((n, 2))
    r = np.sqrt(((locs[:, None, :] - locs[None, :, :]) ** 2).sum(-1))
    c = np.sqrt(3.0) / 0.2
    S = 2.0 * (1 + c * r) * np.exp(-c * r) + 0.3 * np.eye(n)
    data = np.linalg.cholesky(S) @ rng.standard_normal(n)
    return locs, data


def test_estimation():
    G = _need_gpu()
    locs, data = _field()
    kw = dict(m=10, cond_yz="z", output_level=0)
    nm = G.vecchia_estimate(data, locs, smoothness=1.5, **kw)
    lb = G.vecchia_estimate(data, locs, smoothness=1.5, method="L-BFGS-B", **kw)
    reltol = np.sqrt(np.finfo(float).eps)
    print("Nelder-Mead", nm["neg_loglik"], nm["n_evals"], nm["theta_hat"], "L-BFGS-B", lb["neg_loglik"], lb["n_evals"],
          lb["theta_hat"])
    assert lb["convergence"] == 0
    assert lb["neg_loglik"] <= nm["neg_loglik"] + 100 * reltol * abs(nm["neg_loglik"])
    assert lb["n_evals"] < nm["n_evals"] / 3
    assert len(lb["theta_hat"]) == 3 and len(nm["theta_hat"]) == 3


def test_estimation_default_call_unchanged():
    G = _need_gpu()
    locs, data = _field()
    res = G.vecchia_estimate(data, locs, m=10, cond_yz="z", output_level=0)
    print("default call:", repr(res["theta_hat"].tolist()), repr(res["neg_loglik"]), res["n_evals"], res["convergence"])
    assert res["theta_hat"].tolist() == _PARENT_DEFAULT["theta_hat"]
    assert res["neg_loglik"] == _PARENT_DEFAULT["neg_loglik"]
    assert res["n_evals"] == _PARENT_DEFAULT["n_evals"] and res["convergence"] == _PARENT_DEFAULT["convergence"]
