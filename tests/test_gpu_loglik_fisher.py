"""gpv_plan_loglik_fisher (gpv_fisher_kernel.hpp) on the GPU: value, gradient and expected Fisher information of the cond.yz='z'
log-likelihood, and Fisher scoring on it.

Truth: tests/_fisher_truth.py, a numpy restatement of the DEFINITION of the information (two traces per row; float64 for whole
plans, a long-double Cholesky for single rows) behind the value and gradient of tests/_grad_truth.py.  A row of row_terms is
{l_k, its derivatives, the upper triangle of F_k}.  Tolerances are the project's (tests/test_gpu_loglik_grad.py, tests/_parity.py):
per row |row_terms[k] - truth|_inf <= 1e-8 max(|truth_k|_inf, 1); totals within 1e-8 sum_k |term_k|.

Inputs, shapes and families are those of tests/test_gpu_loglik_grad.py (its SHAPES, FAMILIES, _setup and _field), the smallest
that reach every row-length bucket and its edges.  They are benign: on the CPU the float64 restatement of the whole row stays
within _F64_VS_LD of the long-double one, measured over ALL rows of every (m, d, family) case below (largest figure per family):
    nu0.5 3.2e-14   nu1.5 6.0e-14   nu2.5 1.0e-13   esqe 4.1e-14      coincident points: 2.2e-13      n = 40, m = 39: 1.5e-14
(the triangle alone, scaled by its own rows: 6.1e-14, coincident points 2.4e-13; the form the product computes, restated in
float64: 1.5e-14), so the float64 truth uses less than 1e-4 of the 1e-8 bar; every test that adjudicates rows asserts _F64_VS_LD
again on them.

What each case reaches:
  test_buckets_and_edges        the buckets 16 / 32 / 64 filled exactly and one past an edge, m = 0, ragged first rows, packed
                                records (d <= 3) and coordinates loaded per pair (d = 9), every family; value and gradient
                                against gpv_plan_loglik_grad's on the same plan; symmetry and positive definiteness
  test_more_than_one_set_per_wavefront   n = 40 000: the grid cap gives every wavefront 9 or 10 sets; twice, bitwise
  test_exact_at_full_conditioning        m = n - 1: the information IS that of the multivariate normal
  test_coincident_points        r = 0 pairs off the diagonal
  test_nan_coordinate           failure semantics
  test_state_*                  the plan's last evaluation stays intact; the refusals of gpv_plan_loglik_grad
  test_estimation_fisher        Fisher scoring against L-BFGS-B; standard errors"""
import functools

import numpy as np
import pytest

import _fisher_truth as F
import _grad_truth as T
import test_gpu_loglik_grad as B

pytestmark = pytest.mark.gpu

TOL = B.TOL
TAU = B.TAU
_F64_VS_LD = 1e-12


@functools.lru_cache(maxsize=None)
def _truth(m, d, n, fam, dup=False):
    locs, z, va = B._setup(m, d, n, dup=dup)
    cm, cp = B._family(fam, d)
    t = F.full_rows_f64(va["locsord"], va["U_prep"]["revNNarray"], z, cm, cp, TAU)
    t.setflags(write=False)
    return t


def _check_rows(rows, truth, what):
    err = T.scaled_row_error(rows, truth)
    print(f"{what}: worst row error {err.max():.3e} (row {int(err.argmax())})")
    assert err.max() <= TOL, (what, float(err.max()), int(err.argmax()))


def _check_totals(cm, ll, grad, info, truth, what):
    tot = np.concatenate([[ll], grad, F.tri(info)])
    want, scale = truth.sum(axis=0), np.abs(truth).sum(axis=0)
    keep = ~np.isnan(want)
    assert np.array_equal(np.isnan(tot), ~keep), (what, tot)
    off = np.abs(tot[keep] - want[keep])                   # (m = 0 has no pairs: its range terms and their scale are exact zeros)
    print(f"{what}: totals off by {(off / np.maximum(scale[keep], 1e-300)).max():.3e} of sum |term|")
    assert np.all(off <= TOL * scale[keep]), (what, tot, want)


def _check_matrix(cm, info):
    """exactly symmetric; NaN exactly in the smoothness row and column; positive definite on the differentiated parameters"""
    assert np.array_equal(info, info.T, equal_nan=True)
    pos = F._positions(cm)
    nan = np.ones(info.shape, bool)
    nan[np.ix_(pos, pos)] = False
    assert np.array_equal(np.isnan(info), nan)
    sub = info[np.ix_(pos, pos)]
    ev = np.linalg.eigvalsh(sub)
    print("eigenvalues of the information:", ev)
    assert ev.min() > 0
    np.linalg.cholesky(sub)


@pytest.mark.parametrize("fam", B.FAMILIES)
@pytest.mark.parametrize("m,d", B.SHAPES, ids=["m%d-d%d" % s for s in B.SHAPES])
def test_buckets_and_edges(m, d, fam):
    G = B._need_gpu()
    n = 200 if m == 63 else 300
    locs, z, va = B._setup(m, d, n)
    cm, cp = B._family(fam, d)
    plan = B._plan(G, va, z)
    ll, grad, info, nfail, rows = plan.loglik_fisher(cm, cp, TAU, row_terms=True)
    assert nfail == 0
    truth = _truth(m, d, n, fam)
    assert rows.shape == truth.shape
    _check_rows(rows, truth, "all rows, float64 truth")
    _check_totals(cm, ll, grad, info, truth, "totals")
    if m > 0:                                                 # (m = 0: no pairs, the range has no information)
        _check_matrix(cm, info)
    else:
        assert np.array_equal(info, info.T, equal_nan=True)
    # the adjudicator on 64 seeded rows and the ragged rows in front
    pick = np.union1d(np.arange(min(m + 1, n)), np.random.default_rng(5).choice(n, 64, replace=False))
    revNN = va["U_prep"]["revNNarray"]
    ld = np.stack([F.full_row_ld(va["locsord"], revNN[k], z, cm, cp, TAU) for k in pick])
    f64_err = T.scaled_row_error(truth[pick], ld.astype(np.float64)).max()
    print(f"float64 restatement against long double on these rows: {f64_err:.2e}")
    assert f64_err <= _F64_VS_LD                              # the inputs are benign
    _check_rows(rows[pick], ld.astype(np.float64), "picked rows, long-double truth")
    # value and gradient: those of gpv_plan_loglik_grad on the same plan, within the same bar
    ll_g, grad_g, nfail_g, rows_g = plan.loglik_grad(cm, cp, TAU, row_terms=True)
    nc = T.ncols(cm)
    _check_rows(rows[:, :nc], rows_g, "value and gradient rows against gpv_plan_loglik_grad")
    scale = np.abs(truth[:, :nc]).sum(axis=0)
    keep = ~np.isnan(grad_g)
    assert abs(ll - ll_g) <= TOL * scale[0] and np.all(np.abs(grad - grad_g)[keep] <= TOL * scale[1:][keep])
    assert np.array_equal(np.isnan(grad), ~keep)


def test_more_than_one_set_per_wavefront():
    G = B._need_gpu()
    n, m, d = 40000, 10, 2
    rng = np.random.default_rng(17)
    locs = rng.random((n, d))
    z = rng.standard_normal(n)
    va = G.vecchia_specify(locs, m, ordering="none", cond_yz="z")
    cm, cp = B._family("nu1.5", d)
    plan = B._plan(G, va, z)
    ll, grad, info, nfail, rows = plan.loglik_fisher(cm, cp, TAU, row_terms=True)
    assert nfail == 0
    truth = F.full_rows_f64(va["locsord"], va["U_prep"]["revNNarray"], z, cm, cp, TAU)
    _check_rows(rows, truth, "n = 40 000, all rows")
    _check_totals(cm, ll, grad, info, truth, "n = 40 000 totals")
    _check_matrix(cm, info)
    ll2, grad2, info2, _, rows2 = plan.loglik_fisher(cm, cp, TAU, row_terms=True)
    assert ll2 == ll and np.array_equal(grad2, grad, equal_nan=True) and np.array_equal(info2, info, equal_nan=True)
    assert np.array_equal(rows2, rows, equal_nan=True)


@pytest.mark.parametrize("fam", ("nu1.5", "esqe"))
def test_exact_at_full_conditioning(fam):
    G = B._need_gpu()
    n = 40
    locs, z, va = B._setup(n - 1, 2, n)
    cm, cp = B._family(fam, 2)
    ll, grad, info, nfail = B._plan(G, va, z).loglik_fisher(cm, cp, TAU)
    assert nfail == 0
    dense = F.dense(locs, cm, cp, TAU)
    truth = _truth(n - 1, 2, n, fam)
    nc = T.ncols(cm)
    scale = F.untri(np.abs(truth[:, nc:]).sum(axis=0), F.npar(cm))       # the scale of the totals: sum_k |term_k|
    keep = ~np.isnan(dense)
    assert np.array_equal(np.isnan(info), ~keep)
    print("dense information: off by", (np.abs(info - dense)[keep] / scale[keep]).max(), "of sum |term|")
    assert np.all(np.abs(info - dense)[keep] <= TOL * scale[keep])
    _check_matrix(cm, info)


@pytest.mark.parametrize("fam", ("nu1.5", "esqe"))
@pytest.mark.parametrize("m,d", [(10, 2), (15, 9)], ids=["m10-d2", "m15-d9"])
def test_coincident_points(m, d, fam):
    G = B._need_gpu()
    n = 300
    locs, z, va = B._setup(m, d, n, dup=True)
    cm, cp = B._family(fam, d)
    ll, grad, info, nfail, rows = B._plan(G, va, z).loglik_fisher(cm, cp, TAU, row_terms=True)
    assert nfail == 0
    truth = _truth(m, d, n, fam, dup=True)
    _check_rows(rows, truth, "coincident points, all rows")
    _check_totals(cm, ll, grad, info, truth, "coincident points, totals")
    _check_matrix(cm, info)
    pick = np.random.default_rng(5).choice(n, 64, replace=False)
    revNN = va["U_prep"]["revNNarray"]
    ld = np.stack([F.full_row_ld(va["locsord"], revNN[k], z, cm, cp, TAU) for k in pick])
    f64_err = T.scaled_row_error(truth[pick], ld.astype(np.float64)).max()
    print(f"float64 restatement against long double on these rows: {f64_err:.2e}")
    assert f64_err <= _F64_VS_LD


@pytest.mark.parametrize("m,d", [(10, 2), (15, 9)], ids=["m10-d2", "m15-d9"])
def test_nan_coordinate(m, d):
    G = B._need_gpu()
    n, bad = 300, 150
    locs, z, va = B._setup(m, d, n)
    cm, cp = B._family("nu1.5", d)
    poisoned = np.array(va["locsord"])
    poisoned[bad, d - 1] = np.nan                           # the LAST coordinate
    ll, grad, info, nfail, rows = B._plan(G, va, z, locs=poisoned).loglik_fisher(cm, cp, TAU, row_terms=True)
    revNN = va["U_prep"]["revNNarray"]
    hit = np.array([bad in T.valid_entries(revNN[k]) for k in range(n)])
    assert hit.sum() >= 1 and nfail == hit.sum()
    assert ll == -np.inf and np.all(np.isnan(grad)) and np.all(np.isnan(info))
    assert np.all(np.isnan(rows[hit]))
    _check_rows(rows[~hit], _truth(m, d, n, "nu1.5")[~hit], "rows away from the NaN coordinate")


def test_state_last_evaluation_stays_intact():
    G = B._need_gpu()
    locs, z, va = B._setup(10, 2, 300)
    cm, cp = B._family("nu1.5", 2)
    plan = B._plan(G, va, z)
    plan.eval(cm, cp, TAU, G.GPV_WANT_U | G.GPV_WANT_LOGLIK_Z)
    sums, Lent, stamp = plan.sums(), plan.Lentries(), plan.factor_stamp()
    ll, grad, info, nfail = plan.loglik_fisher(cm, [0.9, 0.2, 2.5], 0.3)      # other parameters than the evaluation's
    assert nfail == 0 and np.isfinite(ll)
    assert np.array_equal(plan.sums(), sums) and np.array_equal(plan.Lentries(), Lent) and plan.factor_stamp() == stamp


def test_state_refusals():
    G = B._need_gpu()
    locs, z, va = B._setup(10, 2, 300)
    cm, cp = B._family("nu1.5", 2)
    plan = B._plan(G, va, z)

    def status(fn):
        with pytest.raises(G.GpvError) as e:
            fn()
        return e.value.status

    assert status(lambda: plan.loglik_fisher("matern", [1.3, 0.25, 0.8], TAU)) == 4          # GPV_ERR_UNSUPPORTED_NU
    assert status(lambda: plan.loglik_fisher("gauss", [1.3, 0.25, 0.5], TAU)) == 3           # GPV_ERR_COVTYPE
    assert status(lambda: plan.loglik_fisher("matern", [1.3, 0.25], TAU)) == 2               # GPV_ERR_BAD_ARG
    assert status(lambda: plan.loglik_fisher("matern", cp, 0.0)) == 2
    assert status(lambda: plan.loglik_fisher("matern", cp, np.inf)) == 2
    prep = va["U_prep"]
    nodata = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
    assert status(lambda: nodata.loglik_fisher(cm, cp, TAU)) == 7                            # GPV_ERR_STATE: no data
    shard = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"], row_begin=0, row_end=150)
    shard.set_data(z)
    assert status(lambda: shard.loglik_fisher(cm, cp, TAU)) == 7                             # a row shard
    sgv = G.vecchia_specify(np.array(locs), 10, ordering="none", cond_yz="SGV")
    assert status(lambda: B._plan(G, sgv, z).loglik_fisher(cm, cp, TAU)) == 7                # latent neighbours
    wide = G.vecchia_specify(np.array(locs), 64, ordering="none", cond_yz="z")
    assert status(lambda: B._plan(G, wide, z).loglik_fisher(cm, cp, TAU)) == 5               # GPV_ERR_UNSUPPORTED_M


def test_estimation_fisher():
    G = B._need_gpu()
    locs, data = B._field()
    kw = dict(m=10, cond_yz="z", output_level=0)
    lb = G.vecchia_estimate(data, locs, smoothness=1.5, method="L-BFGS-B", **kw)
    fs = G.vecchia_estimate(data, locs, smoothness=1.5, method="fisher", **kw)
    reltol = np.sqrt(np.finfo(float).eps)
    print("L-BFGS-B", lb["neg_loglik"], lb["n_evals"], lb["theta_hat"], "fisher", fs["neg_loglik"], fs["n_evals"], fs["theta_hat"],
          "se", fs["theta_se"])
    assert fs["convergence"] == 0
    assert fs["neg_loglik"] <= lb["neg_loglik"] + 100 * reltol * abs(lb["neg_loglik"])
    assert fs["n_evals"] <= lb["n_evals"]
    assert len(fs["theta_hat"]) == 3
    assert not any(k in lb for k in ("fisher_info", "theta_cov", "theta_se"))
    # the standard errors: a fresh information at theta_hat (the calls are bitwise reproducible)
    va = G.vecchia_specify(locs, 10, cond_yz="z")
    th = fs["theta_hat"]
    ll, g, info = G.vecchia_likelihood_fisher(fs["z"], va, [th[0], th[1], 1.5], th[2])
    sub = np.delete(np.delete(info, 2, axis=0), 2, axis=1)
    assert abs(-ll - fs["neg_loglik"]) <= 1e-12 * abs(ll)
    assert np.allclose(fs["fisher_info"], sub, rtol=1e-12, atol=0)
    assert np.allclose(fs["theta_cov"], np.linalg.inv(sub), rtol=1e-9, atol=0)
    assert np.allclose(fs["theta_se"], np.sqrt(np.diag(np.linalg.inv(sub))), rtol=1e-9, atol=0)
