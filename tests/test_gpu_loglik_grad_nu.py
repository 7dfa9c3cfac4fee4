"""gpv_plan_loglik_grad_nu / gpv_plan_loglik_fisher_nu on the GPU: value, gradient and expected Fisher information of the cond.yz='z'
log-likelihood under the general-nu Matern covariance, the smoothness differentiated (gpv_grad.hip, gpv_fisher_kernel.hpp with
COV_MATERN_GEN; the pair functions and their per-call tables: gpv_bessel.hpp, gpv_matern_dtab_kernel).

Truth: tests/_grad_nu_truth.py (bulk: numpy float64 with scipy's K_nu and an own quadrature of dK_nu/dnu; adjudicator: every pair
function from 40-digit mpmath, mpmath.diff in the order, long-double Cholesky).  Rows are {l_k, d/d variance, d/d range,
d/d smoothness, d/d nugget, the 10 entries of the information's upper triangle}.  Tolerances are the project's flat bar: per row
1e-8 max(|truth_k|_inf, 1), totals 1e-8 sum_k |term_k|.  Under cond.yz='z' the nugget bounds every block's condition number by
(p sigma^2 + tau) / tau < 1e3, so the bar has room.  Every test that adjudicates rows asserts again that the bulk truth is within
_F64_VS_ADJ = 1e-12 (1e-4 of the bar) of the adjudicator there.

Inputs follow tests/test_gpu_loglik_grad.py (its _setup): seeded uniform locations, tau = 0.1, range 0.25 sqrt(d / 2),
ordering="none", exact neighbours from the oracle, n = 600.

  test_buckets_and_edges        (m, d) in {(0,2), (10,2), (31,2), (40,3), (15,9)} x nu in {0.3 (n_up = 0, the K_(1-nu) weight),
                                0.8 (mu < 0), 2.2 (the recurrence)}: gradient rows and information rows, totals
  test_table_against_direct     range 1e-4 (most pairs beyond the table and in underflow) and range 50 (tiny s); the route with
                                GPV_NO_MATERN_TABLE (quadrature per pair) against the tables
  test_coincident_points        r = 0 pairs off the diagonal: derivatives 1, 0, 0
  test_more_than_one_set_per_wavefront   n = 6000, twice, bitwise
  test_against_existing_path    value against GPV_WANT_LOGLIK_Z, range and smoothness derivatives against its central differences
  test_closed_forms_and_esqe    the new entries return the old entries' bits; the old entries still refuse a general smoothness
  test_state                    the plan's last evaluation stays intact
  test_estimation               L-BFGS-B and Fisher scoring with a FREE smoothness against Nelder-Mead over the same four

Worst row error measured on an MI355X (of the 1e-8 bar): see DESIGN.md 4j."""
import functools

import numpy as np
import pytest

import _grad_nu_truth as N
import _grad_truth as T
import test_gpu_loglik_grad as B

pytestmark = pytest.mark.gpu

TOL = 1e-8
TAU = 0.1
N_ROWS = 600
SHAPES = [(0, 2), (10, 2), (31, 2), (40, 3), (15, 9)]
NUS = (0.3, 0.8, 2.2)
_F64_VS_ADJ = 1e-12


@functools.lru_cache(maxsize=None)
def _setup(m, d, n, dup=False):
    """The inputs of test_gpu_loglik_grad._setup.  With coincident points at n = 600 a point can have more than m earlier points
    at distance 0, and the oracle's neighbour row then need not hold the point itself, which that helper assumes: here the point
    goes in front and the last of the (equally near) others leaves."""
    if not dup:
        return B._setup(m, d, n)
    G = B._need_gpu()
    from oracle import r_side as R
    rng = np.random.default_rng(11)
    locs = rng.random((n, d))
    z = rng.standard_normal(n)
    for j in range(2, n, 3):                                       # every third point sits on an earlier one
        locs[j] = locs[rng.integers(j)]
    NN = R.findOrderedNN(locs, m)
    for j in np.where(NN[:, 0] != np.arange(1, n + 1))[0]:
        at = np.where(NN[j] == j + 1)[0]
        if len(at):
            NN[j, 0], NN[j, at[0]] = NN[j, at[0]], NN[j, 0]
        else:
            NN[j, 1:] = NN[j, :-1].copy()
            NN[j, 0] = j + 1
    NN = np.nan_to_num(NN, nan=0.0).astype(np.int32)
    va = G.vecchia_specify(locs, m, ordering="none", cond_yz="z", NNarray=NN)
    for a in (locs, z, va["locsord"], va["U_prep"]["revNNarray"], va["U_prep"]["revCond"]):
        a.setflags(write=False)
    return locs, z, va


def _cp(d, nu, rng_=None):
    return [1.3, B._range_rule(d) if rng_ is None else rng_, nu]


@functools.lru_cache(maxsize=None)
def _truth(m, d, n, nu, rng_=None, dup=False, form=False):
    locs, z, va = _setup(m, d, n, dup=dup)
    t = N.full_rows_f64(va["locsord"], va["U_prep"]["revNNarray"], z, _cp(d, nu, rng_), TAU, form=form)
    t.setflags(write=False)
    return t


def _check_rows(rows, truth, what):
    err = N.scaled_row_error(rows, truth)
    print(f"{what}: worst row error {err.max():.3e} (row {int(err.argmax())})")
    assert err.max() <= TOL, (what, float(err.max()), int(err.argmax()))


def _check_totals(tot, truth, what):
    """tot: the call's totals in the column order of truth"""
    want, scale = truth.sum(axis=0), np.abs(truth).sum(axis=0)
    assert np.all(np.isfinite(tot)), (what, tot)
    off = np.abs(tot - want)
    print(f"{what}: totals off by {(off / np.maximum(scale, 1e-300)).max():.3e} of sum |term|")
    assert np.all(off <= TOL * scale), (what, tot, want)


def _adjudicate(va, z, cp, truth, rows, pick, what):
    revNN = va["U_prep"]["revNNarray"]
    adj = np.stack([N.row_adj(va["locsord"], revNN[k], z, cp, TAU) for k in pick]).astype(np.float64)
    gap = N.scaled_row_error(truth[pick], adj).max()
    print(f"{what}: bulk truth against the adjudicator on {len(pick)} rows: {gap:.2e}")
    assert gap <= _F64_VS_ADJ
    _check_rows(rows[pick], adj, what + ", adjudicated rows")


def _both(plan, cp):
    """(rows of the gradient call, rows of the information call, totals of the information call in truth's column order)"""
    ll, grad, nfail, rows_g = plan.loglik_grad("matern", cp, TAU, row_terms=True, smoothness_grad=True)
    assert nfail == 0 and np.all(np.isfinite(grad)) and np.isfinite(ll)
    ll2, grad2, info, nfail2, rows_f = plan.loglik_fisher("matern", cp, TAU, row_terms=True, smoothness_grad=True)
    assert nfail2 == 0 and np.all(np.isfinite(info))
    assert np.array_equal(info, info.T)
    tot_g = np.concatenate([[ll], grad])
    tot_f = np.concatenate([[ll2], grad2, [info[i, j] for i in range(4) for j in range(i, 4)]])
    return rows_g, rows_f, tot_g, tot_f


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("m,d", SHAPES, ids=["m%d-d%d" % s for s in SHAPES])
def test_buckets_and_edges(m, d, nu):
    G = B._need_gpu()
    locs, z, va = B._setup(m, d, N_ROWS)
    cp = _cp(d, nu)
    rows_g, rows_f, tot_g, tot_f = _both(B._plan(G, va, z), cp)
    truth = _truth(m, d, N_ROWS, nu)
    assert rows_g.shape == (N_ROWS, 5) and rows_f.shape == (N_ROWS, 15)
    _check_rows(rows_g, truth[:, :5], "gradient rows")
    _check_rows(rows_f, truth, "information rows")
    _check_totals(tot_g, truth[:, :5], "gradient totals")
    _check_totals(tot_f, truth, "information totals")
    # the adjudicator: the ragged rows in front (up to 11 entries) and, where whole rows are that short, 6 seeded ones
    pick = np.arange(min(m, 10) + 1)
    if m <= 10:
        pick = np.union1d(pick, np.random.default_rng(5).choice(N_ROWS, 6, replace=False))
    _adjudicate(va, z, cp, truth, rows_f, pick, "information rows")


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("rng_", (1e-4, 50.0), ids=["range1e-4", "range50"])
def test_table_against_direct(rng_, nu, monkeypatch):
    G = B._need_gpu()
    m, d = 10, 2
    locs, z, va = B._setup(m, d, N_ROWS)
    cp = _cp(d, nu, rng_)
    plan = B._plan(G, va, z)
    truth = _truth(m, d, N_ROWS, nu, rng_, form=True)
    monkeypatch.delenv("GPV_NO_MATERN_TABLE", raising=False)
    rows_g, rows_f, tot_g, tot_f = _both(plan, cp)
    assert np.all(np.isfinite(rows_g)) and np.all(np.isfinite(rows_f))
    _check_rows(rows_g, truth[:, :5], "tables, gradient rows")
    _check_rows(rows_f, truth, "tables, information rows")
    _check_totals(tot_f, truth, "tables, information totals")
    pick = np.union1d(np.arange(11), np.random.default_rng(5).choice(N_ROWS, 6, replace=False))
    _adjudicate(va, z, cp, truth, rows_f, pick, "tables")
    monkeypatch.setenv("GPV_NO_MATERN_TABLE", "1")                # the library reads it at every call
    drows_g, drows_f, dtot_g, dtot_f = _both(plan, cp)
    _check_rows(drows_g, truth[:, :5], "quadrature per pair, gradient rows")
    _check_rows(drows_f, truth, "quadrature per pair, information rows")
    _check_rows(drows_f, rows_f, "quadrature per pair against the tables")
    _check_totals(dtot_f, truth, "quadrature per pair, information totals")


@pytest.mark.parametrize("nu", NUS)
def test_direct_route_at_the_tests_range(nu, monkeypatch):
    G = B._need_gpu()
    m, d = 10, 2
    locs, z, va = B._setup(m, d, N_ROWS)
    cp = _cp(d, nu)
    monkeypatch.setenv("GPV_NO_MATERN_TABLE", "1")
    rows_g, rows_f, tot_g, tot_f = _both(B._plan(G, va, z), cp)
    truth = _truth(m, d, N_ROWS, nu)
    _check_rows(rows_g, truth[:, :5], "quadrature per pair, gradient rows")
    _check_rows(rows_f, truth, "quadrature per pair, information rows")


@pytest.mark.parametrize("nu", NUS)
def test_coincident_points(nu):
    G = B._need_gpu()
    m, d = 10, 2
    locs, z, va = _setup(m, d, N_ROWS, dup=True)
    cp = _cp(d, nu)
    rows_g, rows_f, tot_g, tot_f = _both(B._plan(G, va, z), cp)
    truth = _truth(m, d, N_ROWS, nu, dup=True)                   # (its r = 0 pairs are 1, 0, 0 by definition)
    revNN = va["U_prep"]["revNNarray"]
    has_dup = [k for k in range(N_ROWS)
               if len(np.unique(va["locsord"][T.valid_entries(revNN[k])], axis=0)) < len(T.valid_entries(revNN[k]))]
    assert len(has_dup) > 50
    _check_rows(rows_g, truth[:, :5], "coincident points, gradient rows")
    _check_rows(rows_f, truth, "coincident points, information rows")
    _check_totals(tot_f, truth, "coincident points, totals")
    _adjudicate(va, z, cp, truth, rows_f, np.array(has_dup[:8]), "coincident points")


def test_more_than_one_set_per_wavefront():
    G = B._need_gpu()
    n, m, d, nu = 6000, 10, 2, 0.8
    rng = np.random.default_rng(17)
    locs = rng.random((n, d))
    z = rng.standard_normal(n)
    va = G.vecchia_specify(locs, m, ordering="none", cond_yz="z")
    cp = _cp(d, nu)
    plan = B._plan(G, va, z)
    rows_g, rows_f, tot_g, tot_f = _both(plan, cp)
    truth = N.full_rows_f64(va["locsord"], va["U_prep"]["revNNarray"], z, cp, TAU)
    _check_rows(rows_g, truth[:, :5], "n = 6000, gradient rows")
    _check_rows(rows_f, truth, "n = 6000, information rows")
    _check_totals(tot_g, truth[:, :5], "n = 6000, gradient totals")
    _check_totals(tot_f, truth, "n = 6000, information totals")
    rows_g2, rows_f2, tot_g2, tot_f2 = _both(plan, cp)
    assert np.array_equal(rows_g2, rows_g) and np.array_equal(rows_f2, rows_f)
    assert np.array_equal(tot_g2, tot_g) and np.array_equal(tot_f2, tot_f)


def test_against_existing_path():
    G = B._need_gpu()
    n, m, d, nu = 1000, 10, 2, 0.8
    locs, z, va = B._setup(m, d, n)
    cp = _cp(d, nu)
    plan = B._plan(G, va, z)
    ll, grad, nfail, rows = plan.loglik_grad("matern", cp, TAU, row_terms=True, smoothness_grad=True)
    assert nfail == 0
    scale = np.abs(rows).sum(axis=0)                              # sum_k |term_k| per column

    def existing(cp_):
        plan.eval("matern", cp_, TAU, G.GPV_WANT_LOGLIK_Z)
        return G.loglik_z_from_sums(plan.sums(), n)

    ll0 = existing(cp)
    print("value: gradient entry", ll, "existing path", ll0, "off", abs(ll - ll0) / scale[0], "of sum |term|")
    assert abs(ll - ll0) <= TOL * scale[0]
    for i in (1, 2):                                              # range, smoothness
        h = 1e-5 * cp[i]
        tp, tm = list(cp), list(cp)
        tp[i] += h
        tm[i] -= h
        cd = (existing(tp) - existing(tm)) / (tp[i] - tm[i])
        print("component", i, "analytic", grad[i], "central difference", cd, "off", abs(cd - grad[i]) / scale[1 + i], "of sum |term|")
        assert abs(cd - grad[i]) <= 1e-6 * scale[1 + i]


def test_closed_forms_and_esqe():
    G = B._need_gpu()
    locs, z, va = B._setup(10, 2, N_ROWS)
    plan = B._plan(G, va, z)
    for fam in B.FAMILIES:
        cm, cp = B._family(fam, 2)
        old = plan.loglik_grad(cm, cp, TAU, row_terms=True)
        new = plan.loglik_grad(cm, cp, TAU, row_terms=True, smoothness_grad=True)
        assert old[0] == new[0] and old[2] == new[2]
        assert np.array_equal(old[1], new[1], equal_nan=True) and np.array_equal(old[3], new[3], equal_nan=True)
        assert np.isnan(new[1][2]) == (cm == "matern")
        old = plan.loglik_fisher(cm, cp, TAU, row_terms=True)
        new = plan.loglik_fisher(cm, cp, TAU, row_terms=True, smoothness_grad=True)
        assert old[0] == new[0] and old[3] == new[3]
        for a, b in ((old[1], new[1]), (old[2], new[2]), (old[4], new[4])):
            assert np.array_equal(a, b, equal_nan=True)
        assert bool(np.all(np.isnan(new[2][2]))) == (cm == "matern")
    for call in (plan.loglik_grad, plan.loglik_fisher):           # the old entries still refuse a general smoothness
        with pytest.raises(G.GpvError) as e:
            call("matern", [1.3, 0.25, 0.8], TAU)
        assert e.value.status == 4
        with pytest.raises(G.GpvError) as e:                     # and the new ones what no entry accepts
            call("matern", [1.3, 0.25, 61.0], TAU, smoothness_grad=True)
        assert e.value.status == 4


def test_state_last_evaluation_stays_intact():
    G = B._need_gpu()
    locs, z, va = B._setup(10, 2, N_ROWS)
    plan = B._plan(G, va, z)
    plan.eval("matern", [1.3, 0.25, 0.8], TAU, G.GPV_WANT_U | G.GPV_WANT_LOGLIK_Z)
    sums, Lent, stamp = plan.sums(), plan.Lentries(), plan.factor_stamp()
    ll, grad, nfail = plan.loglik_grad("matern", [0.9, 0.2, 1.1], 0.3, smoothness_grad=True)
    assert nfail == 0 and np.isfinite(ll)
    assert np.array_equal(plan.sums(), sums) and np.array_equal(plan.Lentries(), Lent) and plan.factor_stamp() == stamp
    ll, grad, info, nfail = plan.loglik_fisher("matern", [0.9, 0.2, 1.1], 0.3, smoothness_grad=True)
    assert nfail == 0 and np.isfinite(ll)
    assert np.array_equal(plan.sums(), sums) and np.array_equal(plan.Lentries(), Lent) and plan.factor_stamp() == stamp


@functools.lru_cache(maxsize=None)
def _field():
    """n = 1500 draws of the general-nu Matern field (variance 2, range 0.1, smoothness 0.8) plus noise 0.3, by dense Cholesky"""
    rng = np.random.default_rng(2025)
    n = 1500
    locs = rng.random((n, 2))
    r = np.sqrt(((locs[:, None, :] - locs[None, :, :]) ** 2).sum(-1))
    C, _ = N.cov_and_derivs(r, [2.0, 0.1, 0.8])
    data = np.linalg.cholesky(C + 0.3 * np.eye(n)) @ rng.standard_normal(n)
    return locs, data


def test_estimation():
    G = B._need_gpu()
    locs, data = _field()
    kw = dict(m=10, cond_yz="z", output_level=0)                  # (maxmin ordering is the default)
    nm = G.vecchia_estimate(data, locs, **kw)                     # the reference's search over the same four parameters
    lb = G.vecchia_estimate(data, locs, method="L-BFGS-B", smoothness_grad=True, **kw)
    fs = G.vecchia_estimate(data, locs, method="fisher", smoothness_grad=True, **kw)
    reltol = np.sqrt(np.finfo(float).eps)
    print("Nelder-Mead", nm["neg_loglik"], nm["n_evals"], nm["theta_hat"])
    print("L-BFGS-B   ", lb["neg_loglik"], lb["n_evals"], lb["theta_hat"])
    print("fisher     ", fs["neg_loglik"], fs["n_evals"], fs["theta_hat"], "se", fs["theta_se"])
    allow = 100 * reltol * abs(nm["neg_loglik"])
    assert len(nm["theta_hat"]) == 4 and len(lb["theta_hat"]) == 4 and len(fs["theta_hat"]) == 4
    assert lb["neg_loglik"] <= nm["neg_loglik"] + allow
    assert fs["neg_loglik"] <= nm["neg_loglik"] + allow
    assert 0.01 < lb["theta_hat"][2] <= 10.0
    se, info = fs["theta_se"], fs["fisher_info"]
    assert se.shape == (4,) and np.all(np.isfinite(se)) and np.all(se > 0)
    assert info.shape == (4, 4) and np.array_equal(info, info.T) and np.all(np.linalg.eigvalsh(info) > 0)
