"""Likelihood-only launches (no U row, no compact block, no a vector) run the lower-triangle LDL^T sweep of the set kernel
(gpv_sets_kernel<P, D, COV, true>, m + 1 = 21, 26, 31); a launch that also asks for GPV_WANT_U keeps the Gauss-Jordan
sweep.  Same plan, two routes: the sums must agree to rounding, the failed sets exactly, and both must follow the oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLAGS = 2 | 4              # GPV_WANT_LOGLIK_Z | GPV_WANT_NUMERATOR: every sum of the fused epilogue
RTOL = 1e-12


def _need_gpu():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


def _case(n, m, d, seed, dup=0, nan_at=None):
    from oracle import r_side as R
    rng = np.random.default_rng(seed)
    locs = rng.random((n, d))
    if dup:                                                  # coincident points: dist == 0 inside many blocks
        at = rng.choice(np.arange(1, n), size=dup, replace=False)
        locs[at] = locs[at - 1]
    z = rng.standard_normal(n)
    va = R.vecchia_specify(locs, m, ordering="none", cond_yz="z")
    if nan_at is not None:                                   # a NaN coordinate: NaN blocks, which must fail
        va["locsord"] = va["locsord"].copy()
        va["locsord"][nan_at, 0] = np.nan
    prep = va["U_prep"]
    G = _need_gpu()
    plan = G.Plan(va["locsord"], np.nan_to_num(prep["revNNarray"], nan=0.0).astype(np.int32),
                  np.nan_to_num(prep["revCond"], nan=-1.0).astype(np.int8))
    plan.set_data(z[va["ord_z"] - 1])
    return z, va, plan


def _params(covmodel, nu, d):
    rg = 0.2 * np.sqrt(d) if d > 1 else 0.02
    if covmodel == "esqe":
        return [0.9, rg, 0.4, 0.5 * rg]
    return [1.3, rg, nu]


def _two_routes(plan, covmodel, cp, tau):
    G = _need_gpu()
    plan.eval(covmodel, cp, tau, FLAGS)                      # likelihood only: lower-triangle sweep
    s_lik = plan.sums()
    plan.eval(covmodel, cp, tau, FLAGS | G.GPV_WANT_U)       # U rows written: Gauss-Jordan
    s_gj = plan.sums()
    return s_lik, s_gj


def _assert_same(a, b, rtol=RTOL):
    for q in range(8):
        x, y = a[q], b[q]
        if not (np.isfinite(x) and np.isfinite(y)):
            assert (np.isnan(x) and np.isnan(y)) or x == y, (q, x, y)
            continue
        assert abs(x - y) <= rtol * max(abs(x), abs(y)), (q, x, y, abs(x - y) / max(abs(x), abs(y)))


def _ll(s, n):
    G = _need_gpu()
    return G.loglik_z_from_sums(s, n)


@pytest.mark.parametrize("cov", [("matern", 0.5), ("matern", 1.5), ("matern", 2.5), ("matern", 1.1), ("esqe", None)])
@pytest.mark.parametrize("d", [1, 2, 3, 5])
@pytest.mark.parametrize("m", [15, 20, 25, 27, 30])
def test_lik_sweep_matches_gauss_jordan(m, d, cov):
    n = 1200
    z, va, plan = _case(n, m, d, 100 * m + d)
    cp = _params(cov[0], cov[1], d)
    for tau in (np.array([0.1]), 0.05 + np.random.default_rng(m).random(n)[va["ord"] - 1]):
        s_lik, s_gj = _two_routes(plan, cov[0], cp, tau)
        assert s_lik[6] == s_gj[6] == 0 and s_lik[7] == s_gj[7] == n
        _assert_same(s_lik, s_gj)
        ll, ll_gj = _ll(s_lik, n), _ll(s_gj, n)
        assert abs(ll - ll_gj) <= RTOL * abs(ll_gj)


@pytest.mark.parametrize("m", [20, 30])
def test_lik_sweep_edge_cases_against_oracle(m):
    """Sets with missing neighbours (the first m rows of every plan), coincident points, a zero nugget, blocks that are not
    positive definite (a negative nugget, a NaN coordinate: they fail), infinite nuggets.  (Exactly singular blocks, a zero
    nugget WITH coincident points, are left out: their last pivot is rounding noise of either sign on any route.)"""
    from oracle import r_side as R
    n = 900
    cp = [1.0, 0.15, 1.5]
    z, va, plan = _case(n, m, 2, 11 + m, dup=40)
    s_lik, s_gj = _two_routes(plan, "matern", cp, np.array([0.1]))
    ref = R.createU(va, cp, 0.1)
    assert s_lik[6] == s_gj[6] == ref["U_entries"]["n_failed"] == 0
    _assert_same(s_lik, s_gj)
    ll_ref = R.vecchia_likelihood_U(z, ref)
    assert abs(_ll(s_lik, n) - ll_ref) <= 1e-8 * abs(ll_ref)
    z, va, plan = _case(n, m, 2, 12 + m)
    s_lik, s_gj = _two_routes(plan, "matern", cp, np.array([0.0]))
    ref = R.createU(va, cp, 0.0)
    assert s_lik[6] == s_gj[6] == ref["U_entries"]["n_failed"]
    # negative nuggets on some rows: every set that holds one of them as an observation fails
    tau = np.full(n, 0.1)
    tau[5::61] = -3.0
    s_lik, s_gj = _two_routes(plan, "matern", cp, tau[va["ord"] - 1])
    ref = R.createU(va, cp, tau)
    assert s_lik[6] == s_gj[6] == ref["U_entries"]["n_failed"] > 0
    # infinite nuggets on some rows: the diagonal is clamped the same way on both routes
    tau = np.full(n, 0.2)
    tau[::97] = np.inf
    s_lik, s_gj = _two_routes(plan, "matern", cp, tau[va["ord"] - 1])
    assert s_lik[6] == s_gj[6] and s_lik[7] == s_gj[7] == n
    _assert_same(s_lik, s_gj)
    # NaN coordinate: every set that contains the point fails, on both routes and in the oracle
    z, va, plan = _case(n, m, 2, 13 + m, nan_at=n // 2)
    s_lik, s_gj = _two_routes(plan, "matern", cp, np.array([0.1]))
    ref = R.createU(va, cp, 0.1)
    assert s_lik[6] == s_gj[6] == ref["U_entries"]["n_failed"] >= 1


def test_lik_sweep_ill_conditioned_blocks():
    """nu = 2.5, range 0.3: smooth, strongly correlated blocks.  The lower-triangle sweep's log-likelihood must be as close to
    the oracle's as the Gauss-Jordan route's (both are backward stable; a factor of 2 covers which of the two roundings
    happens to land nearer)."""
    from oracle import r_side as R
    n, m = 1500, 30
    cp = [1.0, 0.3, 2.5]
    z, va, plan = _case(n, m, 2, 31)
    for tau in (1e-2, 1e-4):
        s_lik, s_gj = _two_routes(plan, "matern", cp, np.array([tau]))
        ref = R.createU(va, cp, tau)
        assert s_lik[6] == s_gj[6] == ref["U_entries"]["n_failed"]
        ll_ref = R.vecchia_likelihood_U(z, ref)
        e_lik, e_gj = abs(_ll(s_lik, n) - ll_ref), abs(_ll(s_gj, n) - ll_ref)
        assert e_lik <= 2.0 * e_gj + 1e-13 * abs(ll_ref), (tau, e_lik, e_gj, ll_ref)
