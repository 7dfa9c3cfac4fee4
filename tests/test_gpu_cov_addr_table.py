"""The likelihood-only set kernels (gpv_sets_kernel<P, D, COV, true>, m + 1 = 21, 26, 31) keep the LDS addresses at which
their covariance rounds stage every pair in registers for the whole task loop (k_cov_addr_table): one table per wavefront,
worked out before its first task.  A launch that also asks for GPV_WANT_U runs the Gauss-Jordan kernel, which derives each
address per pair as before.  Same plan, two routes: the sums must agree to rounding and the failed sets exactly; both must
follow the oracle; a table that were right for a wavefront's first task only, or that depended on how the tasks are dealt to
the wavefronts, would show at the row counts chosen here.

Task layout (4 sets per task at these row lengths; a 256-CU device holds 512 workgroups = 2048 wavefronts): up to 8192 rows
every wavefront takes at most one task, at 20 000 rows two or three, and from 49 152 rows (6 tasks per wavefront slot) the
older wavefront of a SIMD takes two task slots per round and the younger one (2 : 1 shares)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLAGS = 2 | 4              # GPV_WANT_LOGLIK_Z | GPV_WANT_NUMERATOR: every sum of the fused epilogue
RTOL = 1e-12               # two routes, same plan (tests/test_gpu_lik_sweep.py)
LL_RTOL = 1e-8             # log-likelihood against the oracle (tests/test_gpu_lik_sweep.py)


def _need_gpu():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


def _plan_of(va):
    G = _need_gpu()
    prep = va["U_prep"]
    return G.Plan(va["locsord"], np.nan_to_num(prep["revNNarray"], nan=0.0).astype(np.int32),
                  np.nan_to_num(prep["revCond"], nan=-1.0).astype(np.int8))


@functools.lru_cache(maxsize=None)
def _case(n, m, d, seed, dup=0, nan_at=None):
    """Plan built the way tests/test_gpu_lik_sweep.py builds it: the oracle's specification, ordering 'none' (the first m
    sets have missing neighbours: padded sets and complete ones in one launch), response-first conditioning."""
    from oracle import r_side as R
    rng = np.random.default_rng(seed)
    locs = rng.random((n, d))
    if dup:                                                  # coincident points: dist == 0 inside many blocks
        at = rng.choice(np.arange(1, n), size=dup, replace=False)
        locs[at] = locs[at - 1]
    z = rng.standard_normal(n)
    NN = None
    if dup:
        # A point and its coincident twin are both at distance 0, and the oracle's stable sort then lists the earlier twin
        # in front of the row's own point: such a row would describe the twin's set, not its own, and the oracle's two
        # log-likelihood routes disagree on it.  Ties are the neighbour search's to break (oracle/r_side.py, findOrderedNN:
        # "up to tie-breaking"): here every row leads with itself, as the plan layout requires.
        NN = R.findOrderedNN(locs, m)
        for k in np.where(NN[:, 0] != np.arange(1, n + 1))[0]:
            at_self = int(np.where(NN[k] == k + 1)[0][0])
            NN[k, 1: at_self + 1] = NN[k, :at_self]
            NN[k, 0] = k + 1
    va = R.vecchia_specify(locs, m, ordering="none", cond_yz="z", NNarray=NN)
    if nan_at is not None:                                   # a NaN coordinate: NaN blocks, which must fail
        va["locsord"] = va["locsord"].copy()
        va["locsord"][nan_at, 0] = np.nan
    plan = _plan_of(va)
    plan.set_data(z[va["ord_z"] - 1])
    return z, va, plan


@functools.lru_cache(maxsize=None)
def _raw_case(n, m, seed):
    """n rows of row length m + 1 whatever n is (n = 3 keeps the 31-column kernel): neighbour arrays straight from the
    definition, 2-D, every neighbour conditioned on as an observation; with the oracle's entries and log-likelihood."""
    from gpvecchia_amd import specify as S
    from oracle import r_side as R
    G = _need_gpu()
    rng = np.random.default_rng(seed)
    locs = rng.random((n, 2))
    z = rng.standard_normal(n)
    revNN = S.find_ordered_nn(locs, m)[:, ::-1].copy()
    revCond = np.where(revNN != 0, 0, -1).astype(np.int8)
    revCond[:, -1] = 1
    plan = G.Plan(locs, revNN, revCond)
    plan.set_data(z)
    cp, tau = [1.0, 0.05, 1.5], 0.1
    ref = R.U_NZentries(R.max_threads(), n, locs, revNN, np.where(revCond < 0, 0, revCond).astype(np.float64),
                        np.full(n, tau), np.full(n, tau), "matern", cp)
    ll_ref, _ = R.separable_sums_condz_vectorised(revNN, ref["Lentries"], z, tau)
    return plan, cp, tau, int(ref["n_failed"]), float(ll_ref)


def _params(covmodel, nu, d):
    rg = 0.2 * np.sqrt(d) if d > 1 else 0.02
    if covmodel == "esqe":
        return [0.9, rg, 0.4, 0.5 * rg]
    return [1.3, rg, nu]


def _two_routes(plan, covmodel, cp, tau):
    G = _need_gpu()
    plan.eval(covmodel, cp, tau, FLAGS)                      # likelihood only: address table
    s_lik = plan.sums()
    plan.eval(covmodel, cp, tau, FLAGS | G.GPV_WANT_U)       # U rows written: Gauss-Jordan, addresses per pair
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
    return _need_gpu().loglik_z_from_sums(s, n)


@pytest.mark.parametrize("cov", [("matern", 0.5), ("matern", 1.5), ("matern", 2.5), ("matern", 1.1), ("esqe", None)])
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("m", [20, 25, 30])
def test_table_route_matches_gauss_jordan(m, d, cov):
    n = 4000
    z, va, plan = _case(n, m, d, 200 * m + d)
    s_lik, s_gj = _two_routes(plan, cov[0], _params(cov[0], cov[1], d), np.array([0.1]))
    assert s_lik[6] == s_gj[6] == 0 and s_lik[7] == s_gj[7] == n
    _assert_same(s_lik, s_gj)


@pytest.mark.parametrize("n", [3, 21, 4001, 20000, 60000])
def test_row_counts_at_the_edges_of_the_task_layout(n):
    """3: fewer rows than one task.  21: 6 tasks for the 8 wavefronts of two workgroups, and fewer than 8 workgroups (no
    XCD-aware order).  4001 = 4 * 1000 + 1: a last task with one set; 1001 tasks dealt to the 8 XCDs in eighths of 125 for 31
    or 32 four-wave workgroups each, so some wavefronts take no task.  20 000: 5000 tasks for 2048 wavefronts, XCD-aware
    order, several tasks per wavefront, the first of wavefront 0 padded and its later ones complete.  60 000: 2 : 1 shares."""
    plan, cp, tau, n_failed, ll_ref = _raw_case(n, 30, 7 + n)
    s_lik, s_gj = _two_routes(plan, "matern", cp, np.array([tau]))
    assert s_lik[6] == s_gj[6] == n_failed == 0 and s_lik[7] == s_gj[7] == n
    _assert_same(s_lik, s_gj)
    print(f"n={n}: loglik {_ll(s_lik, n)!r} oracle {ll_ref!r} rel {abs(_ll(s_lik, n) - ll_ref) / abs(ll_ref):.2e}")
    assert abs(_ll(s_lik, n) - ll_ref) <= LL_RTOL * abs(ll_ref)
    assert abs(_ll(s_gj, n) - ll_ref) <= LL_RTOL * abs(ll_ref)


@pytest.mark.parametrize("m", [20, 30])
def test_padded_sets_coincident_points_and_a_nan(m):
    """The first m sets of every plan here have missing neighbours: their tasks run the masked rounds with the same table,
    in one launch with complete sets.  Coincident points (distance 0 inside many blocks) must not fail; a NaN coordinate
    must fail every set that contains the point, on both routes and in the oracle."""
    from oracle import r_side as R
    n = 4000
    cp = [1.0, 0.15, 1.5]
    z, va, plan = _case(n, m, 2, 11 + m, dup=40)
    s_lik, s_gj = _two_routes(plan, "matern", cp, np.array([0.1]))
    ref = R.createU(va, cp, 0.1)
    assert s_lik[6] == s_gj[6] == ref["U_entries"]["n_failed"] == 0 and s_lik[7] == n
    _assert_same(s_lik, s_gj)
    ll_ref, _ = R.separable_loglik_condz(va, ref["U_entries"], z, 0.1)
    assert abs(_ll(s_lik, n) - ll_ref) <= LL_RTOL * abs(ll_ref)
    z, va, plan = _case(n, m, 2, 13 + m, nan_at=n // 2)
    s_lik, s_gj = _two_routes(plan, "matern", cp, np.array([0.1]))
    ref = R.createU(va, cp, 0.1)
    assert s_lik[6] == s_gj[6] == ref["U_entries"]["n_failed"] >= 1


def test_table_route_is_reproducible():
    plan, cp, tau, _, _ = _raw_case(20000, 30, 7 + 20000)
    plan.eval("matern", cp, np.array([tau]), FLAGS)
    a = np.array(plan.sums(), dtype=np.float64)
    plan.eval("matern", cp, np.array([tau]), FLAGS)
    b = np.array(plan.sums(), dtype=np.float64)
    assert a.tobytes() == b.tobytes()
