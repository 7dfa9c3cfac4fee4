"""A plan's device resources across rebuilds, growth and destruction (gpv_hip_raii.hpp: every buffer, event and graph of a
plan is a member that releases itself; a rebuild replaces tables and drops the captured graphs that name them).

Every path below is documented as bitwise reproducible, so every comparison is assert_array_equal.  One geometry: 3000
uniform points in the unit square, m = 20, SGV, maxmin ordering: more columns than the 128 of the posterior pass's dense
top block, so a level schedule exists, and 40 rows / 33 columns are two batches of gpv_lincomb_batch() = 32.
"""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

pytestmark = pytest.mark.gpu

N, M = 3000, 20
CP, CP_GEN = [1.0, 0.1, 1.5], [1.0, 0.1, 1.1]


def _need_gpu():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


@pytest.fixture(scope="module")
def case():
    G = _need_gpu()
    rng = np.random.default_rng(2024)
    locs = rng.random((N, 2))
    va = G.vecchia_specify(locs, M, ordering="maxmin", cond_yz="SGV")
    vz = G.vecchia_specify(locs, M, ordering="maxmin", cond_yz="z")
    z = np.sin(5 * locs[:, 0]) * np.cos(4 * locs[:, 1]) + 0.3 * rng.standard_normal(N)
    tau = 0.05 + 0.1 * rng.random(N)
    E = rng.standard_normal((33, N))
    return dict(G=G, va=va, vz=vz, z_ord=z[va["ord"] - 1], tau_ord=tau[va["ord"] - 1], E=E)


def _new_plan(c, va=None):
    va = va or c["va"]
    prep = va["U_prep"]
    plan = c["G"].api.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
    plan.set_data(c["z_ord"])
    return plan


def _round(c, plan):
    """build_posterior, one evaluation with denominator + mean and a nugget vector, and everything that reads its factor"""
    import scipy.sparse as sp
    G = c["G"]
    assert plan.build_posterior() > 1                                   # a level schedule, not the top block alone
    plan.eval("matern", CP, c["tau_ord"], G.GPV_WANT_DENOM | G.GPV_WANT_MEAN)
    out = dict(sums=plan.sums(), mean=plan.posterior_mean())
    rows = N - 1 - 7 * np.arange(40)                                    # 40 unit rows: two batches
    H = sp.csr_matrix((np.ones(40), (np.arange(40), rows)), shape=(40, N))
    out["vars"] = plan.lincomb(H)
    out["gram"] = plan.lincomb(H[:32], cov_mat=True)                    # (a covariance matrix takes at most one batch of rows)
    out["solve_t"] = plan.solve_t(c["E"])                               # 33 columns: a full batch and one more
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert_array_equal(a[k], b[k], err_msg=k)


@pytest.fixture(scope="module")
def first_round(case):
    plan = _new_plan(case)
    return plan, _round(case, plan)


def test_rebuild_gives_the_first_rounds_results(case, first_round):
    """A second gpv_plan_build_posterior replaces every table and drops the three kinds of captured graph; the same calls
    then give the first round's results, which are also those of a plan that never saw a rebuild."""
    plan, ref = first_round
    assert np.all(np.isfinite(ref["sums"])) and np.all(ref["vars"] > 0.0) and np.all(np.isfinite(ref["solve_t"]))
    _same(_round(case, plan), ref)
    _same(_round(case, _new_plan(case)), ref)


def test_draws_buffers_grow(case, first_round):
    """32 draws, then 96 on the same plan (the per-draw buffers are replaced by larger ones) = 96 draws on a fresh plan."""
    plan, _ = first_round
    plan.draws_summary(32, seed=7)
    got = plan.draws_summary(96, seed=7)
    fresh = _new_plan(case)
    _round(case, fresh)
    want = fresh.draws_summary(96, seed=7)
    for k in ("mean", "var", "draw_max", "draw_mean"):
        assert_array_equal(got[k], want[k], err_msg=k)


def test_destroy_after_every_first_use_buffer_exists(case, first_round):
    """A plan goes through the posterior pass, lincomb, solve_t and the draws; Lentries, Zentries, a general-nu evaluation
    and (on a cond.yz='z' plan of the same points) loglik_grad allocate the rest.  Destroying both and creating the same
    plan again gives the first round's sums: the release order holds under the real runtime."""
    from gpvecchia_amd import _lib as L
    G = case["G"]
    ref = first_round[1]
    plan = _new_plan(case)
    _round(case, plan)
    plan.draws_summary(32, seed=7)
    plan.eval("matern", CP, case["tau_ord"], G.GPV_WANT_U | G.GPV_WANT_NUMERATOR)
    assert np.all(np.isfinite(plan.Lentries())) and np.all(np.isfinite(plan.Zentries()))
    plan.eval("matern", CP_GEN, case["tau_ord"], G.GPV_WANT_NUMERATOR)
    assert np.all(np.isfinite(plan.sums()))
    pz = _new_plan(case, case["vz"])
    ll, _, nfail = pz.loglik_grad("matern", CP, 0.1, row_terms=True)[:3]
    assert np.isfinite(ll) and nfail == 0
    for p in (plan, pz):
        assert L.lib().gpv_plan_destroy(p._h) == 0
        p._h.value = None                                              # (so that __del__ does not destroy it again)
    assert_array_equal(_round(case, _new_plan(case))["sums"], ref["sums"])
