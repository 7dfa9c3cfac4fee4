"""gpv_plan_loglik_grad_sgv (gpv_grad_sgv.hip) on the GPU: value and analytic gradient of the log-likelihood at the default
conditioning cond.yz='SGV'.

Truth: tests/_sgv_grad_truth.py, a dense numpy restatement in the direct form (tests/test_sgv_grad_truth_host.py keeps it
honest on the CPU: against long-double central differences, the dense normal, the 'z' restatement, and float64 against long
double on every case below).  Bars, the project's flat 1e-8: per column |col_terms[k] - truth|_inf <= 1e-8 max(scale_k, 1) with
scale_k the sum of the absolute values of the column's summands; totals within 1e-8 sum_k scale_k; the value within 1e-8
relative of the truth and equal to loglik_from_sums of the plan's sums.

Inputs (tests/_sgv_grad_cases.py): seeded uniform locations in the unit cube, tau = 0.1, range 0.25 sqrt(d / 2) (0.06 and 0.03
for nu 1.5 and 2.5 in two dimensions, where the longer range makes the float64 truth itself too inexact), variance 1.3,
ordering none, exact ordered neighbours, SGV flags from vecchia_specify; n = 300, so that columns exist outside the 128-column
dense top block of the posterior pass."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _grad_truth as T
import _sgv_grad_cases as K

pytestmark = pytest.mark.gpu

TOL = 1e-8
TAU = K.TAU
HERE = os.path.dirname(os.path.abspath(__file__))


def _need_gpu():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


def _plan(G, va, z, locs=None, posterior=True):
    prep = va["U_prep"]
    plan = G.Plan(va["locsord"] if locs is None else locs, prep["revNNarray"], prep["revCond"])
    plan.set_data(z)
    if posterior:
        plan.build_posterior()
    return plan


def _check(ll, grad, cols, t, what):
    want, scale = t["col_terms"], t["scale"]
    keep = ~np.isnan(want[0])
    assert np.array_equal(np.isnan(cols), np.isnan(want)), what
    err = np.abs(cols[:, keep] - want[:, keep]).max(axis=1) / np.maximum(scale[:, keep].max(axis=1), 1.0)
    print(f"{what}: worst column error {err.max():.3e} (column {int(err.argmax())})")
    assert err.max() <= TOL, (what, float(err.max()), int(err.argmax()))
    off = np.abs(grad[keep] - t["grad"][keep]) / scale[:, keep].sum(axis=0)
    print(f"{what}: totals off by {off.max():.3e} of sum scale; value off {abs(ll - t['loglik']) / abs(t['loglik']):.3e}")
    assert np.array_equal(np.isnan(grad), ~keep) and off.max() <= TOL, (what, grad, t["grad"])
    assert abs(ll - t["loglik"]) <= TOL * abs(t["loglik"]), (what, ll, t["loglik"])


@pytest.mark.parametrize("fam", K.FAMILIES)
@pytest.mark.parametrize("m,d", K.SHAPES, ids=["m%d-d%d" % s for s in K.SHAPES])
def test_buckets_and_edges(m, d, fam):
    G = _need_gpu()
    locs, z, va = K.setup(m, d)
    cm, cp = K.family(fam, d)
    plan = _plan(G, va, z)
    ll, grad, nfail, cols = plan.loglik_grad_sgv(cm, cp, TAU, col_terms=True)
    assert nfail == 0
    assert ll == G.loglik_from_sums(plan.sums(), K.N)
    _check(ll, grad, cols, K.truth(m, d, fam), f"m = {m}, d = {d}, {fam}")


@pytest.mark.parametrize("fam", ("nu1.5", "esqe"))
def test_cond_z_plan_with_a_structure(fam):
    """W is diagonal: the entry agrees with gpv_plan_loglik_grad (and with the truth of this file) within the same bar"""
    G = _need_gpu()
    m, d = 10, 2
    locs, z, va = K.setup(m, d, cond="z")
    cm, cp = K.family(fam, d)
    plan = _plan(G, va, z)
    ll, grad, nfail, cols = plan.loglik_grad_sgv(cm, cp, TAU, col_terms=True)
    assert nfail == 0
    t = K.truth(m, d, fam, cond="z")
    _check(ll, grad, cols, t, f"cond z, {fam}")
    llz, gz, nfz, rows = plan.loglik_grad(cm, cp, TAU, row_terms=True)
    keep = ~np.isnan(gz)
    err = np.abs(cols[:, keep] - rows[:, 1:][:, keep]).max(axis=1) / np.maximum(t["scale"][:, keep].max(axis=1), 1.0)
    print("against Plan.loglik_grad: worst column", err.max(), "value", abs(ll - llz) / abs(llz))
    assert nfz == 0 and err.max() <= TOL and abs(ll - llz) <= TOL * abs(llz)
    assert np.all(np.abs(grad - gz)[keep] <= TOL * t["scale"][:, keep].sum(axis=0))


@pytest.mark.parametrize("fam", ("nu1.5", "esqe"))
def test_exact_at_full_conditioning(fam):
    """m = n - 1 under SGV: the Vecchia density is the multivariate normal"""
    G = _need_gpu()
    n = 60
    locs, z, va = K.setup(n - 1, 2, n=n)
    cm, cp = K.family(fam, 2)
    ll, grad, nfail, cols = _plan(G, va, z).loglik_grad_sgv(cm, cp, TAU, col_terms=True)
    assert nfail == 0
    t = K.truth(n - 1, 2, fam, n=n)
    _check(ll, grad, cols, t, f"m = n - 1, {fam}")
    ll_d, g_d = T.dense_mvn(locs, z, cm, cp, TAU)
    keep = ~np.isnan(g_d)
    scale = t["scale"][:, keep].sum(axis=0)
    print("dense MVN: value off", abs(ll - ll_d) / abs(ll_d), "gradient off", (np.abs(grad - g_d)[keep] / scale).max())
    assert abs(ll - ll_d) <= TOL * abs(ll_d)
    assert np.all(np.abs(grad - g_d)[keep] <= TOL * scale)


def _child(tmp_path, name, env_extra, m=30, d=2, fam="nu1.5"):
    out = str(tmp_path / f"{name}.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_sgv_grad_child.py"), str(m), str(d), fam, out],
                       env=dict(os.environ, **env_extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out)


@functools.lru_cache(maxsize=None)
def _here(m=30, d=2, fam="nu1.5"):
    G = _need_gpu()
    locs, z, va = K.setup(m, d)
    cm, cp = K.family(fam, d)
    return _plan(G, va, z).loglik_grad_sgv(cm, cp, TAU, col_terms=True)


@pytest.mark.parametrize("name,env", [("top0", {"GPV_POST_TOP": "0"}), ("top64", {"GPV_POST_TOP": "64"}),
                                      ("top128", {"GPV_POST_TOP": "128"}), ("nograph", {"GPV_NO_GRAPH": "1"})])
def test_posterior_routes_in_fresh_processes(tmp_path, name, env):
    """every form of the posterior pass's top block agrees within 1e-12 of the scales; launch by launch instead of the captured
    graphs gives the same bits"""
    ll, grad, nfail, cols = _here()
    r = _child(tmp_path, name, env)
    t = K.truth(30, 2, "nu1.5")
    keep = ~np.isnan(grad)
    assert int(r["nfail"]) == 0
    err = np.abs(r["cols"][:, keep] - cols[:, keep]).max(axis=1) / np.maximum(t["scale"][:, keep].max(axis=1), 1.0)
    off = np.abs(r["grad"][keep] - grad[keep]) / t["scale"][:, keep].sum(axis=0)
    print(name, "columns", err.max(), "totals", off.max(), "value", abs(float(r["ll"]) - ll) / abs(ll))
    assert err.max() <= 1e-12 and off.max() <= 1e-12 and abs(float(r["ll"]) - ll) <= 1e-12 * abs(ll)
    if name in ("top128", "nograph"):
        assert float(r["ll"]) == ll and np.array_equal(r["grad"], grad, equal_nan=True)
        assert np.array_equal(r["cols"], cols, equal_nan=True)


@functools.lru_cache(maxsize=None)
def _large():
    """n = 40 000, m = 10, 2-D, the product's own neighbour search: the grid cap gives every wavefront 9 or 10 sets.  The plan
    and two successive results, shared by the two tests below.  The range is that of the n = 300 cases scaled with the point
    spacing (K.family_at: 0.06 sqrt(300 / 40 000) = 0.0052), so that the blocks are distributed as theirs."""
    G = _need_gpu()
    n, m, d = 40000, 10, 2
    rng = np.random.default_rng(17)
    locs = rng.random((n, d))
    z = rng.standard_normal(n)
    va = G.vecchia_specify(locs, m, ordering="none", cond_yz="SGV")
    cm, cp = K.family_at("nu1.5", d, n)
    plan = _plan(G, va, z)
    return plan, n, cm, cp, plan.loglik_grad_sgv(cm, cp, TAU, col_terms=True), plan.loglik_grad_sgv(cm, cp, TAU, col_terms=True)


def test_more_than_one_set_per_wavefront():
    G = _need_gpu()
    plan, n, cm, cp, (ll, grad, nfail, cols), (ll2, grad2, _, cols2) = _large()
    assert nfail == 0
    assert ll2 == ll and np.array_equal(grad2, grad, equal_nan=True) and np.array_equal(cols2, cols, equal_nan=True)
    keep = ~np.isnan(grad)
    off = np.abs(cols[:, keep].sum(axis=0) - grad[keep]) / np.abs(cols[:, keep]).sum(axis=0)
    print("rows of col_terms against grad:", off)
    assert off.max() <= 1e-10
    plan.eval(cm, cp, TAU, G.GPV_WANT_DENOM)
    assert ll == G.loglik_from_sums(plan.sums(), n)                      # the value is the SGV evaluation's


def test_central_differences_of_the_evaluation():
    """Every component within 1e-6 relative of central differences (h = 1e-6 theta) of GPV_WANT_DENOM evaluations, after the
    round-off bound eps |l| / h / |g| < 1e-7 of tests/test_gpu_loglik_grad.py::test_against_existing_path.

    Measured on an MI355X at the range of _large (relative distance of the analytic component from the central difference;
    the round-off bound is 1.5e-9, 5.1e-10, 8.6e-10):
        h / theta     variance     range        nugget
        1e-6          9.9e-10      1.1e-9       7.8e-10
        1e-5          5.7e-10      8.3e-11      5.5e-11
        1e-4          7.3e-9       2.4e-9       5.4e-9        (the truncation of the differences, 100 times that of 1e-5)
    Why the range is scaled: at range 0.25, forty times the point spacing of this plan, the check is missed for the variance
    and the range (4.5e-6 and 5.4e-6 at h = 1e-6 theta, 3.4e-7 and 1.2e-7 at 1e-5, 1.1e-7 and 4.1e-9 at 1e-4: falling as 1 / h,
    the behaviour of noise in the evaluated values).  Under SGV the latent entries of a block carry no nugget, so blocks of
    close latent points are ill conditioned; the sums of an evaluation then carry 1e5 eps each (the differences of sums [0] and
    [2] at h = 1e-6 theta are off by 1e-4 of themselves, in proportion, and cancel in the likelihood but for 300 eps |l|),
    which is no property of the gradient and which the bound eps |l| / h / |g| does not know.  It is the conditioning that makes
    the float64 truth of the n = 300 cases stray at that range (tests/_sgv_grad_cases.py), and the remedy is the same: a shorter
    range, here by the rule of K.family_at.  The figures of the other steps are printed, not asserted."""
    G = _need_gpu()
    plan, n, cm, cp, (ll, grad, nfail, cols), _ = _large()

    def existing(cp_, tau_):
        plan.eval(cm, cp_, tau_, G.GPV_WANT_DENOM)
        return G.loglik_from_sums(plan.sums(), n)

    ll0 = existing(cp, TAU)
    theta = np.array([cp[0], cp[1], TAU])
    g = np.array([grad[0], grad[1], grad[3]])

    def relative(i, rel):
        tp, tm = theta.copy(), theta.copy()
        tp[i] += rel * theta[i]
        tm[i] -= rel * theta[i]
        cd = (existing([tp[0], tp[1], 1.5], tp[2]) - existing([tm[0], tm[1], 1.5], tm[2])) / (tp[i] - tm[i])
        print(f"h = {rel:g} theta, component {i}: analytic {g[i]:.10g} central difference {cd:.10g} "
              f"relative {abs(cd - g[i]) / abs(g[i]):.3e}")
        return abs(cd - g[i]) / abs(g[i])

    for rel in (1e-5, 1e-4):
        for i in range(3):
            relative(i, rel)
    roundoff = np.finfo(float).eps * abs(ll0) / (1e-6 * theta) / np.abs(g)
    print("round-off bound of the central differences, relative to the components:", roundoff)
    assert roundoff.max() < 1e-7
    worst = max(relative(i, 1e-6) for i in range(3))
    assert worst <= 1e-6


def test_state_is_that_of_a_mean_evaluation():
    G = _need_gpu()
    locs, z, va = K.setup(30, 2)
    cm, cp = K.family("nu1.5", 2)
    a, b = _plan(G, va, z), _plan(G, va, z)
    a.eval(cm, [0.9, 0.2, 2.5], 0.3, G.GPV_WANT_MEAN)                    # an earlier evaluation at other parameters
    b.eval(cm, [0.9, 0.2, 2.5], 0.3, G.GPV_WANT_MEAN)
    stamp = a.factor_stamp()
    ll, grad, nfail = a.loglik_grad_sgv(cm, cp, TAU)
    b.eval(cm, cp, TAU, G.GPV_WANT_MEAN)
    assert nfail == 0 and ll == G.loglik_from_sums(b.sums(), K.N)
    assert np.array_equal(a.sums(), b.sums()) and np.array_equal(a.posterior_mean(), b.posterior_mean())
    assert a.factor_stamp() == stamp + 1 == b.factor_stamp()
    va_, da = a.selinv()[:2]
    vb_, db = b.selinv()[:2]
    assert np.array_equal(va_, vb_) and da == db == 0


def test_state_refusals_leave_the_plan_untouched():
    G = _need_gpu()
    locs, z, va = K.setup(10, 2)
    cm, cp = K.family("nu1.5", 2)
    plan = _plan(G, va, z)
    plan.eval(cm, cp, TAU, G.GPV_WANT_MEAN)
    sums, mean, stamp = plan.sums(), plan.posterior_mean(), plan.factor_stamp()

    def status(fn):
        with pytest.raises(G.GpvError) as e:
            fn()
        return e.value.status

    assert status(lambda: plan.loglik_grad_sgv("matern", [1.3, 0.25, 0.8], TAU)) == 4      # GPV_ERR_UNSUPPORTED_NU
    assert status(lambda: plan.loglik_grad_sgv("matern_scaledim", [1.3, 0.25, 0.25, 1.5], TAU)) == 4
    assert status(lambda: plan.loglik_grad_sgv("gauss", [1.3, 0.25, 0.5], TAU)) == 3       # GPV_ERR_COVTYPE
    assert status(lambda: plan.loglik_grad_sgv("matern", [1.3, 0.25], TAU)) == 2           # GPV_ERR_BAD_ARG
    assert status(lambda: plan.loglik_grad_sgv("matern", cp, 0.0)) == 2
    assert status(lambda: plan.loglik_grad_sgv("matern", cp, np.inf)) == 2
    assert np.array_equal(plan.sums(), sums) and np.array_equal(plan.posterior_mean(), mean) and plan.factor_stamp() == stamp
    prep = va["U_prep"]
    nodata = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
    nodata.build_posterior()
    assert status(lambda: nodata.loglik_grad_sgv(cm, cp, TAU)) == 7                        # GPV_ERR_STATE: no data
    assert status(lambda: _plan(G, va, z, posterior=False).loglik_grad_sgv(cm, cp, TAU)) == 7     # no posterior structure
    filled = _plan(G, va, z, posterior=False)
    assert filled.build_posterior_fill() is not None
    assert status(lambda: filled.loglik_grad_sgv(cm, cp, TAU)) == 7                        # a filled structure
    unobs = _plan(G, va, z)
    unobs.set_observed(np.arange(K.N) % 7 != 0)
    assert status(lambda: unobs.loglik_grad_sgv(cm, cp, TAU)) == 7                         # unobserved locations
    shard = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"], row_begin=0, row_end=150)
    shard.set_data(z)
    assert status(lambda: shard.loglik_grad_sgv(cm, cp, TAU)) == 7                         # a row shard
    vy = G.vecchia_specify(np.array(locs), 10, ordering="none", cond_yz="y")
    drops = _plan(G, vy, z)                                                                # 'y' flags on the unfilled pattern
    assert status(lambda: drops.loglik_grad_sgv(cm, cp, TAU)) == 7                         # its selected inverse drops terms
    wide = G.vecchia_specify(np.array(locs), 64, ordering="none", cond_yz="z")
    assert status(lambda: _plan(G, wide, z, posterior=False).loglik_grad_sgv(cm, cp, TAU)) == 5   # GPV_ERR_UNSUPPORTED_M
    # the entries that refuse SGV plans keep refusing them
    assert status(lambda: plan.loglik_grad(cm, cp, TAU)) == 7
    with pytest.raises(ValueError, match="cond_yz='z'"):
        G.vecchia_likelihood_grad(z, va, cp, TAU)


def test_nan_coordinate():
    G = _need_gpu()
    m, d, bad = 10, 2, 150
    locs, z, va = K.setup(m, d)
    cm, cp = K.family("nu1.5", d)
    poisoned = np.array(va["locsord"])
    poisoned[bad, d - 1] = np.nan
    ll, grad, nfail, cols = _plan(G, va, z, locs=poisoned).loglik_grad_sgv(cm, cp, TAU, col_terms=True)
    revNN = va["U_prep"]["revNNarray"]
    hit = np.array([bad in T.valid_entries(revNN[k]) for k in range(K.N)])
    assert hit.sum() >= 1 and nfail == hit.sum()
    assert ll == -np.inf and np.all(np.isnan(grad))
    assert np.all(np.isnan(cols[hit]))


def test_python_wrapper_agrees_with_the_plan():
    G = _need_gpu()
    locs, z, va = K.setup(10, 2)
    cm, cp = K.family("nu1.5", 2)
    ll, grad, _, _ = _here(10, 2, "nu1.5")
    ll2, grad2 = G.vecchia_likelihood_grad_sgv(z, va, cp, TAU, covmodel=cm)
    assert ll2 == ll and np.array_equal(grad2, grad, equal_nan=True)


@functools.lru_cache(maxsize=None)
def _field():
    """n = 1500 draws of a Matern-1.5 field (variance 2, range 0.2) plus noise 0.3, by dense Cholesky on the host (the field
    of tests/test_gpu_loglik_grad.py)"""
    rng = np.random.default_rng(2024)
    n = 1500
    locs = rng.random((n, 2))
    r = np.sqrt(((locs[:, None, :] - locs[None, :, :]) ** 2).sum(-1))
    c = np.sqrt(3.0) / 0.2
    Sg = 2.0 * (1 + c * r) * np.exp(-c * r) + 0.3 * np.eye(n)
    data = np.linalg.cholesky(Sg) @ rng.standard_normal(n)
    return locs, data


def test_estimation():
    G = _need_gpu()
    locs, data = _field()
    kw = dict(m=10, cond_yz="SGV", output_level=0)
    nm = G.vecchia_estimate(data, locs, smoothness=1.5, **kw)
    lb = G.vecchia_estimate(data, locs, smoothness=1.5, method="L-BFGS-B", **kw)
    reltol = np.sqrt(np.finfo(float).eps)
    print("Nelder-Mead", nm["neg_loglik"], nm["n_evals"], nm["theta_hat"], "L-BFGS-B", lb["neg_loglik"], lb["n_evals"],
          lb["theta_hat"])
    assert lb["convergence"] == 0
    assert lb["neg_loglik"] <= nm["neg_loglik"] + 100 * reltol * abs(nm["neg_loglik"])
    assert lb["n_evals"] < nm["n_evals"] / 3
    with pytest.raises(ValueError, match="cond_yz"):
        G.vecchia_estimate(data, locs, smoothness=1.5, method="L-BFGS-B", m=10, output_level=0)
    with pytest.raises(ValueError, match="cond_yz"):
        G.vecchia_estimate(data, locs, smoothness=1.5, method="fisher", **kw)
