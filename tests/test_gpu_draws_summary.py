"""gpv_plan_draws_normals / gpv_plan_draws_summary / vecchia_posterior_summary on the GPU (gpv_lincomb.hip: the fill, the
accumulation and the finish kernels around the transposed sweep).

The sweep itself is held to the oracle by tests/test_gpu_posterior_sample.py; here the device generator is held to the host
generator (tests/test_draws_generator_host.py holds that one to a restatement), and the fused sums to NumPy ON THE SAME BITS:
E = Plan.draws_normals, X = Plan.solve_t(E), the summaries of mu + X in NumPy.  Counts and the maximum must then be equal
exactly; sums to 1e-12 (order of summation, a few ulp of exp).

Run as a script (`python tests/test_gpu_draws_summary.py OUT.npz`) this file computes the summary of _child_case on plan (a) and
saves it: the tests start it in fresh child processes under GPV_NO_GRAPH=1 and GPV_POST_TOP=0, switches the library reads once."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
THR = [-0.4, 0.1, 0.8]
KEYS = ("mean", "var", "exceed", "draw_max", "draw_mean")
SEED4 = 3          # test 4: chosen on the CPU, see there


def _need_gpu():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


def _plan_a(G):
    """n = 1500, m = 10, maxmin + SGV, Matern 1.5, vector nuggets, no prediction locations."""
    rng = np.random.default_rng(61)
    n = 1500
    locs = rng.random((n, 2))
    z = np.sin(5 * locs[:, 0]) * np.cos(4 * locs[:, 1]) + 0.3 * rng.standard_normal(n)
    tau = 0.05 + 0.1 * rng.random(n)
    cp = [1.0, 0.1, 1.5]
    va = G.vecchia_specify(locs, 10, ordering="maxmin", cond_yz="SGV")
    preds = G.vecchia_prediction(z, va, cp, tau, return_values="meanmat")
    plan = G.api._plan_for(va, 0)
    return dict(va=va, preds=preds, plan=plan, off=0, mu=plan.posterior_mean(), n=n, z=z, cp=cp, tau=tau, locs=locs)


def _plan_b(G):
    """1000 observed + 237 prediction locations, the default 'zy': 1000 dummy rows in front, Nlocs = 2237 = 34 * 64 + 61."""
    rng = np.random.default_rng(62)
    n, n_p = 1000, 237
    locs, lp = rng.random((n, 2)), rng.random((n_p, 2))
    z = np.sin(5 * locs[:, 0]) * np.cos(4 * locs[:, 1]) + 0.3 * rng.standard_normal(n)
    tau = 0.05 + 0.1 * rng.random(n)
    cp = [1.0, 0.1, 1.5]
    va = G.vecchia_specify(locs, 10, locs_pred=lp)
    assert va["cond_yz"] == "zy"
    preds = G.vecchia_prediction(z, va, cp, tau, return_values="meanmat")
    assert preds["factor"]["kind"] == "device" and preds["factor"]["offset"] == n
    plan = G.api._plan_for(va, 0)
    assert plan.Nlocs == 2 * n + n_p and plan.Nlocs % 64 != 0
    mu = plan.posterior_mean()
    mu[:n] = 0.0
    return dict(va=va, preds=preds, plan=plan, off=n, mu=mu, n=n, n_p=n_p, z=z, cp=cp, tau=tau)


@pytest.fixture(scope="module")
def plans():
    G = _need_gpu()
    return dict(a=_plan_a(G), b=_plan_b(G))


def _mask(N_locs):
    return (np.arange(N_locs) * 7) % 3 == 0                              # about a third of the locations, spread over the order


def _child_case(c):
    return dict(ndraws=75, seed=9, skip_front=c["off"], mu_ord=c["mu"], link=1, thresholds=THR, mask=_mask(c["plan"].Nlocs))


def _g(link):
    return [lambda y: y, np.exp, lambda y: 1.0 / (1.0 + np.exp(-y))][link]


def _close(name, got, ref, tol=TOL):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))) if ref.size else 0.0
    print(f"{name}: max |diff| / max(1, |ref|) = {err:.3e}")
    assert err <= tol, (name, err)


# ---- 1. the device generator is the host generator ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["a", "b"])
def test_device_normals_equal_host_normals(plans, which):
    from gpvecchia_amd import lincomb as LC
    c = plans[which]
    plan, off, seed = c["plan"], c["off"], 2 ** 63 + 5
    E = plan.draws_normals(seed, 70, skip_front=off)
    assert E.shape == (70, plan.Nlocs)
    H = LC.draws_normals_host(seed, 0, plan.Nlocs, 0, 70)
    diff = np.abs(E[:, off:] - H[:, off:]).max()
    print(f"plan ({which}): max |device - host| normal = {diff:.3e}")
    assert diff <= 1e-13
    assert np.all(E[:, :off] == 0.0)                                      # the dummy rows of 'zy'
    assert np.all(E[:, off:] != 0.0)
    E2 = plan.draws_normals(seed, 38, col0=32, skip_front=off)
    assert np.array_equal(E2, E[32:70])
    E3 = plan.draws_normals(seed, 3, col0=33, skip_front=off)          # an odd first draw: the sine half of a pair
    assert np.array_equal(E3, E[33:36])
    assert not np.array_equal(plan.draws_normals(seed + 1, 2, skip_front=off), E[:2])


# ---- 2. summaries against NumPy on the same bits -------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 33, 75])
@pytest.mark.parametrize("which", ["a", "b"])
def test_summaries_against_numpy_on_the_same_draws(plans, which, N):
    c = plans[which]
    plan, off, mu, seed = c["plan"], c["off"], c["mu"], 17
    n = plan.Nlocs
    E = plan.draws_normals(seed, N, skip_front=off)
    X = plan.solve_t(E)
    assert np.all(X[:, :off] == 0.0)
    Y = mu[None, :] + X                                                  # one rounded add, as on the device
    live = np.arange(n) >= off
    for link, masked in ((0, True), (0, False), (1, True), (2, False)):
        mask = _mask(n) if masked else None
        res = plan.draws_summary(N, seed=seed, skip_front=off, mu_ord=mu, link=link, thresholds=THR, mask=mask)
        g = _g(link)
        GY, gmu = g(Y), g(mu)
        D = GY - gmu[None, :]
        name = f"plan ({which}) N={N} link={link} mask={masked}"
        exceed = np.array([np.count_nonzero(Y > t, axis=0) / N for t in THR]) * live[None, :]
        assert np.array_equal(res["exceed"], exceed), name                # counts: exactly
        sel = live if mask is None else (mask & live)
        dmax = GY[:, sel].max(axis=1)
        if link == 0:
            assert np.array_equal(res["draw_max"], dmax), name
        _close(name + " draw_max", res["draw_max"], dmax)
        _close(name + " draw_mean", res["draw_mean"], GY[:, sel].mean(axis=1))
        _close(name + " mean", res["mean"], np.where(live, gmu + D.sum(axis=0) / N, 0.0))
        _close(name + " var", res["var"], np.where(live, np.var(GY, axis=0, ddof=1), 0.0))
        assert np.all(res["var"][live] > 0.0) and np.all(res["var"][~live] == 0.0) and np.all(res["mean"][~live] == 0.0)
    # without thresholds and without the per-draw functionals: the same moments
    res2 = plan.draws_summary(N, seed=seed, skip_front=off, mu_ord=mu, link=2, draw_stats=False)
    assert res2["exceed"].shape == (0, n) and res2["draw_max"] is None
    assert np.array_equal(res2["mean"], res["mean"]) and np.array_equal(res2["var"], res["var"])
    # mu absent stands for zeros
    res3 = plan.draws_summary(N, seed=seed, skip_front=off, link=0)
    res4 = plan.draws_summary(N, seed=seed, skip_front=off, mu_ord=np.zeros(n), link=0)
    assert all(np.array_equal(res3[k], res4[k]) for k in KEYS)


# ---- 3. reproducibility and routes ---------------------------------------------------------------------------------------------
def _child(tmp_path, env_extra):
    out = str(tmp_path / "summary.npz")
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out)


def test_two_calls_and_the_launch_by_launch_route_give_the_same_bits(plans, tmp_path):
    c = plans["a"]
    stamp = c["plan"].factor_stamp()
    r1 = c["plan"].draws_summary(**_child_case(c))
    r2 = c["plan"].draws_summary(**_child_case(c))
    assert all(np.array_equal(r1[k], r2[k]) for k in KEYS)
    assert c["plan"].factor_stamp() == stamp
    ch = _child(tmp_path, {"GPV_NO_GRAPH": "1"})
    for k in KEYS:
        assert np.array_equal(ch[k], r1[k]), k


def test_all_columns_scheduled_route_agrees(plans, tmp_path):
    """GPV_POST_TOP=0: no dense top block, another exact route through the same factor: 1e-10."""
    c = plans["a"]
    r1 = c["plan"].draws_summary(**_child_case(c))
    ch = _child(tmp_path, {"GPV_POST_TOP": "0"})
    for k in KEYS:
        _close("GPV_POST_TOP=0 " + k, ch[k], r1[k], 1e-10)


# ---- 4. Monte-Carlo variances against the exact ones -----------------------------------------------------------------------------
def test_monte_carlo_variances_against_exact_ones(plans):
    """N = 4096 draws on plan (a), identity link: max_k |var_k / exact_k - 1| <= 6 sqrt(2 / (N - 1)) = 0.133 (the relative
    standard error of a Gaussian sample variance is sqrt(2 / (N - 1))), and |mean_k - mu_k| <= 6 sqrt(exact_k / N).  A condition,
    not a measurement.  The seed was chosen on the CPU with the host route of vecchia_posterior_summary on the same plan (oracle
    createU, api.U2V) and the same generator, asking for 5 sqrt(2 / (N - 1)) = 0.110 there: SEED4 gives 0.0860 for the variances
    and 3.21 sqrt(exact_k / N) for the means on the host (seeds 1 .. 6: 0.076 .. 0.096)."""
    from gpvecchia_amd import lincomb as LC
    c = plans["a"]
    plan, N = c["plan"], 4096
    exact = LC.exact_variances_device(plan, c["n"], 0)
    res = plan.draws_summary(N, seed=SEED4, mu_ord=c["mu"], link=0, draw_stats=False)
    rel = np.abs(res["var"] / exact - 1.0).max()
    zm = (np.abs(res["mean"] - c["mu"]) / np.sqrt(exact / N)).max()
    print(f"N = {N}: max |var / exact - 1| = {rel:.4f} (bound {6 * np.sqrt(2 / (N - 1)):.4f}), max |mean - mu| / se = {zm:.3f}")
    assert rel <= 6.0 * np.sqrt(2.0 / (N - 1))
    assert zm <= 6.0


# ---- 5. the public function ------------------------------------------------------------------------------------------------------
def test_public_function_device_route_against_host_route(plans):
    G = _need_gpu()
    from gpvecchia_amd import api as A
    from gpvecchia_amd import lincomb as LC
    c = plans["b"]
    preds, N = c["preds"], 64
    mask_pred = np.arange(c["n_p"]) % 2 == 0
    kw = dict(seed=5, thresholds=THR)
    dev = G.vecchia_posterior_summary(preds, N, **kw)
    assert dev["mean_obs"].shape == (c["n"],) and dev["var_pred"].shape == (c["n_p"],)
    assert dev["exceed_obs"].shape == (3, c["n"]) and dev["exceed_pred"].shape == (3, c["n_p"]) and dev["draw_max"].shape == (N,)
    U_obj = A.createU(c["va"], c["cp"], c["tau"])
    hp = dict(factor=LC._host_factor(U_obj, A.U2V(U_obj)), mu_obs=preds["mu_obs"], mu_pred=preds["mu_pred"])
    assert c["plan"].factor_stamp() == preds["factor"]["stamp"]
    host = G.vecchia_posterior_summary(hp, N, **kw)
    for nm in ("mean_obs", "mean_pred", "draw_max", "draw_mean"):        # per entry, |diff| <= 1e-8 max(1, |ref|)
        _close("device vs host route, " + nm, dev[nm], host[nm], 1e-8)
    for nm in ("var_obs", "var_pred"):                                    # variances are positive: per entry, purely relative
        err = (np.abs(dev[nm] - host[nm]) / host[nm]).max()
        print(f"device vs host route, {nm}: max relative diff {err:.3e}")
        assert np.all(host[nm] > 0.0) and err <= 1e-8, nm
    for nm in ("exceed_obs", "exceed_pred"):
        assert np.abs(dev[nm] - host[nm]).max() <= 2.0 / N, nm
    # a region of prediction locations, and the exp link
    dm = G.vecchia_posterior_summary(preds, N, link="exp", mask_pred=mask_pred, **kw)
    hm = G.vecchia_posterior_summary(hp, N, link="exp", mask_pred=mask_pred, **kw)
    for nm in ("mean_pred", "var_pred", "draw_max", "draw_mean"):
        _close("exp link, region: device vs host route, " + nm, dm[nm], hm[nm], 1e-8)
    assert np.all(dm["draw_max"] <= np.exp(dev["draw_max"]) * (1.0 + 1e-12))       # a region's maximum is below the whole field's
    with pytest.raises(ValueError):
        G.vecchia_posterior_summary(preds, 1)
    with pytest.raises(ValueError):
        G.vecchia_posterior_summary(preds, 8, link="probit")
    with pytest.raises(ValueError):
        G.vecchia_posterior_summary(preds, 8, mask_pred=np.zeros(c["n_p"], dtype=bool))
    with pytest.raises(ValueError):
        G.vecchia_posterior_summary(dict(mu_obs=preds["mu_obs"], mu_pred=preds["mu_pred"]), 8)


def test_vecchia_laplace_data_scale_moments():
    """Poisson counts, n = 400, m = 10: link='exp' gives the moments of the rate.  Jensen: mean >= exp(mu) wherever var > 0.
    For the SAMPLE the inequality is exact against exp(sample mean of y) at any N (same seed: the same draws under both links).
    Against exp(mu) the Monte-Carlo error of the mean, sd / sqrt(N) relative, has to stay below the gap sd^2 / 2 of the
    lognormal mean, that is sd sqrt(N) / 2 standard errors: with the posterior sd of this latent field, 0.218 .. 0.527
    (printed), N = 2048 leaves 4.9 standard errors at the worst location (with 64 draws 0.9: the inequality then fails at many
    locations by chance alone).  Two summaries of 2048 draws: 128 sweeps."""
    G = _need_gpu()
    rng = np.random.default_rng(13)
    n, m, N = 400, 10, 2048
    locs = rng.random((n, 2))
    cp = [0.5, 0.2, 1.5]
    z = rng.poisson(np.exp(0.5 * np.sin(5 * locs[:, 0]) + 0.3 * rng.standard_normal(n))).astype(np.float64)
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="SGV")
    vl = G.calculate_posterior_VL(z, va, "poisson", covparms=cp)
    assert vl["cnvgd"]
    out = G.vecchia_laplace_prediction(vl, va, cp, return_values="all")
    s = G.vecchia_posterior_summary(out, N, seed=3, link="exp", thresholds=[0.0])
    lat = G.vecchia_posterior_summary(out, N, seed=3, thresholds=[0.0])
    assert s["mean_obs"].shape == (n,) and s["mean_pred"].shape == (0,) and s["exceed_obs"].shape == (1, n)
    assert np.all(np.isfinite(s["mean_obs"])) and np.all(s["mean_obs"] > 0.0) and np.all(np.isfinite(s["var_obs"]))
    pos = s["var_obs"] > 0.0
    assert pos.all()
    sd = np.sqrt(out["var_obs"])
    print(f"VL: posterior sd of the latent field in [{sd.min():.3f}, {sd.max():.3f}]; min mean / exp(mu) = "
          f"{(s['mean_obs'] / np.exp(out['mu_obs'])).min():.5f}; MC var / exact in "
          f"[{(lat['var_obs'] / out['var_obs']).min():.3f}, {(lat['var_obs'] / out['var_obs']).max():.3f}]")
    assert np.all(s["mean_obs"] >= np.exp(lat["mean_obs"]) * (1.0 - 1e-12))          # Jensen for the sample: exact
    assert np.all(s["mean_obs"][pos] >= np.exp(out["mu_obs"][pos]) * (1.0 - 1e-12))
    assert np.array_equal(s["exceed_obs"], lat["exceed_obs"])                        # thresholds are on the latent scale
    assert np.all((s["exceed_obs"] >= 0.0) & (s["exceed_obs"] <= 1.0))
    assert np.all(s["draw_max"] > s["draw_mean"]) and np.all(s["draw_mean"] > 0.0)


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors_leave_the_plan_alone(plans):
    import ctypes as C
    G = _need_gpu()
    from gpvecchia_amd import _lib as L
    c = plans["a"]
    plan, n = c["plan"], c["plan"].Nlocs
    lib = L.lib()
    before = plan.draws_summary(**_child_case(c))
    stamp = plan.factor_stamp()
    mean, var, ex, dmx, dmn = np.zeros(n), np.zeros(n), np.zeros((8, n)), np.zeros(40), np.zeros(40)
    thr = np.arange(8, dtype=np.float64)
    none, some = np.zeros(n, dtype=np.uint8), np.ones(n, dtype=np.uint8)
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))

    def call(ndraws=40, skip=0, link=0, nthr=0, thr_=None, mask=None, mean_=L.dptr(mean), var_=L.dptr(var), ex_=None, dmx_=None,
             dmn_=None, h=plan._h):
        return lib.gpv_plan_draws_summary(h, ndraws, 1, skip, L.dptr(c["mu"]), link, nthr, thr_, mask, mean_, var_, ex_, dmx_, dmn_)
    BAD, STATE = 2, 7
    assert call(ndraws=1) == BAD and call(ndraws=0) == BAD and call(ndraws=-3) == BAD
    assert call(nthr=-1, thr_=L.dptr(thr), ex_=L.dptr(ex)) == BAD and call(nthr=9, thr_=L.dptr(thr), ex_=L.dptr(ex)) == BAD
    assert call(link=-1) == BAD and call(link=3) == BAD
    assert call(skip=-1) == BAD and call(skip=n) == BAD
    assert call(mask=u8(none), dmx_=L.dptr(dmx), dmn_=L.dptr(dmn)) == BAD
    assert call(mean_=None) == BAD and call(var_=None) == BAD
    assert call(nthr=2, thr_=None, ex_=L.dptr(ex)) == BAD and call(nthr=2, thr_=L.dptr(thr), ex_=None) == BAD
    assert call(dmx_=L.dptr(dmx)) == BAD and call(dmn_=L.dptr(dmn)) == BAD
    assert call(h=None) == BAD
    E = np.zeros((2, n))
    assert lib.gpv_plan_draws_normals(plan._h, 1, 0, 0, 2, None, n) == BAD
    assert lib.gpv_plan_draws_normals(plan._h, 1, 0, 0, -1, L.dptr(E), n) == BAD
    assert lib.gpv_plan_draws_normals(plan._h, 1, 0, -1, 2, L.dptr(E), n) == BAD
    assert lib.gpv_plan_draws_normals(plan._h, 1, 0, 0, 2, L.dptr(E), n - 1) == BAD
    assert lib.gpv_plan_draws_normals(plan._h, 1, n, 0, 2, L.dptr(E), n) == BAD
    assert lib.gpv_plan_draws_normals(plan._h, 1, -1, 0, 2, L.dptr(E), n) == BAD
    assert lib.gpv_plan_draws_normals(plan._h, 1, 0, 0, 0, L.dptr(E), n) == 0
    # a plan with the structure but without a factor
    rng = np.random.default_rng(7)
    va2 = G.vecchia_specify(rng.random((300, 2)), 8, ordering="maxmin", cond_yz="SGV")
    p2 = G.api._plan_for(va2, 0)
    assert p2.ensure_posterior() and p2.factor_stamp() == 0
    m2 = np.zeros(300)
    assert lib.gpv_plan_draws_summary(p2._h, 4, 1, 0, None, 0, 0, None, None, L.dptr(m2), L.dptr(m2), None, None, None) == STATE
    assert lib.gpv_plan_draws_normals(p2._h, 1, 0, 0, 1, L.dptr(m2), 300) == STATE
    with pytest.raises(G.GpvError) as ei:
        p2.draws_summary(4)
    assert ei.value.status == STATE
    # a communicator attached (world 1, the library's own RCCL binding): sharded plans have no posterior factor to sweep with
    comm = G.Comm(0, 0, 1, lambda mine: mine)
    plan.set_comm(comm)
    assert call() == STATE
    assert lib.gpv_plan_draws_normals(plan._h, 1, 0, 0, 2, L.dptr(E), n) == STATE
    assert call(ndraws=1) == BAD                                          # arguments are looked at first
    plan.set_comm(None)
    # (the last state rule, columns of more than 64 entries, cannot be reached: gpv_plan_build_posterior refuses such a
    # structure with GPV_ERR_UNSUPPORTED_M, so no plan ever holds a factor with post_ld > 64)
    # valid calls through the same arguments; then the plan answers as before and its factor is the same one
    assert call(mask=u8(some), dmx_=L.dptr(dmx), dmn_=L.dptr(dmn), nthr=8, thr_=L.dptr(thr), ex_=L.dptr(ex)) == 0
    after = plan.draws_summary(**_child_case(c))
    assert all(np.array_equal(before[k], after[k]) for k in KEYS)
    assert plan.factor_stamp() == stamp
    assert np.array_equal(plan.solve_t(np.ones(n)), plan.solve_t(np.ones(n)))


if __name__ == "__main__":
    import torch  # noqa: F401  (first: see tests/conftest.py)
    sys.path.insert(0, ROOT)
    import gpvecchia_amd as G
    c = _plan_a(G)
    np.savez(sys.argv[1], **c["plan"].draws_summary(**_child_case(c)))
