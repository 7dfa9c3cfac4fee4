"""gpv_plan_krige (gpv_krige.hip) on the GPU: local kriging of a cond.yz='z' plan at new locations, and what is built on it
(Plan.krige, vecchia_krige, vecchia_pred(local=True)).

Truth: tests/_krige_truth.py (the search definition and a long-double Cholesky per prediction location, proven on the CPU by
tests/test_krige_truth_host.py).  Observations: n = 6000 uniform points in the unit square, tau = 0.1, ranges 0.05 - 0.1, the
regime where SURVEY.md §8d measured cond(Sigma) <= 5e3.  Prediction locations: 130 (three wavefronts' worth of work for one
workgroup, the last partial), 5 of them on observations and 5 outside the bounding box.

The bar is the project's contract figure: every row within 1e-8 of the truth, the mean relative to ||u_J / u_last||_1 ||z||_inf
(the size of the sum it is), the variance relative to itself.  Each accuracy test prints the maxima it observed.  Observed on an
MI355X: mean <= 4.2e-14 and variance <= 1.3e-14 for the closed forms and esqe, 2.3e-14 and 7.3e-14 at smoothness 0.8 (DESIGN.md
§4s).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import _krige_truth as KT

pytestmark = pytest.mark.gpu

N, NQ, TAU, BAR = 6000, 130, 0.1, 1e-8
GPV_ERR_UNSUPPORTED_M, GPV_ERR_STATE = 5, 7
MATERN15 = ("matern", (1.2, 0.07, 1.5))


def _G():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


@functools.lru_cache(maxsize=None)
def _case(dim=2):
    """observations, 16 data columns, prediction locations and the 'z' specification (m = 10), shared and read-only"""
    G = _G()
    rng = np.random.default_rng(60 + dim)
    locs = rng.random((N, dim))
    Z = rng.standard_normal((N, 16))
    q = rng.random((NQ, dim))
    q[:5] = locs[rng.choice(N, 5, replace=False)]                  # on observations
    q[5:10, :2] = [[-0.3, 0.5], [1.2, 1.1], [0.5, 1.004], [-2.0, -3.0], [1.0 + 1e-9, 0.2]]                   # outside the box
    scale = None if dim == 2 else np.array([0.06, 0.08, 0.1])
    va = G.vecchia_specify(locs, 10, cond_yz="z", scale=scale)
    for a in (locs, Z, q):
        a.setflags(write=False)
    return dict(locs=locs, Z=Z, q=q, va=va, scale=scale)


@functools.lru_cache(maxsize=None)
def _truth(covmodel, cp, m, dim=2):
    """the long-double truth of all 16 columns for one family and list length: (mean, var, l1); no failure on these inputs"""
    c = _case(dim)
    sc = 1.0 if c["scale"] is None else c["scale"]
    NN = KT.query_nn(c["locs"] / sc, c["q"] / sc, m)
    mean, var, l1, failed = KT.krige_ld(c["locs"], TAU, c["Z"], c["q"], NN, covmodel, list(cp))
    assert not failed.any()
    return mean, var, l1


def _errors(got_mean, got_var, mean, var, l1, zmax):
    em = np.abs(got_mean - mean).max(axis=1) / (l1 * zmax)
    ev = np.abs(got_var - var) / var
    return float(em.max()), float(ev.max())


CONFIGS = [(MATERN15[0], MATERN15[1], m, 16) for m in (7, 15, 16, 30, 31, 63)] + \
          [("matern", (1.2, 0.07, 1.5), 30, 1), ("matern", (1.2, 0.07, 1.5), 30, 3),
           ("matern", (1.2, 0.1, 0.5), 30, 3), ("matern", (1.2, 0.05, 2.5), 30, 3), ("matern", (1.2, 0.06, 0.8), 30, 3),
           ("matern", (1.2, 0.06, 0.8), 63, 1), ("esqe", (0.8, 0.1, 0.4, 0.05), 30, 3), ("esqe", (0.8, 0.1, 0.4, 0.05), 15, 16)]


@pytest.mark.parametrize("covmodel,cp,m,R", CONFIGS)
def test_rows_agree_with_the_long_double_truth(covmodel, cp, m, R):
    G, c = _G(), _case()
    mean, var, l1 = _truth(covmodel, cp, m)
    Z = c["Z"][:, 0] if R == 1 else c["Z"][:, :R]
    out = G.vecchia_krige(Z, c["va"], c["q"], list(cp), TAU, covmodel=covmodel, m=m)
    assert out["n_failed"] == 0
    gm = out["mean_pred"][:, None] if R == 1 else out["mean_pred"]
    assert gm.shape == (NQ, R) and out["var_pred"].shape == (NQ,)
    em, ev = _errors(gm, out["var_pred"], mean[:, :R], var, l1, np.abs(c["Z"][:, :R]).max())
    print(f"krige {covmodel} {cp} m={m} R={R}: max mean error {em:.3g}, max var error {ev:.3g}")
    assert em <= BAR and ev <= BAR


def test_scaledim_in_three_dimensions_with_scale():
    G, c = _G(), _case(3)
    cp = (1.2, 0.06, 0.08, 0.1, 1.5)
    mean, var, l1 = _truth("matern_scaledim", cp, 30, 3)
    out = G.vecchia_krige(c["Z"][:, :3], c["va"], c["q"], list(cp), TAU, covmodel="matern_scaledim", m=30, scale=c["scale"])
    assert out["n_failed"] == 0
    em, ev = _errors(out["mean_pred"], out["var_pred"], mean[:, :3], var, l1, np.abs(c["Z"][:, :3]).max())
    print(f"krige matern_scaledim 3-D m=30: max mean error {em:.3g}, max var error {ev:.3g}")
    assert em <= BAR and ev <= BAR


def _plan_args(c):
    """the plan of the shared case and its ORDERED arrays"""
    from gpvecchia_amd import api
    va = c["va"]
    return api._plan_for(va), c["Z"][va["ord_z"] - 1]


def test_chunking_and_column_count_change_no_bit():
    c = _case()
    plan, Zord = _plan_args(c)
    covmodel, cp = MATERN15
    for m in (15, 30, 63):
        a = plan.krige(covmodel, cp, TAU, c["q"], m, Z_ord=Zord)
        b = plan.krige(covmodel, cp, TAU, c["q"], m, Z_ord=Zord, chunk=64)
        assert a[2] == 0 and b[2] == 0
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        for col in (0, 7, 15):                                         # a column alone, and among 16
            one = plan.krige(covmodel, cp, TAU, c["q"], m, Z_ord=Zord[:, col], chunk=33)
            assert np.array_equal(one[0][:, 0], a[0][:, col]) and np.array_equal(one[1], a[1])
        three = plan.krige(covmodel, cp, TAU, c["q"], m, Z_ord=Zord[:, 5:8])
        assert np.array_equal(three[0], a[0][:, 5:8])


def test_the_plans_own_data_and_given_neighbours():
    """Z_ord = None reads the plan's resident column; NNq given equals the search of the device"""
    from gpvecchia_amd import specify as S
    c = _case()
    plan, Zord = _plan_args(c)
    covmodel, cp = MATERN15
    a = plan.krige(covmodel, cp, TAU, c["q"], 30, Z_ord=Zord[:, 2])
    plan.set_data(Zord[:, 2])
    b = plan.krige(covmodel, cp, TAU, c["q"], 30)
    NNq = S.find_query_nn_gpu(c["va"]["locsord"], c["q"], 30)
    d = plan.krige(covmodel, cp, TAU, c["q"], 30, Z_ord=Zord[:, 2], NNq=NNq)
    for x in (b, d):
        assert np.array_equal(x[0], a[0]) and np.array_equal(x[1], a[1]) and x[2] == 0


def test_chain_rule_on_the_device():
    """vecchia_likelihood of the (n+1)-point 'z' plan through the set kernel = vecchia_likelihood(z) + the predictive log
    density of vecchia_krige, the appended location inside and outside the observed region"""
    G, c = _G(), _case()
    covmodel, cp = MATERN15
    z, tau0, z0, m = c["Z"][:, 0], 0.07, 0.4, 20
    va0 = G.vecchia_specify(c["locs"], m, cond_yz="z", ordering="none")
    ll0 = G.vecchia_likelihood(z, va0, list(cp), TAU, covmodel=covmodel)
    for s0 in ([0.41, 0.57], [1.05, -0.02]):
        s0 = np.array([s0])
        kr = G.vecchia_krige(z, va0, s0, list(cp), TAU, covmodel=covmodel, predict="z", nugget_pred=tau0)
        assert kr["n_failed"] == 0
        va1 = G.vecchia_specify(np.vstack([c["locs"], s0]), m, cond_yz="z", ordering="none")
        ll1 = G.vecchia_likelihood(np.append(z, z0), va1, list(cp), np.append(np.full(N, TAU), tau0), covmodel=covmodel)
        want = ll0 + KT.log_density(z0, kr["mean_pred"][0], kr["var_pred"][0])
        print(f"chain rule at {s0[0]}: {ll1!r} against {want!r}")
        assert abs(ll1 - want) <= 1e-10 * abs(ll1)


def test_a_vector_of_nuggets_agrees_with_the_truth():
    G, c = _G(), _case()
    covmodel, cp = MATERN15
    tau = 0.05 + 0.1 * np.random.default_rng(3).random(N)
    NN = KT.query_nn(c["locs"], c["q"], 30)
    mean, var, l1, failed = KT.krige_ld(c["locs"], tau, c["Z"][:, :3], c["q"], NN, covmodel, list(cp))
    assert not failed.any()
    out = G.vecchia_krige(c["Z"][:, :3], c["va"], c["q"], list(cp), tau, covmodel=covmodel, m=30)
    em, ev = _errors(out["mean_pred"], out["var_pred"], mean, var, l1, np.abs(c["Z"][:, :3]).max())
    print(f"krige with a nugget vector: max mean error {em:.3g}, max var error {ev:.3g}")
    assert out["n_failed"] == 0 and em <= BAR and ev <= BAR


def test_a_location_on_an_observation_without_nugget_fails_alone():
    G, c = _G(), _case()
    covmodel, cp = MATERN15
    j = int(np.nonzero((c["locs"] == c["q"][2]).all(axis=1))[0][0])    # the observation under prediction location 2
    tau = np.full(N, TAU)
    tau[j] = 0.0
    out = G.vecchia_krige(c["Z"][:, :3], c["va"], c["q"], list(cp), tau, covmodel=covmodel, m=30)
    assert out["n_failed"] == 1
    assert np.isnan(out["mean_pred"][2]).all() and np.isnan(out["var_pred"][2])
    rest = np.arange(NQ) != 2
    NN = KT.query_nn(c["locs"], c["q"], 30)
    mean, var, l1, _ = KT.krige_ld(c["locs"], tau, c["Z"][:, :3], c["q"][rest], NN[rest], covmodel, list(cp))
    em, ev = _errors(out["mean_pred"][rest], out["var_pred"][rest], mean, var, l1, np.abs(c["Z"][:, :3]).max())
    assert em <= BAR and ev <= BAR


def test_missing_data_never_enter_a_conditioning_set():
    G, c = _G(), _case()
    covmodel, cp = MATERN15
    z = c["Z"][:, 0].copy()
    miss = np.arange(N) % 3 == 0
    z[miss] = np.nan
    out = G.vecchia_krige(z, c["va"], c["q"], list(cp), TAU, covmodel=covmodel, m=15)
    NN = KT.query_nn(c["locs"], c["q"], 15, eligible=~miss)
    mean, var, l1, failed = KT.krige_ld(c["locs"], TAU, np.where(miss, 0.0, z), c["q"], NN, covmodel, list(cp))
    em, ev = _errors(out["mean_pred"][:, None], out["var_pred"], mean, var, l1, np.nanmax(np.abs(z)))
    assert not failed.any() and out["n_failed"] == 0 and em <= BAR and ev <= BAR
    with pytest.raises(ValueError):
        G.vecchia_krige(np.stack([z, z], axis=1), c["va"], c["q"], list(cp), TAU, covmodel=covmodel)


def _raw(plan, m, nq=NQ):
    """the C entry on sentinel-filled outputs: (status, mean, var, n_failed)"""
    from gpvecchia_amd import _lib as L
    c = _case()
    q = np.asfortranarray(c["q"][:nq])
    cp = np.array(MATERN15[1])
    nug = np.array([TAU])
    Z = np.asfortranarray(c["Z"][c["va"]["ord_z"] - 1][:, :2])
    mean, var, nf = np.full((nq, 2), -77.0, order="F"), np.full(nq, -77.0), C.c_int64(-77)
    st = L.lib().gpv_plan_krige(plan._h, b"matern", L.dptr(cp), 3, L.dptr(nug), 1, L.dptr(Z), N, 2, L.dptr(q), nq, m, None, None,
                                None, 0, L.dptr(mean), nq, L.dptr(var), C.byref(nf))
    return st, mean, var, nf.value


def test_refusals_write_nothing():
    G, c = _G(), _case()
    from gpvecchia_amd import api
    plan, _ = _plan_args(c)
    va = c["va"]
    prep = va["U_prep"]
    shard = api.Plan(va["locsord"], prep["revNNarray"], prep["revCond"], row_begin=0, row_end=N // 2)
    sgv = G.vecchia_specify(c["locs"][:500], 10, cond_yz="SGV")
    sgv_plan = api._plan_for(sgv)
    for pl, m, want in ((plan, 64, GPV_ERR_UNSUPPORTED_M), (shard, 30, GPV_ERR_STATE)):
        st, mean, var, nf = _raw(pl, m)
        assert st == want and (mean == -77.0).all() and (var == -77.0).all() and nf == -77
    from gpvecchia_amd import _lib as L
    q, cp, nug, Z = np.asfortranarray(c["q"]), np.array(MATERN15[1]), np.array([TAU]), np.zeros((500, 1), order="F")
    mean, var, nf = np.full((NQ, 1), -77.0, order="F"), np.full(NQ, -77.0), C.c_int64(-77)
    st = L.lib().gpv_plan_krige(sgv_plan._h, b"matern", L.dptr(cp), 3, L.dptr(nug), 1, L.dptr(Z), 500, 1, L.dptr(q), NQ, 10, None,
                                None, None, 0, L.dptr(mean), NQ, L.dptr(var), C.byref(nf))
    assert st == GPV_ERR_STATE and (mean == -77.0).all() and (var == -77.0).all() and nf.value == -77
    with pytest.raises(ValueError):
        G.vecchia_krige(np.zeros(500), sgv, c["q"], list(MATERN15[1]), TAU)
    with pytest.raises(G.GpvError) as e:
        G.vecchia_krige(c["Z"][:, 0], va, c["q"], list(MATERN15[1]), TAU, m=64)
    assert e.value.status == GPV_ERR_UNSUPPORTED_M
    st, mean, var, nf = _raw(plan, 63)                                  # the longest list is served
    assert st == 0 and nf == 0 and np.isfinite(mean).all() and np.isfinite(var).all()


def test_vecchia_pred_local_adds_the_trend_back():
    G = _G()
    rng = np.random.default_rng(8)
    n, m = 400, 10
    locs = rng.random((n, 2))
    Sigma = KT.cov_matrix(locs, "matern", [1.0, 0.1, 1.5]) + 0.05 * np.eye(n)
    data = 3.0 + np.linalg.cholesky(Sigma) @ rng.standard_normal(n)
    est = G.vecchia_estimate(data, locs, m=m, output_level=0, maxit=40, cond_yz="z")
    q = np.vstack([rng.random((40, 2)), [[1.1, 0.4]]])
    pred = G.vecchia_pred(est, q, m=m, local=True)
    th = np.asarray(est["theta_hat"])
    NN = KT.query_nn(locs, q, m)
    mean, var, l1, failed = KT.krige_ld(locs, th[-1], est["z"], q, NN, "matern", list(th[:-1]))
    assert not failed.any()
    em, ev = _errors(pred["mean_pred"][:, None] - est["beta_hat"][0], pred["var_pred"], mean, var, l1, np.abs(est["z"]).max())
    print(f"vecchia_pred(local=True): max mean error {em:.3g}, max var error {ev:.3g}")
    assert est["trend"] == "constant" and em <= BAR and ev <= BAR
