"""gpv_plan_selinv / Plan.selinv / vecchia_selinv / vecchia_prediction(var_exact=False) on the GPU (gpv_selinv.hip): every
posterior variance from ONE pass of the selected inverse of the posterior factor on its own pattern.

Against the plan's exact route (unit rows of gpv_plan_lincomb, lincomb.exact_variances_device) where the pattern drops nothing,
and against the dense numpy restatement of the recursion with the zero-fill rule (tests/_selinv_truth.py, on the oracle's dense
U of the same approximation) where it drops pairs.  Every comparison: the project's flat tolerance of tests/test_gpu_lincomb.py,
|got - ref| <= 1e-8 max(1, max|ref|); the dropped counts are compared exactly.

Run as a script (`python tests/test_gpu_selinv.py OUT.npy`) this file evaluates the first plan of case 1 and saves two
successive results of Plan.selinv: the tests start it in fresh child processes under GPV_POST_TOP=0 / 64 / 128 and
GPV_NO_GRAPH=1, switches the library reads once."""
import ctypes as C
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CP = [1.0, 0.15, 1.5]


def _need_gpu():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


def _to_oracle_va(va):
    prep = dict(va["U_prep"])
    nn = prep["revNNarray"]
    prep["revNNarray"] = np.where(nn == 0, np.nan, nn.astype(np.float64))
    prep["revCond"] = np.where(prep["revCond"] < 0, np.nan, prep["revCond"].astype(np.float64))
    out = {k: v for k, v in va.items() if not isinstance(k, tuple)}
    out["U_prep"] = prep
    return out


def _close(name, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max()) / scale
    print(f"{name}: {got.size} values, max |got - ref| / max(1, max|ref|) = {err:.3e}")
    assert got.shape == ref.shape and err <= RTOL, (name, err)


def _data(n, dim, seed):
    rng = np.random.default_rng(seed)
    return rng.random((n, dim)), rng.standard_normal(n), 0.05 + 0.1 * rng.random(n)


def _truth(va, tau):
    """(diag, n_dropped) of the recursion on the oracle's dense U of this approximation, ordered latent layout."""
    from oracle import r_side as R
    import _selinv_truth as T
    Uo = R.createU(_to_oracle_va(va), CP, tau)
    Rf, pattern = T.latent_factor(Uo)
    return T.selinv_truth(Rf, pattern)


# ---- 1. exact against the existing exact route -----------------------------------------------------------------------------
def _case1(G, n=700, m=10, dim=2, ordering="maxmin", seed=31):
    locs, z, tau = _data(n, dim, seed)
    va = G.vecchia_specify(locs, m, ordering=ordering, cond_yz="SGV")
    preds = G.vecchia_prediction(z, va, CP, tau, return_values="meanmat")
    return va, preds, (locs, z, tau)


@pytest.fixture(scope="module")
def case1():
    G = _need_gpu()
    from gpvecchia_amd import lincomb as LC
    va, preds, data = _case1(G)
    plan = preds["factor"]["plan"]
    return dict(va=va, preds=preds, plan=plan, data=data, exact=LC.exact_variances_device(plan, plan.Nlocs), sel=plan.selinv())


def test_first_plan_has_scheduled_levels_and_equals_the_exact_route(case1):
    c = case1
    assert c["plan"].Nlocs == 700 and c["plan"].posterior_levels() >= 2          # columns beyond the 128 of the top block
    v, dropped = c["sel"]
    assert dropped == 0
    _close("case 1, n = 700, m = 10", v, c["exact"])
    assert np.all(v > 0)


@pytest.mark.parametrize("n,m,dim,ordering", [(600, 40, 2, "maxmin"), (300, 63, 3, "maxmin"), (500, 10, 2, "none")])
def test_exact_on_sgv_plans(n, m, dim, ordering):
    """m = 40: columns of more than 32 entries; m = 63: row length 64, the limit; ordering 'none': long chains, narrow levels."""
    G = _need_gpu()
    from gpvecchia_amd import lincomb as LC
    va, preds, _ = _case1(G, n, m, dim, ordering, seed=n + m)
    plan = preds["factor"]["plan"]
    v, dropped = plan.selinv()
    assert dropped == 0
    _close(f"SGV n = {n}, m = {m}, {dim}-D, {ordering}", v, LC.exact_variances_device(plan, n))


# ---- 2. simple and filled patterns -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [5, 0])
def test_z_plans_have_a_diagonal_latent_block(m):
    G = _need_gpu()
    from gpvecchia_amd import lincomb as LC
    n = 400
    locs, z, tau = _data(n, 2, 40 + m)
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="z")
    preds = G.vecchia_prediction(z, va, CP, tau, return_values="meanmat")
    plan = preds["factor"]["plan"]
    v, dropped = plan.selinv()
    assert dropped == 0
    _close(f"'z', m = {m}: exact route", v, LC.exact_variances_device(plan, n))
    from oracle import r_side as R
    import _selinv_truth as T
    Rf, _ = T.latent_factor(R.createU(_to_oracle_va(va), CP, tau))
    assert np.count_nonzero(Rf - np.diag(np.diag(Rf))) == 0
    _close(f"'z', m = {m}: 1 / R_kk^2", v, 1.0 / np.diag(Rf) ** 2)


def test_y_on_the_filled_structure_is_exact():
    """cond.yz = 'y', n = 400, m = 5, through gpv_plan_build_posterior_fill: the filled pattern is closed, nothing is dropped."""
    G = _need_gpu()
    from gpvecchia_amd import lincomb as LC
    n, m = 400, 5
    locs, z, tau = _data(n, 2, 45)
    # coordinate ordering: the filled factor has 4.5 times the entries of B and columns of up to 40 rows (maxmin: 129, refused)
    va = G.vecchia_specify(locs, m, ordering="coord", cond_yz="y")
    plan = G.api._plan_for(va, 0)
    ratio = plan.build_posterior_fill(max_fill=8.0)
    assert ratio is not None and ratio > 1.0, ratio
    plan.set_data(z[va["ord_z"] - 1])
    plan.eval("matern", CP, tau[va["ord"] - 1], G.GPV_WANT_MEAN)
    v, dropped = plan.selinv()
    print("'y' filled: fill ratio", ratio)
    assert dropped == 0
    _close("'y' on the filled pattern", v, LC.exact_variances_device(plan, n))
    from oracle import r_side as R
    Uo = R.createU(_to_oracle_va(va), CP, tau)
    Uy = Uo["U"][np.asarray(Uo["latent"], dtype=bool), :]
    _close("'y' on the filled pattern: diag(W^-1)", v, np.diag(np.linalg.inv(Uy @ Uy.T)))


# ---- 3. patterns that drop pairs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2])
def test_sgv_prediction_plan_equals_the_truth_with_dropped_pairs(dim):
    G = _need_gpu()
    n, n_p, m = 300, 80, 8
    rng = np.random.default_rng(50 + dim)
    locs, lp = rng.random((n, dim)), rng.random((n_p, dim))
    z, tau = rng.standard_normal(n), 0.05 + 0.1 * rng.random(n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        va = G.vecchia_specify(locs, m, ordering="maxmin" if dim == 2 else "coord", cond_yz="SGV", locs_pred=lp,
                               ordering_pred="obspred")
        preds = G.vecchia_prediction(z, va, CP, tau, return_values="meanmat")
    assert preds.get("route") == "device"                               # (gpv_plan_set_observed)
    plan = preds["factor"]["plan"]
    assert plan.Nlocs == n + n_p
    v, dropped = plan.selinv()
    ref, ref_dropped = _truth(va, tau)
    print(f"SGV prediction plan, {dim}-D: dropped {dropped} (truth {ref_dropped})")
    assert dropped == ref_dropped and dropped > 0
    _close(f"SGV prediction plan, {dim}-D", v, ref)
    out = G.vecchia_selinv(preds)
    vo, vp = G.api.split_mean(ref, dict(ord=va["ord"], obs=va["obs"]))
    assert out["n_dropped"] == dropped and out["var_obs"].shape == (n,) and out["var_pred"].shape == (n_p,)
    _close("vecchia_selinv var_obs", out["var_obs"], vo)
    _close("vecchia_selinv var_pred", out["var_pred"], vp)


def test_zy_plan_equals_the_truth_and_the_dummy_rows_are_zero():
    G = _need_gpu()
    n, n_p, m = 400, 150, 8
    rng = np.random.default_rng(60)
    locs, lp = rng.random((n, 2)), rng.random((n_p, 2))
    z, tau = rng.standard_normal(n), 0.05 + 0.1 * rng.random(n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="zy", locs_pred=lp, ordering_pred="obspred")
        preds = G.vecchia_prediction(z, va, CP, tau, return_values="meanmat")
    fac = preds["factor"]
    plan = fac["plan"]
    assert fac["offset"] == n and plan.Nlocs == 2 * n + n_p
    v, dropped = plan.selinv(skip_front=n)
    ref, ref_dropped = _truth(va, tau)
    print(f"'zy' plan: dropped {dropped} (truth {ref_dropped})")
    assert dropped == ref_dropped
    assert np.all(v[:n] == 0.0)
    _close("'zy' plan", v[n:], ref)


# ---- 4. switches -----------------------------------------------------------------------------------------------------------
def _child(tmp_path, name, env_extra):
    out = str(tmp_path / f"{name}.npy")
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out)


_RUNS = {}                                                             # results of the children that have run, by switch


@pytest.mark.parametrize("name,env", [("top0", {"GPV_POST_TOP": "0"}), ("top64", {"GPV_POST_TOP": "64"}),
                                      ("top128", {"GPV_POST_TOP": "128"}), ("nograph", {"GPV_NO_GRAPH": "1"})])
def test_switches_in_fresh_processes(case1, tmp_path, name, env):
    """One child per switch.  Every form of the top block agrees with the exact route, with this process and with the
    children before it to the flat tolerance; two calls in one process give the same bits; the default form (128) and the
    launch-by-launch replay give the bits of this process's captured graph."""
    r = _child(tmp_path, name, env)
    assert r.shape == (2, 700)
    assert np.array_equal(r[0], r[1])
    _close(f"{name} against the exact route", r[0], case1["exact"])
    _close(f"{name} against this process", r[0], case1["sel"][0])
    for other, v in _RUNS.items():
        _close(f"{name} against {other}", r[0], v)
    if name in ("top128", "nograph"):
        assert np.array_equal(r[0], case1["sel"][0])
    _RUNS[name] = r[0]


# ---- 5. read-only, statuses ------------------------------------------------------------------------------------------------
def test_the_factor_is_only_read(case1):
    import scipy.sparse as sp
    c = case1
    plan, n = c["plan"], 700
    H = sp.identity(n, format="csr")[[0, 5, 130, n - 1]]
    e = np.zeros(n)
    e[n // 2] = 1.0
    before = (plan.factor_stamp(), plan.lincomb(H), plan.solve_t(e), plan.posterior_mean())
    v, _ = plan.selinv()
    after = (plan.factor_stamp(), plan.lincomb(H), plan.solve_t(e), plan.posterior_mean())
    assert before[0] == after[0] != 0
    for b, a in zip(before[1:], after[1:]):
        assert np.array_equal(b, a)
    assert np.array_equal(v, c["sel"][0])
    assert np.array_equal(c["preds"]["mu_obs"][c["va"]["ord"] - 1], after[3])


def test_statuses():
    G = _need_gpu()
    from gpvecchia_amd import _lib as L
    n = 300
    locs, z, tau = _data(n, 2, 70)
    va = G.vecchia_specify(locs, 5, ordering="maxmin", cond_yz="z")
    plan = G.api._plan_for(va, 0)
    out, nd = np.zeros(n), C.c_int64(-1)
    call = lambda skip, vars_: L.lib().gpv_plan_selinv(plan._h, skip, vars_, C.byref(nd))
    assert call(0, L.dptr(out)) == 7                                   # GPV_ERR_STATE: no posterior structure
    assert plan.ensure_posterior()
    assert call(0, L.dptr(out)) == 7                                   # no evaluation
    plan.set_data(z[va["ord_z"] - 1])
    plan.eval("matern", CP, tau[va["ord"] - 1], G.GPV_WANT_LOGLIK_Z)
    assert call(0, L.dptr(out)) == 7                                   # an evaluation without a posterior pass
    assert call(0, None) == 2                                          # GPV_ERR_BAD_ARG before the state is looked at
    plan.eval("matern", CP, tau[va["ord"] - 1], G.GPV_WANT_DENOM)
    assert call(0, None) == 2 and call(-1, L.dptr(out)) == 2 and call(n, L.dptr(out)) == 2
    assert L.lib().gpv_plan_selinv(plan._h, 0, L.dptr(out), None) == 2
    assert nd.value == -1 and np.all(out == 0.0)                       # nothing was written by a refused call
    assert call(n - 1, L.dptr(out)) == 0 and nd.value == 0
    assert np.all(out[:n - 1] == 0.0) and out[n - 1] > 0


# ---- 6. Python -------------------------------------------------------------------------------------------------------------
def test_vecchia_prediction_var_exact_false_takes_the_selected_inverse(case1, monkeypatch):
    G = _need_gpu()
    from gpvecchia_amd import lincomb as LC
    locs, z, tau = case1["data"]
    va = case1["va"]
    exact = G.vecchia_prediction(z, va, CP, tau, return_values="meanvar", var_exact=True)
    default = G.vecchia_prediction(z, va, CP, tau, return_values="meanvar")
    assert "var_dropped" not in exact and "var_dropped" not in default
    assert np.array_equal(exact["var_obs"], default["var_obs"])

    def refuse(*a, **k):
        raise AssertionError("var_exact=False must not take the unit-row route")
    monkeypatch.setattr(LC, "exact_variances_device", refuse)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                  # nothing is dropped: no warning
        sel = G.vecchia_prediction(z, va, CP, tau, return_values="all", var_exact=False)
    assert sel["var_dropped"] == 0 and sel["var_pred"].shape == (0,)
    assert np.array_equal(sel["mu_obs"], exact["mu_obs"])
    _close("var_exact=False against True", sel["var_obs"], exact["var_obs"])
    # the handle of that prediction serves vecchia_selinv until the plan is evaluated again
    out = G.vecchia_selinv(sel)
    assert out["n_dropped"] == 0 and np.array_equal(out["var_obs"], sel["var_obs"])
    G.vecchia_prediction(z, va, [2.0, 0.2, 1.5], tau)
    with pytest.raises(RuntimeError, match="evaluated again"):
        G.vecchia_selinv(sel)


def test_prediction_plan_warns_that_pairs_are_dropped():
    G = _need_gpu()
    rng = np.random.default_rng(52)
    n, n_p = 300, 80
    locs, lp = rng.random((n, 2)), rng.random((n_p, 2))
    z, tau = rng.standard_normal(n), 0.05 + 0.1 * rng.random(n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        va = G.vecchia_specify(locs, 8, ordering="maxmin", cond_yz="SGV", locs_pred=lp, ordering_pred="obspred")
    with pytest.warns(UserWarning, match="var.exact = FALSE"):
        sel = G.vecchia_prediction(z, va, CP, tau, return_values="meanvar", var_exact=False)
    ref, ref_dropped = _truth(va, tau)
    assert sel["var_dropped"] == ref_dropped > 0
    vo, vp = G.api.split_mean(ref, dict(ord=va["ord"], obs=va["obs"]))
    _close("prediction plan var_obs", sel["var_obs"], vo)
    _close("prediction plan var_pred", sel["var_pred"], vp)


def test_vecchia_laplace_prediction_passes_var_exact_through(monkeypatch):
    G = _need_gpu()
    from gpvecchia_amd import lincomb as LC
    rng = np.random.default_rng(13)
    n, m = 500, 10
    locs = rng.random((n, 2))
    cp = [0.5, 0.2, 1.5]
    z = rng.poisson(np.exp(0.5 * np.sin(5 * locs[:, 0]) + 0.3 * rng.standard_normal(n))).astype(np.float64)
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="SGV")
    vl = G.calculate_posterior_VL(z, va, "poisson", covparms=cp)
    assert vl["cnvgd"]
    exact = G.vecchia_laplace_prediction(vl, va, cp, return_values="meanvar")
    monkeypatch.setattr(LC, "exact_variances_device", lambda *a, **k: (_ for _ in ()).throw(AssertionError("unit-row route")))
    sel = G.vecchia_laplace_prediction(vl, va, cp, return_values="meanvar", var_exact=False)
    assert sel["var_dropped"] == 0 and "var_dropped" not in exact
    _close("Vecchia-Laplace var_obs", sel["var_obs"], exact["var_obs"])
    _close("Vecchia-Laplace upper quantiles", sel["data_obs_upper_quantiles"], exact["data_obs_upper_quantiles"])


if __name__ == "__main__":
    import torch  # noqa: F401  (first: see tests/conftest.py)
    sys.path.insert(0, ROOT)
    import gpvecchia_amd as G
    _, preds, _ = _case1(G)
    plan = preds["factor"]["plan"]
    np.save(sys.argv[1], np.stack([plan.selinv()[0], plan.selinv()[0]]))
