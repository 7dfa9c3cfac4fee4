"""gpv_plan_lincomb / vecchia_lincomb / the exact posterior variances of vecchia_prediction on the GPU
(gpv_lincomb.hip) against the ORACLE's sparse chain: createU_sparse -> U2V_sparse -> _tri_solve(V, rev(h)) -> sum of
squares, which is vecchia_lincomb (R/vecchia_prediction.R:164-178) restated literally, and against dense numpy identities.

Tolerance: the project's flat 1e-8 relative to max(1, max|truth|).  A row beyond it is adjudicated like the posterior mean
(tests/test_gpu_posterior_oracle.py): both sides against the chain in x87 extended precision, err_hip <= max(4 err_oracle,
1e-8), for at most 1 row in 10; implemented for plans without prediction locations, the others hold the flat tolerance.

Run as a script (`python tests/test_gpu_lincomb.py OUT.npy`) this file evaluates case 2 below and saves its variances: the
tests start it in fresh child processes under GPV_NO_GRAPH=1 and GPV_POST_TOP=0, switches the library reads once."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _prep_V(V):
    import scipy.sparse as sp
    V = sp.csc_matrix(V)
    V.sort_indices()
    return sp.csc_matrix((V.data, V.indices.astype(np.int64), V.indptr.astype(np.int64)), shape=V.shape)


def _oracle_temp(V, ord_, H):
    """vecchia_lincomb's temp = solve(V.ord, t(H[, rev(ord)])), one column per row of H (R/vecchia_prediction.R:169-170)."""
    from oracle import r_side as R
    import scipy.sparse as sp
    Hrev = sp.csr_matrix(H)[:, (np.asarray(ord_) - 1)[::-1]].toarray()
    return np.stack([R._tri_solve(V, h) for h in Hrev], axis=1)


def _oracle_unit_vars(V, nlat):
    """diag(W^-1) in ordered layout: the unit rows of vecchia_var's exact branch (:223-244) on the oracle's own V."""
    from oracle import r_side as R
    out = np.empty(nlat)
    for p in range(nlat):
        e = np.zeros(nlat, dtype=V.dtype)
        e[nlat - 1 - p] = 1.0
        t = R._tri_solve(V, e)
        out[p] = float(np.sum(t * t))
    return out


def _extended_V(va, cp, tau):
    """V.ord of a plan without prediction locations in x87 extended precision: the factor part of
    oracle.r_side.posterior_extended (rows_extended -> createU_sparse -> long double W and Cholesky)."""
    from oracle import r_side as R
    import scipy.sparse as sp
    ld = np.longdouble
    vb = _to_oracle_va(va)
    prep = vb["U_prep"]
    n = int(np.sum(vb["obs"]))
    nug = np.repeat(np.asarray(tau, dtype=np.float64), n) if np.size(tau) == 1 else np.asarray(tau, dtype=np.float64)
    Lx = R.rows_extended(np.arange(n), vb["locsord"], prep["revNNarray"], prep["revCond"], nug[vb["ord"] - 1], "matern", cp)
    zd = 1.0 / np.sqrt(nug[vb["ord_z"] - 1].astype(ld))
    Zx = np.stack([-zd, zd], axis=1).reshape(-1).astype(np.float64)
    Us = R.createU_sparse(vb, cp, nug, "matern", U_entries=dict(Lentries=Lx, Zentries=Zx))
    U = sp.csr_matrix(Us["U"]).astype(ld)
    Uy = U[np.where(np.asarray(Us["latent"], dtype=bool))[0], :]
    return R.sparse_chol_lower(R._rev_sparse(Uy @ Uy.T))


def _check_rows(name, got, ref, adjudicate=None):
    """flat 1e-8 on every row; rows beyond it go to adjudicate(rows) -> extended-precision truth (at most 1 row in 10)."""
    got, ref = np.asarray(got), np.asarray(ref)
    scale = max(1.0, float(np.abs(ref).max()))
    err = np.abs(got - ref) / scale
    bad = np.where(~(err <= RTOL))[0]
    print(f"{name}: {got.size} rows, max rel diff {err.max():.3e}, beyond 1e-8: {bad.size}")
    if bad.size == 0:
        return
    assert adjudicate is not None, (name, err.max())
    assert bad.size * 10 <= got.size, (name, bad.size, got.size)
    truth = np.asarray(adjudicate(bad), dtype=np.float64)
    err_hip, err_or = np.abs(got[bad] - truth) / scale, np.abs(ref[bad] - truth) / scale
    print(f"{name}: adjudicated rows {bad.tolist()}: err_hip {err_hip.max():.3e} err_oracle {err_or.max():.3e}")
    assert np.all(err_hip <= np.maximum(4.0 * err_or, RTOL)), (err_hip, err_or)


# ---- 1. exactness identity -------------------------------------------------------------------------------------------------
def test_exact_variances_equal_the_dense_conditional_variances():
    """Every point conditions on ALL its predecessors (m = number of locations - 1: 59 without, 74 with the 15 prediction
    locations), SGV, maxmin, Matern 1.5, vector nuggets: the Vecchia posterior is the exact one, so var_obs =
    diag(K - K (K + D)^-1 K) and var_pred the exact conditional variances, whatever the oracle says.  Tolerance: max(4 x the
    oracle chain's own error to the same identity, 1e-8)."""
    import warnings
    G = _need_gpu()
    from oracle import r_side as R
    rng = np.random.default_rng(41)
    n, n_p = 60, 15
    locs, lp = rng.random((n, 2)), rng.random((n_p, 2))
    z = rng.standard_normal(n)
    tau = 0.05 + 0.1 * rng.random(n)
    cp = [1.3, 0.25, 1.5]
    for with_pred in (False, True):
        allp = np.vstack([locs, lp]) if with_pred else locs
        N = allp.shape[0]
        K = R.MaternFun(R.rdist(allp), np.asarray(cp))
        A = K[:, :n]
        post = K - A @ np.linalg.solve(K[:n, :n] + np.diag(tau), A.T)
        truth = np.diag(post)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            va = G.vecchia_specify(locs, N - 1, ordering="maxmin", cond_yz="SGV", locs_pred=lp if with_pred else None,
                                   ordering_pred="obspred" if with_pred else None)
            pred = G.vecchia_prediction(z, va, cp, tau, return_values="meanvar")
        Us = R.createU_sparse(_to_oracle_va(va), cp, tau)
        V = _prep_V(R.U2V_sparse(Us))
        vo_obs, vo_pred = G.api.split_mean(_oracle_unit_vars(V, N), Us)
        got = np.concatenate([pred["var_obs"], pred["var_pred"]])
        ora = np.concatenate([vo_obs, vo_pred])
        scale = max(1.0, np.abs(truth).max())
        err_hip, err_or = np.abs(got - truth).max() / scale, np.abs(ora - truth).max() / scale
        print(f"exactness (pred={with_pred}): err_hip {err_hip:.3e} err_oracle {err_or:.3e}")
        assert pred["var_obs"].shape == (n,) and pred["var_pred"].shape == ((n_p,) if with_pred else (0,))
        assert err_hip <= max(4.0 * err_or, RTOL), (err_hip, err_or)


# ---- 2. schedule coverage --------------------------------------------------------------------------------------------------
def _case2(G):
    """n = 20 000, m = 20, 2-D, maxmin + SGV, vector nuggets in [0.1, 0.2], Matern 1.5, range 0.01; 40 rows of H."""
    import scipy.sparse as sp
    n, m = 20_000, 20
    rng = np.random.default_rng(23)
    locs = rng.random((n, 2)); z = rng.standard_normal(n)
    tau = 0.1 + 0.1 * rng.random(n)
    cp = [1.2, 0.01, 1.5]
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="SGV", nn_backend="gpu")
    preds = G.vecchia_prediction(z, va, cp, tau, return_values="all")
    ord_ = va["ord"]
    # 10 unit vectors by ORDERED index: the first two and one more of the dense top block, the last (a leaf), others
    unit_ord = np.array([0, 1, 30, n - 1, n - 2, 64, 200, 1000, 5000, 12345])
    rows, cols, vals = [], [], []
    for r, p in enumerate(unit_ord):
        rows.append(r); cols.append(ord_[p] - 1); vals.append(1.0)
    for r in range(10, 30):                                            # 20 random sparse rows of 50 entries
        c = rng.choice(n, 50, replace=False)
        rows += [r] * 50; cols += c.tolist(); vals += rng.standard_normal(50).tolist()
    for r in range(30, 40):                                            # 10 regional averages: all locations in a box
        lo = rng.random(2) * 0.7
        inside = np.where(np.all((locs >= lo) & (locs <= lo + 0.3), axis=1))[0]
        rows += [r] * inside.size; cols += inside.tolist(); vals += [1.0 / inside.size] * inside.size
    H = sp.csr_matrix((vals, (rows, cols)), shape=(40, n))
    return dict(va=va, preds=preds, H=H, cp=cp, tau=tau, z=z, n=n, unit_ord=unit_ord)


@pytest.fixture(scope="module")
def case2():
    G = _need_gpu()
    from oracle import r_side as R
    c = _case2(G)
    c["vars"] = G.vecchia_lincomb(c["H"], c["preds"])
    Us = R.createU_sparse(_to_oracle_va(c["va"]), c["cp"], c["tau"])
    c["V"] = _prep_V(R.U2V_sparse(Us))
    c["temp"] = _oracle_temp(c["V"], c["va"]["ord"], c["H"])
    return c


def test_schedule_coverage_vars_against_oracle(case2):
    """Top block, head, narrow and wide levels, the leaf level; one full batch and a short one."""
    G = _need_gpu()
    from oracle import r_side as R
    c = case2
    plan = c["va"][("_plan", 0)]
    levels = plan.posterior_levels()
    print("case 2: posterior levels", levels, "batch", G._lib.lib().gpv_lincomb_batch())
    assert levels >= 15
    assert c["preds"]["var_obs"].shape == (c["n"],)
    ref = np.sum(c["temp"] ** 2, axis=0)

    def adjudicate(rows):
        Vx = _prep_V(_extended_V(c["va"], c["cp"], c["tau"]))
        tx = _oracle_temp(Vx, c["va"]["ord"], c["H"][rows])
        return np.sum(tx * tx, axis=0).astype(np.float64)
    _check_rows("case 2 vars", c["vars"], ref, adjudicate)
    # the unit rows are the exact variances vecchia_prediction returned for those locations
    ord_ = c["va"]["ord"]
    assert np.array_equal(c["vars"][:10], c["preds"]["var_obs"][ord_[c["unit_ord"]] - 1])


def test_schedule_coverage_cov_mat_and_reproducibility(case2):
    G = _need_gpu()
    c = case2
    nb = G._lib.lib().gpv_lincomb_batch()
    cov = G.vecchia_lincomb(c["H"][:nb], c["preds"], cov_mat=True)
    ref = c["temp"][:, :nb].T @ c["temp"][:, :nb]
    scale = max(1.0, np.abs(ref).max())
    print("case 2 cov: max rel diff", np.abs(cov - ref).max() / scale)
    assert cov.shape == (nb, nb) and np.abs(cov - ref).max() <= RTOL * scale
    assert np.array_equal(np.diag(cov), c["vars"][:nb])               # bit for bit: the same sums in the same order
    with pytest.raises(G.GpvError) as ei:                             # more rows than one batch with a covariance matrix
        G.vecchia_lincomb(c["H"], c["preds"], cov_mat=True)
    assert ei.value.status == 2                                       # GPV_ERR_BAD_ARG
    assert np.array_equal(G.vecchia_lincomb(c["H"], c["preds"]), c["vars"])   # the same call twice: the same bits


def _child_vars(tmp_path, env_extra):
    out = str(tmp_path / "vars.npy")
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out)


def test_schedule_coverage_without_graph_is_bitwise_the_same(case2, tmp_path):
    v = _child_vars(tmp_path, {"GPV_NO_GRAPH": "1"})
    assert np.array_equal(v, case2["vars"])


def test_schedule_coverage_all_columns_scheduled_agrees(case2, tmp_path):
    """GPV_POST_TOP=0: no dense top block, every column is a column of the schedule -- the cross-check route."""
    v = _child_vars(tmp_path, {"GPV_POST_TOP": "0"})
    rel = np.abs(v - case2["vars"]) / np.abs(case2["vars"])
    print("case 2, GPV_POST_TOP=0 vs default: max rel diff", rel.max())
    assert rel.max() <= 1e-12


# ---- 3. more than 32 entries per column, a second batch --------------------------------------------------------------------
def test_long_columns_and_second_batch_against_oracle():
    """m = 40, n = 6000, SGV: columns with more than 32 latent entries (the factor pass's ld > 32 forms); 33 unit rows."""
    G = _need_gpu()
    from oracle import r_side as R
    import scipy.sparse as sp
    n, m = 6000, 40
    rng = np.random.default_rng(29)
    locs = rng.random((n, 2)); z = rng.standard_normal(n)
    tau = 0.1 + 0.1 * rng.random(n)
    cp = [1.0, 0.03, 1.5]
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="SGV")
    preds = G.vecchia_prediction(z, va, cp, tau, return_values="meanmat")
    assert preds["var_obs"] is None and "factor" in preds
    cols = np.concatenate([[va["ord"][0] - 1, va["ord"][n - 1] - 1], rng.choice(n, 31, replace=False)])
    H = sp.csr_matrix((np.ones(33), (np.arange(33), cols)), shape=(33, n))
    got = G.vecchia_lincomb(H, preds)
    Us = R.createU_sparse(_to_oracle_va(va), cp, tau)
    assert int(np.diff(sp.csc_matrix(Us["U"])[np.where(Us["latent"])[0], :][:, np.where(Us["latent"])[0]].indptr).max()) > 32
    V = _prep_V(R.U2V_sparse(Us))
    ref = np.sum(_oracle_temp(V, va["ord"], H) ** 2, axis=0)

    def adjudicate(rows):
        tx = _oracle_temp(_prep_V(_extended_V(va, cp, tau)), va["ord"], H[rows])
        return np.sum(tx * tx, axis=0).astype(np.float64)
    _check_rows("case 3 vars", got, ref, adjudicate)


# ---- 4. prediction plans ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cond,ordering_pred,n,n_p", [("SGV", "obspred", 4000, 1000), ("SGVT", "obspred", 4000, 1000),
                                                      ("zy", "obspred", 4000, 1000), ("y", "general", 1500, 300)])
def test_prediction_plan_variances_against_oracle(cond, ordering_pred, n, n_p):
    import warnings
    G = _need_gpu()
    from oracle import r_side as R
    m = 15
    rng = np.random.default_rng(11)
    locs, lp = rng.random((n, 2)), rng.random((n_p, 2))
    z = np.sin(6 * locs[:, 0]) * np.cos(5 * locs[:, 1]) + 0.3 * rng.standard_normal(n)
    tau = 0.05 + 0.1 * rng.random(n)
    cp = [1.0, 0.05, 1.5]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz=cond, locs_pred=lp, ordering_pred=ordering_pred)
        mean_only = G.vecchia_prediction(z, va, cp, tau)
        pred = G.vecchia_prediction(z, va, cp, tau, return_values="meanvar")
    if cond == "y" and pred.get("route") != "device":
        pytest.skip("build_posterior_fill refused the filled structure of this plan: the host route served it")
    assert mean_only["var_obs"] is None and mean_only["var_pred"] is None
    assert np.array_equal(mean_only["mu_obs"], pred["mu_obs"]) and np.array_equal(mean_only["mu_pred"], pred["mu_pred"])
    assert pred["var_obs"].shape == (n,) and pred["var_pred"].shape == (n_p,)
    assert np.all(pred["var_obs"] > 0) and np.all(pred["var_pred"] > 0)
    if cond == "SGV":
        assert pred.get("route") == "device"
    Us = R.createU_sparse(_to_oracle_va(va), cp, tau)
    V = _prep_V(R.U2V_sparse(Us))
    vo_obs, vo_pred = G.api.split_mean(_oracle_unit_vars(V, n + n_p), Us)
    _check_rows(f"case 4 {cond} var_obs", pred["var_obs"], vo_obs)
    _check_rows(f"case 4 {cond} var_pred", pred["var_pred"], vo_pred)


# ---- 5. state --------------------------------------------------------------------------------------------------------------
def test_lincomb_state_and_index_errors():
    import ctypes as C
    import scipy.sparse as sp
    G = _need_gpu()
    from gpvecchia_amd import _lib as L
    rng = np.random.default_rng(7)
    n = 500
    locs = rng.random((n, 2)); z = rng.standard_normal(n)
    va = G.vecchia_specify(locs, 10, ordering="maxmin", cond_yz="SGV")
    plan = G.api._plan_for(va, 0)
    assert plan.ensure_posterior() and plan.factor_stamp() == 0
    with pytest.raises(G.GpvError) as ei:                             # structure, but no posterior evaluation yet
        plan.lincomb(sp.identity(n, format="csr")[:3])
    assert ei.value.status == 7                                       # GPV_ERR_STATE
    preds = G.vecchia_prediction(z, va, [1.0, 0.1, 1.5], 0.1, return_values="all")
    H = sp.identity(n, format="csr")[:5]
    v = G.vecchia_lincomb(H, preds)
    assert np.array_equal(v, preds["var_obs"][:5])
    hptr = np.array([0, 1], dtype=np.int64); hval = np.ones(1); out = np.zeros(1)
    for idx, status in ((n, 8), (-1, 8), (n - 1, 0)):                 # GPV_ERR_INDEX: an index equal to Nlocs
        hidx = np.array([idx], dtype=np.int32)
        st = L.lib().gpv_plan_lincomb(plan._h, 1, hptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                      hidx.ctypes.data_as(C.POINTER(C.c_int32)), L.dptr(hval), L.dptr(out), None)
        assert st == status, (idx, st)
    # repeated indices within a row add in the order given: (0.25 + 0.75) e_k is e_k
    hptr = np.array([0, 2], dtype=np.int64); hidx = np.array([n - 1, n - 1], dtype=np.int32); hval = np.array([0.25, 0.75])
    two = np.zeros(1)
    assert L.lib().gpv_plan_lincomb(plan._h, 1, hptr.ctypes.data_as(C.POINTER(C.c_int64)), hidx.ctypes.data_as(C.POINTER(C.c_int32)),
                                    L.dptr(hval), L.dptr(two), None) == 0
    assert two[0] == out[0]
    # another evaluation of the plan: the old prediction's factor is gone
    plan.eval("matern", [2.0, 0.2, 1.5], 0.3, G.GPV_WANT_DENOM)
    with pytest.raises(RuntimeError, match="evaluated again"):
        G.vecchia_lincomb(H, preds)


# ---- 6. vecchia_pred -------------------------------------------------------------------------------------------------------
def test_vecchia_pred_returns_prediction_variances():
    """The reference's own example shape (R/vecchia_prediction.R:13-14): locs = 1:5, locs.pred = locs + .5, m = 3,
    covparms = c(1, 2, .5), nuggets = .2.  var_pred against dense algebra on the oracle's U of the same approximation."""
    import warnings
    G = _need_gpu()
    from oracle import r_side as R
    locs = np.arange(1.0, 6.0)[:, None]
    lp = locs + 0.5
    z = np.random.default_rng(3).standard_normal(5)
    est = dict(locs=locs, z=z, theta_hat=np.array([1.0, 2.0, 0.5, 0.2]), covmodel="matern", trend="none", beta_hat=np.array([]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = G.vecchia_pred(est, lp, m=3)
        va = G.vecchia_specify(locs, 3, locs_pred=lp)
    assert out["mean_pred"].shape == (5,) and out["var_pred"].shape == (5,)
    assert np.all(np.isfinite(out["var_pred"])) and np.all(out["var_pred"] > 0)
    Uo = R.createU(_to_oracle_va(va), [1.0, 2.0, 0.5], 0.2)
    lat = np.asarray(Uo["latent"], dtype=bool)
    if va["cond_yz"] == "zy":
        B = Uo["U"][np.ix_(lat, lat)]
        Winv = np.linalg.inv(B @ B.T)
    else:
        Uy = Uo["U"][lat, :]
        Winv = np.linalg.inv(Uy @ Uy.T)
    _, ref = G.api.split_mean(np.diag(Winv), Uo)
    np.testing.assert_allclose(out["var_pred"], ref, rtol=0, atol=RTOL * max(1.0, np.abs(ref).max()))


if __name__ == "__main__":
    import torch  # noqa: F401  (first: see tests/conftest.py)
    sys.path.insert(0, ROOT)
    import gpvecchia_amd as G
    c = _case2(G)
    np.save(sys.argv[1], G.vecchia_lincomb(c["H"], c["preds"]))
