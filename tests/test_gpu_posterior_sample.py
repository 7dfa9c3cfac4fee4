"""gpv_plan_solve_t / Plan.solve_t / vecchia_posterior_sample on the GPU (gpv_lincomb.hip, the transposed sweep R^T X = E)
against the ORACLE's sparse chain: createU_sparse -> U2V_sparse gives the reversed lower V (V V^T = rev(W)), and
rev(x) = _tri_solve(V, rev(e), transpose=True).  The Cholesky factor with positive diagonal is unique, so the solves are
compared element by element, not in distribution.

Tolerance, per right-hand side: max|got - ref| / max(1, max|ref|) <= 1e-8.  A column beyond it is adjudicated like the rows
of tests/test_gpu_lincomb.py: both sides against the chain in x87 extended precision, err_hip <= max(4 err_oracle, 1e-8), for
at most 1 column in 10 (plans without prediction locations; the others hold the flat tolerance).

Run as a script (`python tests/test_gpu_posterior_sample.py OUT.npy`) this file solves case 2 below and saves X: the tests
start it in fresh child processes under GPV_NO_GRAPH=1 and GPV_POST_TOP=0, switches the library reads once."""
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


def _oracle_solve_t(V, E_ord):
    """rows e of E_ord (ordered layout): x = R^-T e through the reversed factor, rev(x) = V^-T rev(e)."""
    from oracle import r_side as R
    return np.stack([R._tri_solve(V, np.asarray(e)[::-1], transpose=True)[::-1] for e in np.atleast_2d(E_ord)], axis=0)


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


def _check_cols(name, got, ref, adjudicate=None):
    """flat 1e-8 on every right-hand side (a row of got / ref); those beyond it go to adjudicate(indices) ->
    extended-precision truth (at most 1 in 10)."""
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = np.maximum(1.0, np.abs(ref).max(axis=1))
    err = np.abs(got - ref).max(axis=1) / scale
    bad = np.where(~(err <= RTOL))[0]
    print(f"{name}: {got.shape[0]} right-hand sides, max rel diff {err.max():.3e}, beyond 1e-8: {bad.size}")
    if bad.size == 0:
        return
    assert adjudicate is not None, (name, err.max())
    assert bad.size * 10 <= got.shape[0], (name, bad.size, got.shape[0])
    truth = np.asarray(adjudicate(bad), dtype=np.float64)
    err_hip = np.abs(got[bad] - truth).max(axis=1) / scale[bad]
    err_or = np.abs(ref[bad] - truth).max(axis=1) / scale[bad]
    print(f"{name}: adjudicated {bad.tolist()}: err_hip {err_hip.max():.3e} err_oracle {err_or.max():.3e}")
    assert np.all(err_hip <= np.maximum(4.0 * err_or, RTOL)), (err_hip, err_or)


def _split_rows(X_ord, U_obj):
    orig = np.argsort(U_obj["ord"], kind="stable")
    X = np.asarray(X_ord)[:, orig]
    obs = np.asarray(U_obj["obs"], dtype=bool)[orig]
    return X[:, obs], X[:, ~obs]


# ---- 1. exactness identity -------------------------------------------------------------------------------------------------
def test_draws_with_identity_noise_give_the_dense_posterior_covariance():
    """Every point conditions on ALL its predecessors (m = N - 1), SGV, maxmin, Matern 1.5, vector nuggets: the Vecchia
    posterior is the exact one, so with E = I_N (three batches, the last one short) the solves' outer products sum to
    K - K_{.o} (K_oo + D)^-1 K_{o.}, whatever the oracle says.  Tolerance: max(4 x the oracle chain's own error to the same
    identity, 1e-8)."""
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
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            va = G.vecchia_specify(locs, N - 1, ordering="maxmin", cond_yz="SGV", locs_pred=lp if with_pred else None,
                                   ordering_pred="obspred" if with_pred else None)
            pred = G.vecchia_prediction(z, va, cp, tau, return_values="all")
        out = G.vecchia_posterior_sample(pred, eps=np.eye(N))
        assert out["y_obs"].shape == (N, n) and out["y_pred"].shape == ((N, n_p) if with_pred else (N, 0))
        X = np.hstack([out["y_obs"] - pred["mu_obs"], out["y_pred"] - pred["mu_pred"]])
        Us = R.createU_sparse(_to_oracle_va(va), cp, tau)
        V = _prep_V(R.U2V_sparse(Us))
        Xo = np.hstack(_split_rows(_oracle_solve_t(V, np.eye(N)), Us))
        scale = max(1.0, np.abs(post).max())
        err_hip, err_or = np.abs(X.T @ X - post).max() / scale, np.abs(Xo.T @ Xo - post).max() / scale
        print(f"exactness (pred={with_pred}): err_hip {err_hip:.3e} err_oracle {err_or:.3e}")
        assert err_hip <= max(4.0 * err_or, RTOL), (err_hip, err_or)
        # and the exact variances of the same prediction are the diagonal
        got_var = np.concatenate([pred["var_obs"], pred["var_pred"]])
        assert np.abs(np.sum(X * X, axis=0) - got_var).max() <= RTOL * scale


# ---- 2. schedule coverage --------------------------------------------------------------------------------------------------
UNIT_ORD = lambda n: np.array([0, 1, 30, 64, 200, 1000, 5000, 12345, n - 2, n - 1])   # top block .. leaves


def _case2(G):
    """n = 20 000, m = 20, 2-D, maxmin + SGV, vector nuggets in [0.1, 0.2], Matern 1.5, range 0.01; 40 right-hand sides in
    ORDERED layout: 30 standard-normal columns, 10 unit vectors."""
    n, m = 20_000, 20
    rng = np.random.default_rng(23)
    locs = rng.random((n, 2)); z = rng.standard_normal(n)
    tau = 0.1 + 0.1 * rng.random(n)
    cp = [1.2, 0.01, 1.5]
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="SGV", nn_backend="gpu")
    preds = G.vecchia_prediction(z, va, cp, tau, return_values="meanmat")
    E = np.zeros((40, n))
    E[:30] = np.random.default_rng(101).standard_normal((30, n))
    E[np.arange(30, 40), UNIT_ORD(n)] = 1.0
    plan = G.api._plan_for(va, 0)
    return dict(va=va, preds=preds, plan=plan, E=E, cp=cp, tau=tau, n=n)


@pytest.fixture(scope="module")
def case2():
    G = _need_gpu()
    from oracle import r_side as R
    c = _case2(G)
    c["X"] = c["plan"].solve_t(c["E"])
    Us = R.createU_sparse(_to_oracle_va(c["va"]), c["cp"], c["tau"])
    c["V"] = _prep_V(R.U2V_sparse(Us))
    c["ref"] = _oracle_solve_t(c["V"], c["E"])
    return c


def test_schedule_coverage_solves_against_oracle(case2):
    """Top block, narrow and wide levels, the leaf level; one full batch and one of 8."""
    c = case2
    levels = c["plan"].posterior_levels()
    print("case 2: posterior levels", levels)
    assert levels >= 15
    assert c["X"].shape == c["E"].shape

    def adjudicate(cols):
        Vx = _prep_V(_extended_V(c["va"], c["cp"], c["tau"]))
        return _oracle_solve_t(Vx, c["E"][cols]).astype(np.float64)
    _check_cols("case 2 solves", c["X"], c["ref"], adjudicate)
    # R^-T is lower triangular: the solve of a unit vector at ordered index p is zero in front of p
    for r, p in zip(range(30, 40), UNIT_ORD(c["n"])):
        assert np.all(c["X"][r, :p] == 0.0) and c["X"][r, p] > 0.0


def test_schedule_coverage_public_function_and_reproducibility(case2):
    G = _need_gpu()
    c = case2
    stamp = c["plan"].factor_stamp()
    out = G.vecchia_posterior_sample(c["preds"], eps=c["E"][28:33])
    assert out["y_obs"].shape == (5, c["n"]) and out["y_pred"].shape == (5, 0)
    ord_ = c["va"]["ord"]
    want = np.empty((5, c["n"]))
    want[:, ord_ - 1] = c["X"][28:33]                               # ordered position p is the caller's location ord[p]
    assert np.array_equal(out["y_obs"], c["preds"]["mu_obs"][None, :] + want)   # mu + the solves, in the caller's order
    assert np.array_equal(c["plan"].solve_t(c["E"]), c["X"])          # the same call twice: the same bits
    assert c["plan"].factor_stamp() == stamp                          # the factor is only read
    one = c["plan"].solve_t(c["E"][7])                                # a single vector: shape (Nlocs,), a batch of one
    assert one.shape == (c["n"],) and np.array_equal(one, c["X"][7])
    # the same column at position 0 and at position 31 of a batch
    E2 = np.random.default_rng(5).standard_normal((32, c["n"]))
    E2[0] = c["E"][3]; E2[31] = c["E"][3]
    X2 = c["plan"].solve_t(E2)
    assert np.array_equal(X2[0], X2[31]) and np.array_equal(X2[0], c["X"][3])


def _child_solves(tmp_path, env_extra):
    out = str(tmp_path / "X.npy")
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out)


def test_schedule_coverage_without_graph_is_bitwise_the_same(case2, tmp_path):
    X = _child_solves(tmp_path, {"GPV_NO_GRAPH": "1"})
    assert np.array_equal(X, case2["X"])


def test_schedule_coverage_all_columns_scheduled_agrees(case2, tmp_path):
    """GPV_POST_TOP=0: no dense top block, every column is a column of the schedule -- the cross-check route."""
    X = _child_solves(tmp_path, {"GPV_POST_TOP": "0"})
    scale = np.maximum(1.0, np.abs(case2["X"]).max(axis=1))
    rel = np.abs(X - case2["X"]).max(axis=1) / scale
    print("case 2, GPV_POST_TOP=0 vs default: max rel diff", rel.max())
    assert rel.max() <= RTOL


# ---- 3. more than 32 entries per column, a second batch --------------------------------------------------------------------
def test_long_columns_and_second_batch_against_oracle():
    """m = 40, n = 6000, SGV: columns with more than 32 latent entries (the ld > 32 forms); 33 right-hand sides."""
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
    E = rng.standard_normal((33, n))
    E[0] = 0.0; E[0, 0] = 1.0
    E[32] = 0.0; E[32, n - 1] = 1.0
    got = G.api._plan_for(va, 0).solve_t(E)
    Us = R.createU_sparse(_to_oracle_va(va), cp, tau)
    assert int(np.diff(sp.csc_matrix(Us["U"])[np.where(Us["latent"])[0], :][:, np.where(Us["latent"])[0]].indptr).max()) > 32
    V = _prep_V(R.U2V_sparse(Us))
    ref = _oracle_solve_t(V, E)

    def adjudicate(cols):
        return _oracle_solve_t(_prep_V(_extended_V(va, cp, tau)), E[cols]).astype(np.float64)
    _check_cols("case 3 solves", got, ref, adjudicate)
    out = G.vecchia_posterior_sample(preds, eps=E[:2])
    assert np.array_equal(out["eps"], E[:2]) and out["y_obs"].shape == (2, n)


# ---- 4. prediction plans ---------------------------------------------------------------------------------------------------
# (cond, ordering.pred, n, n_p, dimension, m, covparms, served by the device).  The 2-D 'y' plan is the one
# tests/test_gpu_lincomb.py::test_prediction_plan_variances_against_oracle uses: build_posterior_fill refuses its fill, the host
# route serves it, and the draws are held to the same oracle there.  The filled pattern the device accepts is the
# one-dimensional 'y' plan of tests/test_gpu_prediction.py (banded factor, little fill; exponential kernel, see there).
_CASE4 = [("SGV", "obspred", 4000, 1000, 2, 15, [1.0, 0.05, 1.5], True), ("SGVT", "obspred", 4000, 1000, 2, 15, [1.0, 0.05, 1.5], True),
          ("zy", "obspred", 4000, 1000, 2, 15, [1.0, 0.05, 1.5], True), ("y", "general", 1500, 300, 2, 15, [1.0, 0.05, 1.5], None),
          ("y", "general", 700, 250, 1, 8, [1.1, 0.05, 0.5], True)]


@pytest.mark.parametrize("cond,ordering_pred,n,n_p,dim,m,cp,device", _CASE4)
def test_prediction_plan_draws_against_oracle(cond, ordering_pred, n, n_p, dim, m, cp, device):
    import warnings
    G = _need_gpu()
    from oracle import r_side as R
    rng = np.random.default_rng(11)
    locs, lp = rng.random((n, dim)), rng.random((n_p, dim))
    z = np.sin(6 * locs[:, 0]) * np.cos(5 * locs[:, -1]) + 0.3 * rng.standard_normal(n)
    tau = 0.05 + 0.1 * rng.random(n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        va = G.vecchia_specify(locs, m, ordering="maxmin" if dim > 1 else None, cond_yz=cond, locs_pred=lp, ordering_pred=ordering_pred)
        pred = G.vecchia_prediction(z, va, cp, tau, return_values="meanmat")
    print(f"case 4 {cond} {dim}-D: served by the {pred['factor']['kind']} route")
    if device:
        assert pred["factor"]["kind"] == "device", "the device route must serve this plan"
    nsim, N = 6, n + n_p
    eps = rng.standard_normal((nsim, N))
    eps[nsim - 1] = 0.0; eps[nsim - 1, 0] = 1.0
    out = G.vecchia_posterior_sample(pred, eps=eps)
    assert out["y_obs"].shape == (nsim, n) and out["y_pred"].shape == (nsim, n_p) and np.array_equal(out["eps"], eps)
    Us = R.createU_sparse(_to_oracle_va(va), cp, tau)
    V = _prep_V(R.U2V_sparse(Us))
    ro, rp = _split_rows(_oracle_solve_t(V, eps), Us)
    got = np.hstack([out["y_obs"] - pred["mu_obs"], out["y_pred"] - pred["mu_pred"]])
    _check_cols(f"case 4 {cond} {dim}-D draws", got, np.hstack([ro, rp]))
    if cond == "zy":                                                  # R := B; the n dummy rows in front come back zero
        off = pred["factor"]["offset"]
        plan = G.api._plan_for(va, 0)
        assert off == n and plan.Nlocs == off + N
        Xfull = plan.solve_t(np.hstack([np.zeros((nsim, off)), eps]))
        assert np.all(Xfull[:, :off] == 0.0)


# ---- 5. state and arguments ------------------------------------------------------------------------------------------------
def test_solve_t_state_and_argument_errors():
    G = _need_gpu()
    from gpvecchia_amd import _lib as L
    rng = np.random.default_rng(7)
    n = 500
    locs = rng.random((n, 2)); z = rng.standard_normal(n)
    va = G.vecchia_specify(locs, 10, ordering="maxmin", cond_yz="SGV")
    plan = G.api._plan_for(va, 0)
    assert plan.ensure_posterior() and plan.factor_stamp() == 0
    with pytest.raises(G.GpvError) as ei:                             # structure, but no posterior evaluation yet
        plan.solve_t(np.ones(n))
    assert ei.value.status == 7                                       # GPV_ERR_STATE
    preds = G.vecchia_prediction(z, va, [1.0, 0.1, 1.5], 0.1, return_values="all")
    E = rng.standard_normal((2, n)); X = np.zeros((2, n))
    lib = L.lib()
    assert lib.gpv_plan_solve_t(plan._h, 2, L.dptr(E), n - 1, L.dptr(X), n) == 2      # GPV_ERR_BAD_ARG: lde < Nlocs
    assert lib.gpv_plan_solve_t(plan._h, 2, L.dptr(E), n, L.dptr(X), n - 1) == 2
    assert lib.gpv_plan_solve_t(plan._h, -1, L.dptr(E), n, L.dptr(X), n) == 2
    assert lib.gpv_plan_solve_t(plan._h, 2, None, n, L.dptr(X), n) == 2
    assert lib.gpv_plan_solve_t(plan._h, 0, L.dptr(E), n, L.dptr(X), n) == 0          # nothing to do
    assert lib.gpv_plan_solve_t(plan._h, 2, L.dptr(E), n, L.dptr(X), n) == 0
    # strides wider than Nlocs, and X = E in place
    Ew = np.zeros((2, n + 3)); Ew[:, :n] = E
    assert lib.gpv_plan_solve_t(plan._h, 2, L.dptr(Ew), n + 3, L.dptr(Ew), n + 3) == 0
    assert np.array_equal(Ew[:, :n], X) and np.all(Ew[:, n:] == 0.0)
    # unit draws reproduce the exact variances of the same prediction
    out = G.vecchia_posterior_sample(preds, eps=np.eye(n))
    var = np.sum((out["y_obs"] - preds["mu_obs"]) ** 2, axis=0)
    assert np.abs(var - preds["var_obs"]).max() <= RTOL * max(1.0, preds["var_obs"].max())
    with pytest.raises(ValueError):
        G.vecchia_posterior_sample(preds, eps=np.zeros((2, n + 1)))
    with pytest.raises(ValueError):
        G.vecchia_posterior_sample(dict(mu_obs=preds["mu_obs"], mu_pred=preds["mu_pred"]))
    # another evaluation of the plan: the old prediction's factor is gone
    plan.eval("matern", [2.0, 0.2, 1.5], 0.3, G.GPV_WANT_DENOM)
    with pytest.raises(RuntimeError, match="evaluated again"):
        G.vecchia_posterior_sample(preds, nsim=2, seed=1)


# ---- 6. Vecchia-Laplace ----------------------------------------------------------------------------------------------------
def test_vecchia_laplace_prediction_variances_quantiles_and_draws():
    from scipy.stats import norm
    G = _need_gpu()
    rng = np.random.default_rng(13)
    n, m = 400, 10
    locs = rng.random((n, 2))
    cp = [0.5, 0.2, 1.5]
    z = rng.poisson(np.exp(0.5 * np.sin(5 * locs[:, 0]) + 0.3 * rng.standard_normal(n))).astype(np.float64)
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="SGV")
    vl = G.calculate_posterior_VL(z, va, "poisson", covparms=cp)
    assert vl["cnvgd"]
    link = vl["data_link"]
    z_pseudo, D = np.asarray(vl["t"]) - vl["prior_mean"], np.asarray(vl["D"])
    # the default call: exactly what it returned before there were variances
    base = G.vecchia_prediction(z_pseudo, va, cp, D)
    old = G.vecchia_laplace_prediction(vl, va, cp)
    assert set(old) == set(base) | {"data_pred", "data_obs"} and "factor" not in old
    assert old["var_obs"] is None and old["var_pred"] is None
    assert np.array_equal(old["mu_obs"], base["mu_obs"] + vl["prior_mean"]) and np.array_equal(old["mu_pred"], base["mu_pred"])
    assert np.array_equal(old["data_obs"], link(old["mu_obs"])) and np.array_equal(old["data_pred"], link(old["mu_pred"]))
    # 'all': variances, the four quantile entries, the factor handle
    ref = G.vecchia_prediction(z_pseudo, va, cp, D, return_values="meanvar")
    out = G.vecchia_laplace_prediction(vl, va, cp, return_values="all")
    assert np.array_equal(out["var_obs"], ref["var_obs"]) and out["var_pred"].shape == (0,)
    assert np.array_equal(out["mu_obs"], old["mu_obs"])
    for key, p, mu, var in (("data_pred_upper_quantile", .95, out["mu_pred"], out["var_pred"]),
                            ("data_pred_lower_quantile", .05, out["mu_pred"], out["var_pred"]),
                            ("data_obs_upper_quantiles", .95, out["mu_obs"], out["var_obs"]),
                            ("data_obs_lower_quantiles", .05, out["mu_obs"], out["var_obs"])):
        want = link(norm.ppf(p, loc=mu, scale=np.sqrt(var)))
        assert out[key].shape == want.shape
        if want.size:
            assert np.abs(out[key] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), key
    assert np.all(out["data_obs_lower_quantiles"] < out["data_obs"]) and np.all(out["data_obs"] < out["data_obs_upper_quantiles"])
    draws = G.vecchia_posterior_sample(out, nsim=33, seed=3)
    assert draws["y_obs"].shape == (33, n) and draws["y_pred"].shape == (33, 0) and np.all(np.isfinite(draws["y_obs"]))
    assert np.all(link(draws["y_obs"]) > 0.0)                         # the data-scale predictive of a Poisson rate
    # 33 draws against 33 unit solves is not a test of the distribution; the spread must still be of the right order
    sd = np.sqrt(out["var_obs"])
    assert np.abs((draws["y_obs"] - out["mu_obs"]) / sd).max() < 8.0


if __name__ == "__main__":
    import torch  # noqa: F401  (first: see tests/conftest.py)
    sys.path.insert(0, ROOT)
    import gpvecchia_amd as G
    c = _case2(G)
    np.save(sys.argv[1], c["plan"].solve_t(c["E"]))
