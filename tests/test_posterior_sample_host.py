"""CPU tests of gpv_plan_solve_t's argument checks (no device is touched before them) and of the host route of
vecchia_posterior_sample: with eps = I the draws' outer products sum to W^-1 = inv(U_y U_y^T), against dense numpy."""
import ctypes as C

import numpy as np
import pytest


def test_solve_t_symbol_and_argument_checks():
    from gpvecchia_amd import _lib as L
    import gpvecchia_amd as G
    lib = L.lib()
    assert "gpv_plan_solve_t" in L.EXPORTS and hasattr(lib, "gpv_plan_solve_t")
    assert callable(G.vecchia_posterior_sample) and hasattr(G.Plan, "solve_t")
    e = np.ones(4); x = np.zeros(4)
    assert lib.gpv_plan_solve_t(None, 1, L.dptr(e), 4, L.dptr(x), 4) == 2          # GPV_ERR_BAD_ARG: no plan
    assert lib.gpv_plan_solve_t(None, 0, L.dptr(e), 4, L.dptr(x), 4) == 2          # (even with nothing to solve)
    assert lib.gpv_plan_solve_t(C.c_void_p(0), -1, L.dptr(e), 4, L.dptr(x), 4) == 2
    assert lib.gpv_plan_solve_t(None, 1, None, 4, None, 4) == 2


def _host_case(n_p, zero_nugget):
    import scipy.sparse as sp
    from gpvecchia_amd import api as A
    from oracle import r_side as R
    rng = np.random.default_rng(17 + n_p)
    n, m = 300, 8
    locs = rng.random((n, 2))
    lp = rng.random((n_p, 2)) if n_p else None
    tau = 0.05 + 0.1 * rng.random(n)
    if zero_nugget:
        tau[[5, 77]] = 0.0
    vb = R.vecchia_specify(locs, m, ordering="maxmin", cond_yz="SGV", locs_pred=lp)
    Uo = R.createU(vb, [1.0, 0.1, 1.5], tau)
    U_obj = dict(Uo)
    U_obj["U"] = sp.csc_matrix(Uo["U"])
    lu = A.U2V(U_obj)
    Uy = Uo["U"][np.asarray(Uo["latent"], dtype=bool), :]
    Winv = np.linalg.inv(Uy @ Uy.T)                                   # ordered layout, one row per (remaining) latent variable
    return U_obj, lu, Winv, n, tau


@pytest.mark.parametrize("n_p,zero_nugget", [(0, False), (40, False), (40, True)])
def test_host_route_draws_have_the_posterior_covariance(n_p, zero_nugget):
    import gpvecchia_amd as G
    from gpvecchia_amd import lincomb as LC
    U_obj, lu, Winv, n, tau = _host_case(n_p, zero_nugget)
    nlat = Winv.shape[0]
    nzero = len(U_obj["zero_nugg"]["inds_z"]) if U_obj["zero_nugg"] else 0
    assert nzero == (2 if zero_nugget else 0) and nlat == n + n_p - nzero
    rng = np.random.default_rng(5)
    mu_obs, mu_pred = rng.standard_normal(n), rng.standard_normal(n_p)
    preds = dict(factor=LC._host_factor(U_obj, lu), mu_obs=mu_obs, mu_pred=mu_pred)
    out = G.vecchia_posterior_sample(preds, eps=np.eye(nlat))
    assert out["y_obs"].shape == (nlat, n) and out["y_pred"].shape == (nlat, n_p) and out["eps"].shape == (nlat, nlat)
    X = np.hstack([out["y_obs"] - mu_obs, out["y_pred"] - mu_pred])   # row i: R^-T e_i in the caller's order
    full = np.zeros((nlat + nzero, nlat + nzero))
    full[:nlat, :nlat] = Winv                                         # variance 0 for the zero-nugget observations
    orig = np.argsort(U_obj["ord"], kind="stable")
    obs_orig = np.asarray(U_obj["obs"], dtype=bool)[orig]
    perm = np.concatenate([orig[obs_orig], orig[~obs_orig]])
    ref = full[np.ix_(perm, perm)]
    np.testing.assert_allclose(X.T @ X, ref, rtol=0, atol=1e-9)
    if zero_nugget:
        assert np.array_equal(out["y_obs"][:, tau == 0.0], np.broadcast_to(mu_obs[tau == 0.0], (nlat, 2)))
    # seed reproduces, another seed does not; nsim gives the shape
    a = G.vecchia_posterior_sample(preds, nsim=3, seed=11)
    b = G.vecchia_posterior_sample(preds, nsim=3, seed=11)
    c = G.vecchia_posterior_sample(preds, nsim=3, seed=12)
    assert a["y_obs"].shape == (3, n) and a["y_pred"].shape == (3, n_p) and a["eps"].shape == (3, nlat)
    assert np.array_equal(a["y_obs"], b["y_obs"]) and np.array_equal(a["y_pred"], b["y_pred"]) and np.array_equal(a["eps"], b["eps"])
    assert not np.array_equal(a["y_obs"], c["y_obs"])
    # a given eps is used as it is: the draw is linear in it
    two = G.vecchia_posterior_sample(preds, eps=2.0 * a["eps"])
    np.testing.assert_allclose(two["y_obs"] - mu_obs, 2.0 * (a["y_obs"] - mu_obs), rtol=0, atol=1e-12)
    for bad in (np.zeros((2, nlat + 1)), np.zeros(nlat), np.zeros((2, nlat - 1))):
        with pytest.raises(ValueError):
            G.vecchia_posterior_sample(preds, eps=bad)


def test_host_route_trifactor_matches_the_dense_solve():
    """The `V` branch of the host solve (api._TriFactor: 'zy', ic0 and the obs-pred shortcut): V^-T e against numpy."""
    import scipy.sparse as sp
    from gpvecchia_amd import api as A
    from gpvecchia_amd import lincomb as LC
    rng = np.random.default_rng(2)
    V = np.tril(rng.standard_normal((30, 30))) * 0.2 + np.diag(1.0 + rng.random(30))
    E = rng.standard_normal((30, 5))
    got = LC._host_solve_t(A._TriFactor(sp.csr_matrix(V)), E)
    np.testing.assert_allclose(got, np.linalg.solve(V.T, E), rtol=0, atol=1e-12)


def test_posterior_sample_needs_a_factor():
    import gpvecchia_amd as G
    with pytest.raises(ValueError):
        G.vecchia_posterior_sample(dict(mu_obs=np.zeros(3), mu_pred=np.zeros(0), var_obs=None))
