"""CPU tests of vecchia_lincomb and the exact posterior variances: the C ABI's argument checks (no device is touched
before them) and the host-route algebra (R/vecchia_prediction.R:164-178, 203-247) against dense numpy."""
import ctypes as C

import numpy as np
import pytest


def test_lincomb_symbols_and_argument_checks():
    from gpvecchia_amd import _lib as L
    lib = L.lib()
    assert "gpv_plan_lincomb" in L.EXPORTS and "gpv_lincomb_batch" in L.EXPORTS
    assert lib.gpv_lincomb_batch() in (16, 32)
    hptr = np.array([0, 1], dtype=np.int64); hidx = np.zeros(1, dtype=np.int32); hval = np.ones(1); out = np.zeros(1)
    st = lib.gpv_plan_lincomb(None, 1, hptr.ctypes.data_as(C.POINTER(C.c_int64)), hidx.ctypes.data_as(C.POINTER(C.c_int32)),
                              L.dptr(hval), L.dptr(out), None)
    assert st == 2                                                    # GPV_ERR_BAD_ARG
    stamp = C.c_int64(7)
    assert lib.gpv_plan_factor_stamp(None, C.byref(stamp)) == 2


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
def test_host_route_variances_and_lincomb_match_dense_algebra(n_p, zero_nugget):
    import scipy.sparse as sp
    import gpvecchia_amd as G
    from gpvecchia_amd import lincomb as LC
    U_obj, lu, Winv, n, tau = _host_case(n_p, zero_nugget)
    nlat = Winv.shape[0]
    nzero = len(U_obj["zero_nugg"]["inds_z"]) if U_obj["zero_nugg"] else 0
    assert nzero == (2 if zero_nugget else 0) and nlat == n + n_p - nzero
    # variances: diag(W^-1) in ordered layout, zeros appended for the zero-nugget observations, back to the caller's order
    var_obs, var_pred = LC.host_variances(U_obj, lu)
    full = np.concatenate([np.diag(Winv), np.zeros(nzero)])
    orig = np.argsort(U_obj["ord"], kind="stable")
    ref = full[orig]
    obs_orig = np.asarray(U_obj["obs"], dtype=bool)[orig]
    assert var_obs.shape == (n,) and var_pred.shape == (n_p,)
    np.testing.assert_allclose(var_obs, ref[obs_orig], rtol=0, atol=1e-10)
    np.testing.assert_allclose(var_pred, ref[~obs_orig], rtol=0, atol=1e-10)
    if zero_nugget:
        assert np.array_equal(var_obs[tau == 0.0], [0.0, 0.0]) and np.all(var_obs[tau > 0.0] > 0.0)
    else:
        assert np.all(var_obs > 0.0)
    # linear combinations: column j of H is location j of the caller's order; with zero nuggets ord is re-ranked (:166-168)
    ord_ = np.asarray(U_obj["ord"])
    if nzero:
        ord_ = np.argsort(np.argsort(ord_[:ord_.size - nzero], kind="stable"), kind="stable") + 1
    rng = np.random.default_rng(3)
    H = sp.random(12, nlat, density=0.05, random_state=5, format="csr") + sp.csr_matrix(
        (np.ones(3), ([0, 1, 2], [0, nlat - 1, nlat // 2])), shape=(12, nlat))
    H = sp.vstack([H, sp.csr_matrix(np.full((1, nlat), 1.0 / nlat))]).tocsr()   # a dense "regional average"
    Hord = H.toarray()[:, ord_ - 1]                                   # ordered position p holds location ord[p]
    cov_ref = Hord @ Winv @ Hord.T
    preds = dict(factor=LC._host_factor(U_obj, lu))
    v = G.vecchia_lincomb(H, preds)
    cv = G.vecchia_lincomb(H, preds, cov_mat=True)
    np.testing.assert_allclose(v, np.diag(cov_ref), rtol=0, atol=1e-10)
    np.testing.assert_allclose(cv, cov_ref, rtol=0, atol=1e-10)
    np.testing.assert_allclose(G.vecchia_lincomb(H.toarray(), preds), v, rtol=0, atol=1e-13)   # dense H: the same


def test_lincomb_needs_a_factor():
    import gpvecchia_amd as G
    with pytest.raises(ValueError):
        G.vecchia_lincomb(np.eye(3), dict(mu_obs=np.zeros(3), var_obs=None))
