"""Linear combinations of the posterior field and exact posterior variances — the mirror of vecchia_lincomb
(R/vecchia_prediction.R:164-178) and of the var.exact path of vecchia_var (:203-247).

With V.ord the reversed factor of W (V V^T = rev(W)), vecchia_lincomb's `temp = solve(V.ord, t(H[, rev(ord)]))` is, in this
repository's unreversed layout, R x = h with W = R R^T, and `colSums(temp^2)` is |x|^2 = h' W^-1 h.  On the device routes
that is gpv_plan_lincomb (gpv_lincomb.hip: one level-scheduled triangular solve for 32 rows of H at a time, on the factor
the prediction's evaluation left in the plan); on the host route the same quantity through the factor object of api.U2V.
Unit-vector rows give diag(W^-1): the exact posterior variances, which for an exact fill-closed factor is also what the
reference's SelInv returns.

vecchia_posterior_sample reads the same factor the other way round: for e ~ N(0, I), x = R^-T e has covariance W^-1, so
mu + x is a draw from the Vecchia posterior of the latent field at every observed and prediction location (conditional
simulation).  Device routes: gpv_plan_solve_t (32 draws per sweep); host route: rev(x) = V^-T rev(e) with the factor of api.U2V.
"""
from __future__ import annotations

import numpy as np

_HOST_CHUNK = 256          # right-hand sides per host solve


def _device_factor(plan, ord_, obs, offset=0):
    """The opaque `factor` entry of a device-route prediction: the plan, the stamp of the evaluation whose factor it holds,
    ord / obs of the latent variables (caller's location -> ordered position) and the number of rows the plan carries in
    front of them (the n dummy rows of cond.yz = 'zy')."""
    return dict(kind="device", plan=plan, stamp=plan.factor_stamp(), ord=np.asarray(ord_), obs=np.asarray(obs, dtype=bool),
                offset=int(offset))


def _host_factor(U_obj, lu):
    return dict(kind="host", U_obj=U_obj, lu=lu)


def _check_stamp(fac):
    plan = fac["plan"]
    if fac["stamp"] == 0 or plan.factor_stamp() != fac["stamp"]:
        raise RuntimeError("vecchia_lincomb: the plan has been evaluated again since this prediction was made; its factor "
                           "is no longer the prediction's.  Call vecchia_prediction again.")
    return plan


def _host_quadform(lu, Hrev, cov_mat):
    """rows h of Hrev (dense or sparse, reversed ordered layout): h' (V V^T)^-1 h, or the whole H (V V^T)^-1 H^T."""
    import scipy.sparse as sp
    Hrev = sp.csr_matrix(Hrev)
    nrows = Hrev.shape[0]
    if cov_mat:
        S = lu.solve(np.asarray(Hrev.T.todense(), dtype=np.float64))
        return np.asarray(Hrev @ S)
    out = np.empty(nrows)
    for b in range(0, nrows, _HOST_CHUNK):
        blk = Hrev[b:b + _HOST_CHUNK]
        D = np.asarray(blk.T.todense(), dtype=np.float64)
        out[b:b + _HOST_CHUNK] = np.einsum("ij,ij->j", D, lu.solve(D))
    return out


def vecchia_lincomb(H, preds, cov_mat=False):
    """R/vecchia_prediction.R:164-178.  H: sparse or dense matrix whose columns are the locations in the caller's order
    (observed locations first, then the prediction locations); preds: the result of vecchia_prediction(...,
    return_values='meanmat' | 'all').  Returns the variances of H y given the data, or with cov_mat the covariance matrix
    (device routes: for at most gpv_lincomb_batch() = 32 rows)."""
    import scipy.sparse as sp
    fac = preds.get("factor") if isinstance(preds, dict) else None
    if fac is None:
        raise ValueError("vecchia_lincomb needs the result of vecchia_prediction(..., return_values='meanmat' or 'all')")
    H = H.tocsc() if sp.issparse(H) else sp.csc_matrix(np.atleast_2d(np.asarray(H, dtype=np.float64)))
    if fac["kind"] == "device":
        plan = _check_stamp(fac)
        ord_ = fac["ord"]
        if H.shape[1] != ord_.size:
            raise ValueError(f"H must have {ord_.size} columns (one per observed and prediction location)")
        # H[, rev(ord)] in the unreversed layout: ordered position p holds the caller's location ord[p]
        Hs = H[:, ord_ - 1]
        if fac["offset"]:
            Hs = sp.hstack([sp.csc_matrix((H.shape[0], fac["offset"])), Hs])
        if Hs.shape[1] != plan.Nlocs:
            raise ValueError("H does not match the plan of this prediction")
        return plan.lincomb(Hs.tocsr(), cov_mat=cov_mat)
    U_obj, lu = fac["U_obj"], fac["lu"]
    ord_ = np.asarray(U_obj["ord"])
    if U_obj["zero_nugg"]:                                                # :166-168
        keep = ord_[:ord_.size - len(U_obj["zero_nugg"]["inds_U"])]
        ord_ = np.argsort(np.argsort(keep, kind="stable"), kind="stable") + 1
    if H.shape[1] < ord_.size:
        raise ValueError(f"H must have at least {ord_.size} columns")
    Hrev = H[:, (ord_ - 1)[::-1]]                                         # :169
    return _host_quadform(lu, Hrev, cov_mat)


def exact_variances_device(plan, nlat, offset=0):
    """diag(W^-1) over the ordered latent variables [offset, offset + nlat) of the plan: unit-vector rows, batched in
    descending ordered index (a batch then touches nothing above its largest index)."""
    import scipy.sparse as sp
    idx = np.arange(offset + nlat - 1, offset - 1, -1)
    Hu = sp.csr_matrix((np.ones(nlat), idx, np.arange(nlat + 1)), shape=(nlat, plan.Nlocs))
    v = plan.lincomb(Hu)
    out = np.empty(nlat)
    out[idx - offset] = v
    return out


def exact_variances_host(lu, nlat):
    """diag(W^-1) in ordered layout from the host factor of the reversed matrix."""
    out = np.empty(nlat)
    for b in range(0, nlat, _HOST_CHUNK):
        e = min(nlat, b + _HOST_CHUNK)
        D = np.zeros((nlat, e - b))
        D[np.arange(b, e), np.arange(e - b)] = 1.0
        out[b:e] = np.einsum("ij,ij->j", D, lu.solve(D))
    return out[::-1]


def host_variances(U_obj, lu):
    """vecchia_var (R/vecchia_prediction.R:203-221) with exact variances on the host factor: (vars.obs, vars.pred) in the
    caller's order, zeros for the zero-nugget observations (:210-212)."""
    from .api import split_mean
    nlat = int(np.sum(U_obj["latent"]))
    var_ord = exact_variances_host(lu, nlat)
    if U_obj["zero_nugg"]:
        var_ord = np.concatenate([var_ord, np.zeros(len(U_obj["zero_nugg"]["inds_z"]))])
    return split_mean(var_ord, U_obj)


def _host_solve_t(lu, Erev):
    """V^-T e for the columns e of Erev (reversed ordered layout), V V^T = rev(W): the mirror of _host_quadform.  SuperLU
    object of api.U2V: rev(W) = L D L^T (natural order, no pivoting), V = L sqrt(D), so V^-T e = L^-T (e / sqrt(diag U))."""
    import scipy.sparse.linalg as spla
    Erev = np.asarray(Erev, dtype=np.float64)
    V = getattr(lu, "V", None)
    if V is not None:                                                     # api._TriFactor
        return spla.spsolve_triangular(V.T.tocsr(), Erev, lower=False)
    nW = lu.shape[0]
    if not (np.array_equal(lu.perm_r, np.arange(nW)) and np.array_equal(lu.perm_c, np.arange(nW))):
        raise RuntimeError("vecchia_posterior_sample: the sparse factorisation pivoted (matrix not positive definite?)")
    d = lu.U.diagonal()
    return spla.spsolve_triangular(lu.L.T.tocsr(), Erev / np.sqrt(d)[:, None], lower=False)


def _split_rows(X_ord, ord_, obs):
    """api.split_mean for every row of X_ord (nsim x ordered latent variables): (nsim x n, nsim x n_p) in the caller's order."""
    orig_order = np.argsort(np.asarray(ord_), kind="stable")
    X = np.asarray(X_ord)[:, orig_order]
    obs_orig = np.asarray(obs, dtype=bool)[orig_order]
    return X[:, obs_orig], X[:, ~obs_orig]


def vecchia_posterior_sample(preds, nsim=1, seed=None, eps=None):
    """Draws from the Vecchia posterior of the latent field given the data (conditional simulation): mu + R^-T eps with
    W = R R^T the posterior precision of vecchia_prediction (R/vecchia_prediction.R:62-126).  preds: the result of
    vecchia_prediction(..., return_values='meanmat' | 'all') (or of vecchia_laplace_prediction with those values: the draws
    are then of the latent field, and vl_posterior['data_link'] of them is the data-scale predictive).  eps: (nsim, number of
    latent variables) standard normals in the ORDERED latent layout; absent, np.random.default_rng(seed).standard_normal.
    Returns dict(y_obs (nsim x n), y_pred (nsim x n_p), eps), locations in the caller's order; zero-nugget observations
    (host route) are their data in every draw (variance 0, :129-132, :210-212)."""
    fac = preds.get("factor") if isinstance(preds, dict) else None
    if fac is None:
        raise ValueError("vecchia_posterior_sample needs the result of vecchia_prediction(..., return_values='meanmat' or 'all')")
    if fac["kind"] == "device":
        plan = _check_stamp(fac)
        nlat, nzero = int(fac["ord"].size), 0
        if fac["offset"] + nlat != plan.Nlocs:
            raise ValueError("preds does not match the plan of this prediction")
    else:
        U_obj, lu = fac["U_obj"], fac["lu"]
        nlat = int(np.sum(U_obj["latent"]))
        nzero = len(U_obj["zero_nugg"]["inds_z"]) if U_obj["zero_nugg"] else 0
    if eps is None:
        nsim = int(nsim)
        if nsim < 0:
            raise ValueError("nsim must not be negative")
        eps = np.random.default_rng(seed).standard_normal((nsim, nlat))
    else:
        eps = np.asarray(eps, dtype=np.float64)
        if eps.ndim != 2 or eps.shape[1] != nlat:
            raise ValueError(f"eps must be (nsim, {nlat}): one column per latent variable, ordered layout")
        nsim = int(eps.shape[0])
    if fac["kind"] == "device":
        off = fac["offset"]
        # (cond.yz = 'zy': the n dummy rows in front carry zeros, as the columns of H do in vecchia_lincomb)
        E = np.hstack([np.zeros((nsim, off)), eps]) if off else eps
        X = plan.solve_t(E)[:, off:] if nsim else np.zeros((0, nlat))
        x_obs, x_pred = _split_rows(X, fac["ord"], fac["obs"])
    else:
        X = np.empty((nsim, nlat))
        for b in range(0, nsim, _HOST_CHUNK):
            X[b:b + _HOST_CHUNK] = _host_solve_t(lu, eps[b:b + _HOST_CHUNK, ::-1].T)[::-1].T
        if nzero:
            X = np.hstack([X, np.zeros((nsim, nzero))])
        x_obs, x_pred = _split_rows(X, U_obj["ord"], U_obj["obs"])
    return dict(y_obs=np.asarray(preds["mu_obs"])[None, :] + x_obs, y_pred=np.asarray(preds["mu_pred"])[None, :] + x_pred, eps=eps)
