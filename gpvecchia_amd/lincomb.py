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


def selected_variances_device(plan, nlat, offset=0):
    """The variances of the ordered latent variables [offset, offset + nlat) of the plan from ONE pass of the selected inverse
    (gpv_plan_selinv, R/vecchia_prediction.R:193-221): (vars, n_dropped).  n_dropped == 0: what exact_variances_device
    returns; otherwise the reference's var.exact = FALSE approximation."""
    v, dropped = plan.selinv(skip_front=offset)
    return v[offset:offset + nlat], dropped


def vecchia_selinv(preds):
    """Posterior variances at every observed and prediction location from one pass of the selected inverse of the posterior
    factor (the SelInv branch of vecchia_var, R/vecchia_prediction.R:193-221).  preds: the result of vecchia_prediction(...,
    return_values='meanmat' | 'all') on a device route, as for vecchia_lincomb.  Returns dict(var_obs, var_pred, n_dropped),
    locations in the caller's order.  n_dropped == 0 (fully observed 'SGV' and 'z' plans, the filled 'y' structure): the exact
    variances; n_dropped > 0: that many terms lie outside the factor's pattern and count as zero, the reference's
    var.exact = FALSE approximation."""
    fac = preds.get("factor") if isinstance(preds, dict) else None
    if fac is None:
        raise ValueError("vecchia_selinv needs the result of vecchia_prediction(..., return_values='meanmat' or 'all')")
    if fac["kind"] != "device":
        raise ValueError("vecchia_selinv: this prediction was made on the host route, which has no selected inverse; "
                         "its var_obs / var_pred are exact")
    plan = _check_stamp(fac)
    nlat, off = int(fac["ord"].size), fac["offset"]
    if off + nlat != plan.Nlocs:
        raise ValueError("preds does not match the plan of this prediction")
    var_ord, dropped = selected_variances_device(plan, nlat, off)
    from .api import split_mean
    var_obs, var_pred = split_mean(var_ord, dict(ord=fac["ord"], obs=fac["obs"]))
    return dict(var_obs=var_obs, var_pred=var_pred, n_dropped=dropped)


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


_LINKS = {None: 0, "identity": 0, "exp": 1, "logistic": 2}


def _link_fun(code):
    if code == 1:
        return np.exp
    if code == 2:
        return lambda y: 1.0 / (1.0 + np.exp(-y))
    return lambda y: y


def _join_ord(a_obs, a_pred, ord_, obs):
    """The inverse of api.split_mean: values at the observed and the prediction locations in the caller's order -> one vector
    in the ordered latent layout."""
    orig_order = np.argsort(np.asarray(ord_), kind="stable")
    obs_orig = np.asarray(obs, dtype=bool)[orig_order]
    a_obs, a_pred = np.asarray(a_obs), np.asarray(a_pred)
    if a_obs.shape != (int(obs_orig.sum()),) or a_pred.shape != (int((~obs_orig).sum()),):
        raise ValueError("one entry per observed location and one per prediction location is needed")
    caller = np.empty(obs_orig.size, dtype=np.result_type(a_obs, a_pred))
    caller[obs_orig] = a_obs
    caller[~obs_orig] = a_pred
    out = np.empty_like(caller)
    out[orig_order] = caller
    return out


def draws_normals_host(seed, k0, nk, col0, ncols):
    """gpv_draws_normals_host: the generator's standard normals of the ordered locations [k0, k0 + nk) and the draws
    [col0, col0 + ncols), computed on the host: (ncols, nk).  No device is needed.  Exported from the package: a caller who wants
    the draws behind a vecchia_posterior_summary passes these rows (k0 = the plan's rows in front, 0 or n for 'zy') as eps to
    vecchia_posterior_sample."""
    from . import _lib as L
    E = np.empty((int(ncols), int(nk)))
    L.check(L.lib().gpv_draws_normals_host(int(seed), int(k0), int(nk), int(col0), int(ncols), L.dptr(E), int(nk)),
            "gpv_draws_normals_host")
    return E


def _host_summary(lu, k0, nzero, mu_ord, nsim, seed, code, thr, mask):
    """What gpv_plan_draws_summary computes, on the host factor, with the same generator: chunks of draws through
    _host_solve_t, the same sums.  mu_ord / mask cover the nlat latent variables and the nzero zero-nugget observations behind
    them (those are their data in every draw)."""
    g = _link_fun(code)
    nlat = mu_ord.size - nzero
    gmu = g(mu_ord)
    S1, S2 = np.zeros(mu_ord.size), np.zeros(mu_ord.size)
    cnt = np.zeros((thr.size, mu_ord.size))
    draw_max, draw_mean = np.empty(nsim), np.empty(nsim)
    for b in range(0, nsim, _HOST_CHUNK):
        nb = min(_HOST_CHUNK, nsim - b)
        E = draws_normals_host(seed, k0, nlat, b, nb)
        X = _host_solve_t(lu, E[:, ::-1].T)[::-1].T
        if nzero:
            X = np.hstack([X, np.zeros((nb, nzero))])
        Y = mu_ord[None, :] + X
        GY = g(Y)
        D = GY - gmu[None, :]
        S1 += D.sum(axis=0)
        S2 += (D * D).sum(axis=0)
        for t in range(thr.size):
            cnt[t] += (Y > thr[t]).sum(axis=0)
        draw_max[b:b + nb] = GY[:, mask].max(axis=1)
        draw_mean[b:b + nb] = GY[:, mask].mean(axis=1)
    N = float(nsim)
    return dict(mean=gmu + S1 / N, var=np.maximum((S2 - S1 * S1 / N) / (N - 1.0), 0.0), exceed=cnt / N,
                draw_max=draw_max, draw_mean=draw_mean)


def vecchia_posterior_summary(preds, nsim, seed=0, thresholds=None, link=None, mask_obs=None, mask_pred=None):
    """Monte-Carlo summaries of nsim draws from the Vecchia posterior (the draws of vecchia_posterior_sample, never brought to
    the host): pointwise mean and variance, exceedance probabilities, and for every draw the maximum and the mean over a region.
    preds: as for vecchia_posterior_sample.  The standard normals come from the library's counter-based generator (Philox4x32-10,
    a function of seed, ordered location and draw alone), on the device routes made on the device (gpv_plan_draws_summary: 32
    draws per sweep, sums folded on the device); the host route computes the same quantities from the same generator.

    link: None / 'identity', 'exp' or 'logistic': mean, var, draw_max and draw_mean are those of link(y), e.g. the data scale of
    a vecchia_laplace_prediction result.  thresholds (at most 8) are on the LATENT scale: exceed[t] = share of draws with
    y > thresholds[t].  mask_obs / mask_pred: booleans per observed / prediction location (caller's order) selecting the region
    of draw_max / draw_mean; both None: every location; one None: no location of that group.

    Returns dict(mean_obs, mean_pred, var_obs, var_pred, exceed_obs (len(thresholds) x n), exceed_pred, draw_max, draw_mean
    (nsim each)).  Zero-nugget observations (host route) have variance 0 and their data as mean."""
    fac = preds.get("factor") if isinstance(preds, dict) else None
    if fac is None:
        raise ValueError("vecchia_posterior_summary needs the result of vecchia_prediction(..., return_values='meanmat' or 'all')")
    if link not in _LINKS:
        raise ValueError("link must be None, 'identity', 'exp' or 'logistic'")
    code, nsim = _LINKS[link], int(nsim)
    if nsim < 2:
        raise ValueError("nsim must be at least 2")
    thr = np.asarray([] if thresholds is None else thresholds, dtype=np.float64).reshape(-1)
    if thr.size > 8:
        raise ValueError("at most 8 thresholds")
    if fac["kind"] == "device":
        plan = _check_stamp(fac)
        ord_, obs, off = fac["ord"], fac["obs"], fac["offset"]
        if off + int(ord_.size) != plan.Nlocs:
            raise ValueError("preds does not match the plan of this prediction")
    else:
        U_obj, lu = fac["U_obj"], fac["lu"]
        ord_, obs = np.asarray(U_obj["ord"]), np.asarray(U_obj["obs"], dtype=bool)
        nzero = len(U_obj["zero_nugg"]["inds_z"]) if U_obj["zero_nugg"] else 0
        off = int(np.sum(obs)) if U_obj.get("cond_yz") == "zy" else 0      # the device layout's dummy rows: the same normals
    mu_ord = _join_ord(np.asarray(preds["mu_obs"], dtype=np.float64), np.asarray(preds["mu_pred"], dtype=np.float64), ord_, obs)
    n_obs = int(np.sum(obs))
    if mask_obs is None and mask_pred is None:
        mask = np.ones(mu_ord.size, dtype=bool)
    else:
        mask = _join_ord(np.zeros(n_obs, dtype=bool) if mask_obs is None else np.asarray(mask_obs, dtype=bool),
                         np.zeros(mu_ord.size - n_obs, dtype=bool) if mask_pred is None else np.asarray(mask_pred, dtype=bool),
                         ord_, obs)
        if not mask.any():
            raise ValueError("the masks select no location")
    if fac["kind"] == "device":
        pad = lambda a, fill: np.concatenate([np.full(off, fill, dtype=a.dtype), a]) if off else a
        res = plan.draws_summary(nsim, seed=seed, skip_front=off, mu_ord=pad(mu_ord, 0.0), link=code, thresholds=thr,
                                 mask=None if (mask_obs is None and mask_pred is None) else pad(mask, False))
        res = dict(mean=res["mean"][off:], var=res["var"][off:], exceed=res["exceed"][:, off:], draw_max=res["draw_max"],
                   draw_mean=res["draw_mean"])
    else:
        res = _host_summary(lu, off, nzero, mu_ord, nsim, seed, code, thr, mask)
    from .api import split_mean
    so = dict(ord=ord_, obs=obs)
    out = dict(draw_max=res["draw_max"], draw_mean=res["draw_mean"])
    out["mean_obs"], out["mean_pred"] = split_mean(res["mean"], so)
    out["var_obs"], out["var_pred"] = split_mean(res["var"], so)
    ex = [split_mean(res["exceed"][t], so) for t in range(thr.size)]
    out["exceed_obs"] = np.array([e[0] for e in ex]).reshape(thr.size, n_obs)
    out["exceed_pred"] = np.array([e[1] for e in ex]).reshape(thr.size, mu_ord.size - n_obs)
    return out
