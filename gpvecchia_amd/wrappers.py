"""Parameter estimation driver — mirror of vecchia_estimate (R/vecchia_wrappers.R:28-106).

The driver is WHY the engine's metric is "likelihood evaluations per second": the plan is specified once
(:55) and vecchia_likelihood is called once per Nelder-Mead step (:72-78, up to maxit = 300 evaluations) with
continuously varying smoothness, i.e. through the general-nu Bessel branch on the device.

stats::optim(method = "Nelder-Mead") is R-core code outside the GPvecchia tree: its simplex search is Nash's
(Compact Numerical Methods, 2nd ed., 1990, algorithm 19) with alpha = 1, beta = 0.5, gamma = 2, started from the
axis-parallel simplex of step 0.1 max|x_i|, stopped when f_high <= f_low + reltol (|f_initial| + reltol) or after
`maxit` function evaluations.  `_nelder_mead_nash` below follows that published algorithm and those control values
(reltol, maxit, parscale as used at :83-93).  Pinned by the known answer printed in R's own documentation of optim
(example `optim(c(-1.2, 1), fr)` on the Rosenbrock function: par 1.000260 1.000506, value 8.825241e-08, 195 function
evaluations), reproduced digit for digit in tests/test_cabi_and_host.py.
"""
from __future__ import annotations

import numpy as np

from . import api as A

_BIG = 1.0e35          # value substituted for a non-finite objective (as optim does)


def _nelder_mead_nash(fn, x0, reltol, maxit, abstol=-np.inf, alpha=1.0, beta=0.5, gamma=2.0):
    """Nelder-Mead polytope search after Nash (1990).  Returns (x, f, n_evals, code): code 0 converged, 1 evaluation
    limit reached, 10 degenerate simplex (the codes optim reports)."""
    x0 = np.asarray(x0, dtype=np.float64)
    n = x0.size
    f0 = fn(x0)
    if not np.isfinite(f0):
        raise RuntimeError("function cannot be evaluated at initial parameters")
    count = 1
    convtol = reltol * (abs(f0) + reltol)
    V = np.tile(x0, (n + 1, 1))                      # vertices
    F = np.full(n + 1, np.nan)
    F[0] = f0
    step = max(0.1 * np.max(np.abs(x0)), 0.0) or 0.1
    size = 0.0
    for j in range(1, n + 1):
        t = step
        while V[j, j - 1] == x0[j - 1]:
            V[j, j - 1] = x0[j - 1] + t
            t *= 10
        size += t
    oldsize = size
    lo = 0
    recompute = True
    code = 0
    while True:
        if recompute:
            for j in range(n + 1):
                if j != lo:
                    f = fn(V[j])
                    F[j] = f if np.isfinite(f) else _BIG
                    count += 1
            recompute = False
        # nmmin's scan: L stays where it is unless a vertex is STRICTLY lower, H starts at L and moves to every strictly
        # higher vertex in index order (ties keep the earlier choice)
        fl = fh = F[lo]
        hi = lo
        for j in range(n + 1):
            if j != lo:
                if F[j] < fl:
                    lo, fl = j, F[j]
                if F[j] > fh:
                    hi, fh = j, F[j]
        if fh <= fl + convtol or fl <= abstol:
            break
        cen = (V.sum(axis=0) - V[hi]) / n
        xr = (1.0 + alpha) * cen - alpha * V[hi]
        fr = fn(xr)
        fr = fr if np.isfinite(fr) else _BIG
        count += 1
        if fr < fl:                                  # try an extension
            xe = gamma * xr + (1.0 - gamma) * cen
            fe = fn(xe)
            fe = fe if np.isfinite(fe) else _BIG
            count += 1
            if fe < fr:
                V[hi], F[hi] = xe, fe
            else:
                V[hi], F[hi] = xr, fr
        else:
            if fr < fh:                              # keep the reflection, then reduce on the low side
                V[hi], F[hi] = xr, fr
            xc = (1.0 - beta) * V[hi] + beta * cen
            fc = fn(xc)
            fc = fc if np.isfinite(fc) else _BIG
            count += 1
            if fc < F[hi]:
                V[hi], F[hi] = xc, fc
            elif fr >= fh:                           # shrink towards the best vertex
                recompute = True
                size = 0.0
                for j in range(n + 1):
                    if j != lo:
                        V[j] = beta * (V[j] - V[lo]) + V[lo]
                        size += np.abs(V[j] - V[lo]).sum()
                if size < oldsize:
                    oldsize = size
                else:
                    code = 10
                    break
        if count > maxit:
            break
    if count > maxit:                                # (like nmmin, the vertex returned is L of the LAST scan, even when the
        code = 1                                     #  evaluation limit stopped the search right after a lower one was stored)
    return V[lo].copy(), float(F[lo]), count, code


def _fisher_scoring(fn, x0, reltol, maxit, max_step=1.0, max_halvings=10):
    """Fisher scoring: maximises a log-likelihood from fn(x) -> (value, gradient, information), the information being the
    expected one (positive definite where the model is identified).  The step s solves information s = gradient and is scaled
    to norm max_step when longer; it is halved while the value at x + s is not finite or does not increase, and after
    max_halvings halvings the search gives up.  It stops when gradient's <= reltol |value|: twice the gain the quadratic model
    still promises.  Every call of fn counts.  Returns (x, value, gradient, information, n_evals, code): code 0 converged,
    1 evaluation limit reached, step not found or information not positive definite."""
    x = np.array(x0, dtype=np.float64)
    f, g, info = fn(x)
    if not np.isfinite(f):
        raise RuntimeError("function cannot be evaluated at initial parameters")
    count = 1
    while True:
        try:
            s = np.linalg.solve(info, g)
        except np.linalg.LinAlgError:
            return x, float(f), g, info, count, 1
        gain = float(g @ s)
        if not np.isfinite(gain) or gain < 0.0:
            return x, float(f), g, info, count, 1
        if gain <= reltol * abs(f):
            return x, float(f), g, info, count, 0
        norm = float(np.sqrt(s @ s))
        if norm > max_step:
            s = s * (max_step / norm)
        for _ in range(max_halvings + 1):
            if count >= maxit:
                return x, float(f), g, info, count, 1
            xn = x + s
            fn_, gn, infon = fn(xn)
            count += 1
            if np.isfinite(fn_) and fn_ > f:
                break
            s = 0.5 * s
        else:
            return x, float(f), g, info, count, 1
        x, f, g, info = xn, fn_, gn, infon


def _nu_slot_checked(g_nu, ll, nu):
    """A free smoothness whose derivative is NaN although the likelihood is finite: the trial point sits exactly on a closed form."""
    if np.isfinite(ll) and np.isnan(g_nu):
        raise ValueError(f"the Matern covariance is not differentiable in the smoothness at exactly {float(nu)!r} (the closed "
                         "forms 0.5, 1.5, 2.5 scale the distance differently): choose a different starting value for the "
                         "smoothness in theta_ini, e.g. one a little off that value")


def profile_negloglik_grad(lg, data, X, va, covmodel="matern", smoothness=None):
    """Negative profile log-likelihood of the GLS trend and its gradient in the log-parameters lg (variance, range[, further
    covparms], nugget; for 'matern' the smoothness is the fixed `smoothness`).  The value and beta_hat(theta) come from
    vecchia_profile_likelihood; the gradient is vecchia_likelihood_grad on the residual data - X beta_hat(theta): at beta_hat
    the derivative of the likelihood in beta vanishes, so the partial gradient in theta IS the gradient of the profile (the
    envelope theorem).  Returns (value, gradient, profile dict)."""
    th = np.exp(np.asarray(lg, dtype=np.float64))
    matern = covmodel in ("matern", "matern_scaledim")
    nu_at = len(th) - 1 if covmodel == "matern_scaledim" else 2      # ('matern_scaledim': variance, the ranges, smoothness)
    cp = np.concatenate([th[:nu_at], [float(smoothness)], th[nu_at:-1]]) if matern else th[:-1]
    prof = A.vecchia_profile_likelihood(data, X, va, cp, th[-1], covmodel=covmodel)
    if not np.isfinite(prof["loglik"]):
        return _BIG, np.zeros_like(th), prof
    _, g = A.vecchia_likelihood_grad(data - X @ prof["beta_hat"], va, cp, th[-1], covmodel=covmodel)
    g = np.delete(g, nu_at) if matern else g
    return -prof["loglik"], -g * th, prof


def vecchia_estimate(data, locs, X="missing", m=20, covmodel="matern", theta_ini=None, output_level=1,
                     reltol=np.sqrt(np.finfo(float).eps), seed=0, maxit=300, smoothness=None, method="Nelder-Mead",
                     trend="ols", smoothness_grad=False, reneighbor=False, loo=False, block_cv=False, **specify_args):
    """block_cv=True or an array of integer block labels in the caller's order, -1 = never held out (needs cond_yz='z' and a
    named family; the default changes nothing): the result gains `block_cv`, the leave-block-out cross-validation summary of
    vecchia_block_cv at the estimate on the detrended data z, for the cells of spatial_blocks(locs) (True) or the given blocks:
    per column rmse, mae, log_score, crps, coverage95, mean_sq_std_resid, joint_log_score, and n_blocks, n_heldout.
    loo=True (needs cond_yz='z' and a named family; the default changes nothing): the result gains `loo`, the leave-one-out
    cross-validation summary of vecchia_loo at the estimate on the detrended data z (with trend="gls" the GLS residual): per
    column rmse, mae, log_score, crps, coverage95, mean_sq_std_resid.
    trend: "ols" (the reference, R/vecchia_wrappers.R:32-51: coefficients by ordinary least squares once, the covariance
    fitted to their residuals) or "gls": generalised least squares with the coefficients profiled out of the likelihood
    (vecchia_profile_likelihood: beta_hat(theta) under the Vecchia precision at every step), for X given or the constant
    column; needs cond_yz='z'.  Nelder-Mead then minimises the negative profile likelihood; "L-BFGS-B" and "fisher" take value and
    beta_hat(theta) from the profile call and gradient / information from vecchia_likelihood_grad / _fisher on the residual
    data - X beta_hat(theta) (the envelope theorem; the expected information is block diagonal between beta and theta, so
    theta_se keeps its meaning).  With "gls" the result also holds beta_cov and beta_se, beta_hat is the GLS value at theta_hat
    and z is the GLS residual.
    smoothness: a value fixes the Matern smoothness and takes it out of the search (theta_ini then holds variance, range,
    nugget).  method: "Nelder-Mead" (the reference's search) or "L-BFGS-B", which minimises over the log-parameters with the
    analytic gradient of the GPU (vecchia_likelihood_grad; d/d log theta = theta d/d theta) and needs cond_yz='z' and, for
    'matern', smoothness in {0.5, 1.5, 2.5} -- or an explicit cond_yz='SGV', the reference's default conditioning, whose gradient
    is vecchia_likelihood_grad_sgv ('matern' at such a smoothness, or 'esqe'; trend="ols", one data vector); or "fisher", Fisher scoring over the log-parameters on the expected information of
    the GPU (vecchia_likelihood_fisher, _fisher_scoring), with the preconditions of "L-BFGS-B".  n_evals counts likelihood (or
    value + gradient [+ information]) evaluations.  For "fisher" the result also holds fisher_info (the information over the
    searched parameters at theta_hat), theta_cov (its inverse) and theta_se (the square roots of that one's diagonal).
    smoothness_grad=True (covmodel='matern'): "L-BFGS-B" and "fisher" differentiate the smoothness as well
    (vecchia_likelihood_grad / _fisher with smoothness_grad=True), so they take a free smoothness -- four searched log-parameters,
    for L-BFGS-B inside box bounds that keep the smoothness in (0.01, 10], the reference's guard (:72-74) as a bound; Fisher
    scoring keeps the same interval by rejecting (and halving) a trial step that leaves it, and returns a 4 x 4 fisher_info and four theta_se, the smoothness's among them -- or any fixed one.  The covariance is
    not differentiable in the smoothness at exactly 0.5, 1.5 and 2.5: a trial point there raises ValueError.  Not with trend="gls".
    Replicated data: `data` as n x R with R > 1 holds R realisations over the same locations (an ensemble, repeated time slices);
    needs cond_yz='z', complete columns and trend="ols".  X="missing" subtracts the grand mean, X=None nothing, a given X one
    common beta_hat by OLS on the replicate mean.  "Nelder-Mead" minimises the negative sum of vecchia_likelihood_replicates;
    "L-BFGS-B" and "fisher" take value, gradient and information of the sum from ONE pass per step
    (vecchia_likelihood_grad_replicates / _fisher_replicates); fisher_info is the R-fold information, so theta_se shrinks with
    sqrt(R).  z is then the n x R residual and the result holds n_replicates.  A 1-D `data` takes the path it always took.
    covmodel='matern_scaledim': the Matern with one range per coordinate; theta_ini, theta_hat and theta_se are in the order
    variance, range_1 .. range_dim, smoothness, nugget (without the smoothness when it is fixed).  Nelder-Mead handles any
    smoothness; "L-BFGS-B" and "fisher" need a fixed smoothness in {0.5, 1.5, 2.5} and at most three coordinates.  The default
    start gives every coordinate the isotropic start's rule on its own extent (a quarter of the mean absolute difference of that
    coordinate over the sampled pairs).  trend="gls" and n x R data work as for 'matern'.  reneighbor=True: after the search the
    approximation is specified once more with scale = the fitted ranges (vecchia_specify) and the search continues from the
    estimate; the default leaves every call as it was."""
    if method not in ("Nelder-Mead", "L-BFGS-B", "fisher"):
        raise ValueError(f"method='{method}' not defined")
    fix_nu = smoothness is not None
    scaledim = isinstance(covmodel, str) and covmodel == "matern_scaledim"
    mfam = scaledim or (isinstance(covmodel, str) and covmodel == "matern")   # the families with a smoothness among the covparms
    if fix_nu and not mfam:
        raise ValueError("smoothness applies to covmodel='matern' and 'matern_scaledim' only")
    if reneighbor and not scaledim:
        raise ValueError("reneighbor applies to covmodel='matern_scaledim' only")
    if trend not in ("ols", "gls"):
        raise ValueError(f"trend='{trend}' not defined")
    gls = trend == "gls"
    if loo and (specify_args.get("cond_yz") != "z" or not isinstance(covmodel, str)):
        raise ValueError("loo=True needs cond_yz='z' and a named covariance family (the fit vecchia_loo cross-validates)")
    want_bcv = block_cv is not False and block_cv is not None
    if want_bcv and (specify_args.get("cond_yz") != "z" or not isinstance(covmodel, str)):
        raise ValueError("block_cv needs cond_yz='z' and a named covariance family (the fit vecchia_block_cv cross-validates)")
    if smoothness_grad and gls:
        raise ValueError("smoothness_grad=True is not available with trend='gls'")
    if smoothness_grad and covmodel != "matern":
        raise ValueError("smoothness_grad applies to covmodel='matern' only")
    if gls:
        if specify_args.get("cond_yz") != "z":
            raise ValueError("trend='gls' needs cond_yz='z' (the likelihood whose whitening operator the GPU applies)")
        if not isinstance(covmodel, str):
            raise ValueError("trend='gls' needs a named covariance family")
        if X is None:
            raise ValueError("trend='gls' needs a trend: X, or the constant column of X='missing'")
    # method="L-BFGS-B" with an EXPLICIT cond_yz='SGV': the gradient of the default conditioning (vecchia_likelihood_grad_sgv)
    sgv_grad = method == "L-BFGS-B" and specify_args.get("cond_yz") == "SGV"
    if sgv_grad:
        if smoothness_grad or scaledim or not isinstance(covmodel, str) or covmodel not in ("matern", "esqe"):
            raise ValueError("method='L-BFGS-B' with cond_yz='SGV' takes covmodel 'matern' (smoothness in {0.5, 1.5, 2.5}, "
                             "smoothness_grad=False) or 'esqe'")
    if method in ("L-BFGS-B", "fisher"):
        if specify_args.get("cond_yz") != "z" and not sgv_grad:
            raise ValueError(f"method='{method}' needs cond_yz='z' (the likelihood whose gradient the GPU returns)")
        if not isinstance(covmodel, str):
            raise ValueError(f"method='{method}' needs a named covariance family")
        if covmodel == "matern" and not smoothness_grad and (not fix_nu or float(smoothness) not in (0.5, 1.5, 2.5)):
            raise ValueError(f"method='{method}' with covmodel='matern' needs smoothness in {{0.5, 1.5, 2.5}}")
        if scaledim and (not fix_nu or float(smoothness) not in (0.5, 1.5, 2.5)):
            raise ValueError(f"method='{method}' with covmodel='matern_scaledim' needs smoothness in {{0.5, 1.5, 2.5}}")
    data = np.asarray(data, dtype=np.float64)
    locs = np.asarray(locs, dtype=np.float64)
    if scaledim and locs.ndim != 2:
        raise ValueError("covmodel='matern_scaledim' needs locs as an n x dim matrix")
    if scaledim and method in ("L-BFGS-B", "fisher") and locs.shape[1] > 3:
        raise ValueError(f"method='{method}' with covmodel='matern_scaledim' needs at most three coordinates")
    nu_at = locs.shape[1] + 1 if scaledim else 2                     # where the smoothness stands among the covparms
    replicated = data.ndim == 2 and data.shape[1] > 1                # R > 1 realisations over the same locations
    if replicated:
        if gls:
            raise ValueError("trend='gls' is not available with replicated data (data n x R)")
        if specify_args.get("cond_yz") != "z":
            raise ValueError("replicated data (data n x R) needs cond_yz='z' (the likelihood whose factor the replicates share)")
        if not isinstance(covmodel, str):
            raise ValueError("replicated data (data n x R) needs a named covariance family")
        if not np.all(np.isfinite(data)):
            raise ValueError("replicated data (data n x R) must be complete and finite (no NaN)")
        if data.shape[0] != locs.shape[0]:
            raise ValueError("replicated data (data n x R) must have one row per location")
    # the three likelihood calls of the objectives below: of the one data vector, or summed over the replicates (one pass)
    if replicated:
        lik = lambda z, *a, **kw: float(np.sum(A.vecchia_likelihood_replicates(z, *a, **kw)))    # noqa: E731
        lik_grad = lambda *a, **kw: A.vecchia_likelihood_grad_replicates(*a, **kw)               # noqa: E731
        lik_fisher = lambda *a, **kw: A.vecchia_likelihood_fisher_replicates(*a, **kw)           # noqa: E731
    else:
        lik = lambda *a, **kw: A.vecchia_likelihood(*a, **kw)                                     # noqa: E731
        lik_grad = lambda *a, **kw: A.vecchia_likelihood_grad(*a, **kw)                           # noqa: E731
        if sgv_grad:
            lik_grad = lambda *a, **kw: A.vecchia_likelihood_grad_sgv(*a, **kw)                   # noqa: E731
        lik_fisher = lambda *a, **kw: A.vecchia_likelihood_fisher(*a, **kw)                       # noqa: E731
    if replicated and isinstance(X, str) and X == "missing":         # the grand mean
        beta_hat = np.array([data.mean()])
        z = data - beta_hat[0]
        trend_kind = "constant"
    elif replicated and X is not None:                               # one common beta_hat: OLS on the replicate mean
        X = np.asarray(X, dtype=np.float64)
        beta_hat = np.linalg.solve(X.T @ X, X.T @ data.mean(axis=1))
        z = data - (X @ beta_hat)[:, None]
        trend_kind = "userspecified"
    elif isinstance(X, str) and X == "missing":                      # :32-37 constant trend
        beta_hat = np.array([data.mean()])
        z = data - beta_hat[0]
        trend_kind = "constant"
        Xg = np.ones((data.shape[0], 1)) if gls else None
    elif X is None:                                                  # :39-44 no trend
        beta_hat = np.array([])
        z = data
        trend_kind = "none"
    else:                                                            # :46-51 user-specified trend
        X = np.asarray(X, dtype=np.float64)
        beta_hat = np.linalg.solve(X.T @ X, X.T @ data)
        z = data - X @ beta_hat
        trend_kind = "userspecified"
        Xg = X if X.ndim == 2 else X[:, None]
    va = A.vecchia_specify(locs, m, **specify_args)                  # :55
    if covmodel == "matern" and (theta_ini is None or np.any(np.isnan(theta_ini))):   # :59-67
        var_res = np.var(z, ddof=1)                                  # (replicates: over all entries)
        n = len(z)
        idx = np.random.default_rng(seed).permutation(n)[: min(n, 300)]   # R: sample(1:n, min(n,300)) with R's RNG
        sub = locs[idx]
        dm = np.sqrt(((sub[:, None, :] - sub[None, :, :]) ** 2).sum(-1))
        theta_ini = np.array([.9 * var_res, dm.mean() / 4, .8, .1 * var_res])        # var, range, smooth, nugget
        if fix_nu:
            theta_ini = np.delete(theta_ini, 2)
    if scaledim and (theta_ini is None or np.any(np.isnan(theta_ini))):
        var_res = np.var(z, ddof=1)
        n = len(z)
        idx = np.random.default_rng(seed).permutation(n)[: min(n, 300)]
        sub = locs[idx]
        ranges = np.abs(sub[:, None, :] - sub[None, :, :]).mean(axis=(0, 1)) / 4   # the rule above, per coordinate
        theta_ini = np.concatenate([[.9 * var_res], ranges, [.8, .1 * var_res]])
        if fix_nu:
            theta_ini = np.delete(theta_ini, nu_at)
    theta_ini = np.asarray(theta_ini, dtype=np.float64)

    def full(th):                                                    # searched parameters -> (covparms, nugget)
        cp = np.concatenate([th[:nu_at], [float(smoothness)], th[nu_at:-1]]) if fix_nu else th[:-1]
        return cp, th[-1]
    n_par = len(theta_ini)
    evals = [0]
    nu_kw = dict(smoothness_grad=True) if smoothness_grad else {}    # (the default call is the call it always was)

    def negloglik(lg):                                               # :72-78
        if mfam and not fix_nu and np.exp(lg[nu_at]) > 10:
            raise RuntimeError("The default optimization routine to find parameters did not converge. "
                               "Try writing your own optimization.")
        evals[0] += 1
        th = np.exp(lg)
        cp, nug = full(th)
        return -lik(z, va, cp, nug, covmodel=covmodel)

    def negloglik_grad(lg):                                          # value and gradient in the log-parameters
        evals[0] += 1
        th = np.exp(lg)
        cp, nug = full(th)
        ll, g = lik_grad(z, va, cp, nug, covmodel=covmodel, **nu_kw)
        if mfam and fix_nu:
            g = np.delete(g, nu_at)
        elif covmodel == "matern":
            _nu_slot_checked(g[2], ll, cp[2])
        if not np.isfinite(ll):
            return _BIG, np.zeros_like(lg)
        return -ll, -g * th

    infos = {}                                                       # information over the searched parameters, by point

    def loglik_fisher(lg):                                           # value, gradient and information in the log-parameters
        evals[0] += 1
        th = np.exp(lg)
        cp, nug = full(th)
        if covmodel == "matern" and not fix_nu and not 0.01 < cp[2] <= 10.0:   # the reference's guard (:72-74) and L-BFGS-B's
            return -np.inf, np.zeros_like(th), np.eye(len(th))                 #  box: a trial step the halving loop rejects
        ll, g, info = lik_fisher(z, va, cp, nug, covmodel=covmodel, **nu_kw)
        if mfam and fix_nu:
            g, info = np.delete(g, nu_at), np.delete(np.delete(info, nu_at, axis=0), nu_at, axis=1)
        elif covmodel == "matern":
            _nu_slot_checked(g[2], ll, cp[2])
        infos[lg.tobytes()] = info
        return ll, g * th, info * np.outer(th, th)

    if gls:                                                          # the same three objectives on the profile likelihood
        def negloglik(lg):                                           # noqa: F811
            if mfam and not fix_nu and np.exp(lg[nu_at]) > 10:
                raise RuntimeError("The default optimization routine to find parameters did not converge. "
                                   "Try writing your own optimization.")
            evals[0] += 1
            cp, nug = full(np.exp(lg))
            return -A.vecchia_profile_likelihood(data, Xg, va, cp, nug, covmodel=covmodel)["loglik"]

        def negloglik_grad(lg):                                      # noqa: F811
            evals[0] += 1
            f, g, _ = profile_negloglik_grad(lg, data, Xg, va, covmodel, smoothness)
            return f, g

        def loglik_fisher(lg):                                       # noqa: F811
            evals[0] += 1
            th = np.exp(lg)
            cp, nug = full(th)
            prof = A.vecchia_profile_likelihood(data, Xg, va, cp, nug, covmodel=covmodel)
            if not np.isfinite(prof["loglik"]):
                return -np.inf, np.zeros_like(th), np.eye(len(th))
            _, g, info = A.vecchia_likelihood_fisher(data - Xg @ prof["beta_hat"], va, cp, nug, covmodel=covmodel)
            if mfam:
                g, info = np.delete(g, nu_at), np.delete(np.delete(info, nu_at, axis=0), nu_at, axis=1)
            infos[lg.tobytes()] = info
            return prof["loglik"], g * th, info * np.outer(th, th)

    def search(theta_ini):                                           # -> (xbest, fbest, conv, parscale)
        parscale = np.ones(n_par)                                        # :83-85 (entries with theta.ini == 1 stay 1; the
        non1 = theta_ini != 1                                            #  reference's rep(1, length(n.par)) leaves them NA)
        parscale[non1] = np.log(theta_ini[non1])
        x0 = np.log(theta_ini) / parscale                                # optim works on par / parscale
        if method == "L-BFGS-B":
            from scipy.optimize import minimize
            bounds = None
            if covmodel == "matern" and not fix_nu:                      # the reference's guard (:72-74: smoothness > 10 is an error)
                bounds = [(None, None)] * n_par
                bounds[2] = (np.log(0.01), np.log(10.0))
            r = minimize(negloglik_grad, np.log(theta_ini), jac=True, method="L-BFGS-B", bounds=bounds,
                         options=dict(maxiter=maxit, ftol=1e-3 * reltol, gtol=1e-5))   # (relative decrease per iteration; gradient in log-parameters)
            return r.x, float(r.fun), (0 if r.success else 1), np.ones(n_par)
        if method == "fisher":
            xbest, ll_best, _, _, _, conv = _fisher_scoring(loglik_fisher, np.log(theta_ini), reltol=reltol, maxit=maxit)
            return xbest, -ll_best, conv, np.ones(n_par)
        xbest, fbest, _, conv = _nelder_mead_nash(lambda x: negloglik(x * parscale), x0, reltol=reltol, maxit=maxit)   # :87-93
        return xbest, fbest, conv, parscale

    xbest, fbest, conv, parscale = search(theta_ini)
    if reneighbor:
        # neighbours chosen in unscaled space are poor under strong anisotropy: once more on locs / fitted ranges, from the estimate
        th = np.exp(xbest * parscale)
        va = A.vecchia_specify(locs, m, **dict(specify_args, scale=th[1:1 + locs.shape[1]]))
        infos.clear()
        xbest, fbest, conv, parscale = search(th)

    class _Res:
        x, fun = xbest, fbest
    res = _Res()
    theta_hat = np.exp(res.x * parscale)
    if gls:                                                          # the GLS coefficients and residual at the estimate
        cp_hat, nug_hat = full(theta_hat)
        prof = A.vecchia_profile_likelihood(data, Xg, va, cp_hat, nug_hat, covmodel=covmodel)
        beta_hat = prof["beta_hat"]
        z = data - Xg @ beta_hat
    rnames = tuple(f"range_{t + 1}" for t in range(locs.shape[1])) if scaledim else ("range",)
    par_names = ("variance",) + rnames + (() if fix_nu else ("smoothness",)) + ("nugget",)
    if output_level > 0:                                             # :98-101
        print("estimated trend coefficients:\n", beta_hat)
        print("estimated covariance parameters:\n",
              dict(zip(par_names, theta_hat)))
    out = dict(z=z, beta_hat=beta_hat, theta_hat=theta_hat, trend=trend_kind, locs=locs, covmodel=covmodel,
               n_evals=evals[0], neg_loglik=float(res.fun), convergence=conv)
    if replicated:
        out["n_replicates"] = int(data.shape[1])
    if method == "fisher":
        out["fisher_info"] = infos[np.asarray(xbest).tobytes()]
        out["theta_cov"] = np.linalg.inv(out["fisher_info"])
        out["theta_se"] = np.sqrt(np.diag(out["theta_cov"]))
    if gls:
        out["beta_cov"] = prof["beta_cov"]
        out["beta_se"] = np.sqrt(np.diag(prof["beta_cov"]))
    if loo:
        cp_hat, nug_hat = full(theta_hat)
        cv = A.vecchia_loo(z, va, cp_hat, nug_hat, covmodel=covmodel)
        out["loo"] = {k: cv[k] for k in ("rmse", "mae", "log_score", "crps", "coverage95", "mean_sq_std_resid")}
    if want_bcv:
        cp_hat, nug_hat = full(theta_hat)
        cv = A.vecchia_block_cv(z, va, cp_hat, nug_hat, covmodel=covmodel, blocks=None if block_cv is True else block_cv)
        out["block_cv"] = {k: cv[k] for k in ("rmse", "mae", "log_score", "crps", "coverage95", "mean_sq_std_resid",
                                              "joint_log_score", "n_blocks", "n_heldout")}
    return out


def vecchia_pred(vecchia_est, locs_pred, X_pred=None, m=30, device=0, local=False, groups=None, weights=None, return_cov=False,
                 nsim=0, seed=0, **specify_args):
    """R/vecchia_wrappers.R:134-161: spatial prediction at new locations from the result of vecchia_estimate, with the
    exact prediction variances of the latent field (vecchia_prediction(..., return_values='meanvar')).  With prediction locations in two or more dimensions vecchia_specify defaults to
    cond.yz='zy' (R/vecchia_specify.R:92-96), whose posterior mean is one triangular solve on the GPU.
    local=True (the default changes nothing): the prediction of the cond_yz='z' model itself, the one vecchia_estimate fits with
    cond_yz='z', by local kriging on the m nearest observations of every location (vecchia_krige): no posterior pass, any
    number of prediction locations.  The observations are specified again with cond_yz='z' (specify_args as for
    vecchia_estimate); the trend is added back as below.
    groups (with local=True): one integer label per prediction location; the members of a group are predicted jointly
    (vecchia_krige_groups, with weights and return_cov), and group_ids, group_mean (the trend included), group_var, n_failed
    and, with return_cov, group_cov join what is returned.  Without groups it is the call it was.
    nsim > 0 (with local=True, without groups): nsim spatially coherent conditional draws of the latent field over locs_pred
    (vecchia_cond_sim, max-min sweep order, `seed`) join what is returned as draws (n_p, nsim), the trend included, with
    n_failed; mean_pred and var_pred stay those of local kriging."""
    import warnings
    theta_hat = np.asarray(vecchia_est["theta_hat"], dtype=np.float64)                               # :140-143
    if groups is not None and not local:
        raise ValueError("groups are predicted by local kriging: local=True")
    if nsim and (not local or groups is not None):
        raise ValueError("conditional draws come from the sequential kriging sweep: local=True, no groups")
    extra = {}
    if local:
        if specify_args.setdefault("cond_yz", "z") != "z":
            raise ValueError("local=True predicts the cond_yz='z' model")
        if np.asarray(vecchia_est["z"]).ndim != 1:
            raise ValueError("local=True takes the result of an estimation from one data vector")
        va = A.vecchia_specify(vecchia_est["locs"], m, **specify_args)
        if groups is None:
            kr = A.vecchia_krige(vecchia_est["z"], va, locs_pred, theta_hat[:-1], theta_hat[-1],
                                 covmodel=vecchia_est.get("covmodel", "matern"), scale=specify_args.get("scale"), device=device)
        else:                                            # the trend joins the locations' and the groups' means alike
            trend = None
            if X_pred is not None:
                trend = np.asarray(X_pred, dtype=np.float64) @ vecchia_est["beta_hat"]
            elif vecchia_est["trend"] == "constant":
                trend = np.asarray(vecchia_est["beta_hat"][0], dtype=np.float64)
            kr = A.vecchia_krige_groups(vecchia_est["z"], va, locs_pred, groups, theta_hat[:-1], theta_hat[-1],
                                        covmodel=vecchia_est.get("covmodel", "matern"), weights=weights, mean_pred=trend,
                                        scale=specify_args.get("scale"), return_cov=return_cov, device=device)
            if vecchia_est["trend"] not in ("none", "constant") and X_pred is None:
                warnings.warn("X.pred was not specified, so no trend was added back to the predictions")
            extra = {k: kr[k] for k in ("group_ids", "group_mean", "group_var", "n_failed", "group_cov") if k in kr}
        preds = dict(mu_pred=kr["mean_pred"], var_pred=kr["var_pred"])
    else:
        from .laplace import vecchia_prediction
        va = A.vecchia_specify(vecchia_est["locs"], m, locs_pred=np.asarray(locs_pred, dtype=np.float64), **specify_args)   # :137
        preds = vecchia_prediction(vecchia_est["z"], va, theta_hat[:-1], theta_hat[-1],
                                   covmodel=vecchia_est.get("covmodel", "matern"), return_values="meanvar", device=device)
    if extra:
        mu_pred = preds["mu_pred"]
    elif X_pred is not None:                                                                         # :146-147
        mu_pred = preds["mu_pred"] + np.asarray(X_pred, dtype=np.float64) @ vecchia_est["beta_hat"]
    elif vecchia_est["trend"] == "none":                                                             # :148-149
        mu_pred = preds["mu_pred"]
    elif vecchia_est["trend"] == "constant":                                                         # :150-151
        mu_pred = preds["mu_pred"] + vecchia_est["beta_hat"][0]
    else:                                                                                            # :152-156
        mu_pred = preds["mu_pred"]
        warnings.warn("X.pred was not specified, so no trend was added back to the predictions")
    if nsim:                                             # the draws of the latent field, the trend the mean got added to them too
        cs = A.vecchia_cond_sim(vecchia_est["z"], va, locs_pred, theta_hat[:-1], theta_hat[-1],
                                covmodel=vecchia_est.get("covmodel", "matern"), nsim=int(nsim), seed=seed,
                                scale=specify_args.get("scale"), device=device)
        if X_pred is not None:
            trend = (np.asarray(X_pred, dtype=np.float64) @ vecchia_est["beta_hat"]).reshape(-1, 1)
        else:
            trend = vecchia_est["beta_hat"][0] if vecchia_est["trend"] == "constant" else 0.0
        extra = dict(draws=cs["draws"] + trend, n_failed=cs["n_failed"])
    return dict(mean_pred=mu_pred, var_pred=preds["var_pred"], **extra)                                           # :159
