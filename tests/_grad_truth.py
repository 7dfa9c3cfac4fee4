"""Truth for the analytic gradient of the cond.yz='z' Vecchia log-likelihood: a restatement of the formula in numpy, holding no
product code.

Per conditioning set with valid entries J (own point last), S' = C(J, J) + tau I, u = S'^-1 e_last, w = S'^-1 z_J, q = u'z_J:
    l_k = 1/2 log u_last - 1/2 q^2 / u_last - 1/2 log 2 pi
    dl_k/dtheta = -1/2 a / u_last + q b / u_last - 1/2 q^2 a / u_last^2,  a = u'D u, b = w'D u, D = dS'/dtheta elementwise.

Rows are returned as {l_k, d/d covparms..., d/d tau}; the smoothness column of 'matern' is NaN (not differentiated).
  rows_f64   every row of a plan, float64, batched by row length (numpy.linalg.solve)
  row_ld     one row with a hand-written Cholesky over numpy.longdouble: the adjudicator
  dense_mvn  value and gradient of the dense multivariate normal (what m = n - 1 must equal)"""
import numpy as np

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


def ncols(covmodel):
    return 5 if covmodel == "matern" else 6


def _cov_and_derivs(r, covmodel, cp):
    """C(r) and its derivatives by the covariance parameters that are differentiated, in covparms order; any float dtype."""
    ft = r.dtype.type
    if covmodel == "matern":
        s2, rho, nu = ft(cp[0]), ft(cp[1]), float(cp[2])
        if nu == 0.5:
            e = np.exp(-r / rho)
            return s2 * e, [e, s2 * e * r / (rho * rho)]
        if nu == 1.5:
            c = np.sqrt(ft(3)) / rho
            e = np.exp(-c * r)
            return s2 * (1 + c * r) * e, [(1 + c * r) * e, s2 * c * c * r * r * e / rho]
        if nu == 2.5:
            c = np.sqrt(ft(5)) / rho
            e = np.exp(-c * r)
            t = c * r
            return s2 * (1 + t + t * t / 3) * e, [(1 + t + t * t / 3) * e, s2 * e * (t * t / 3) * (1 + t) / rho]
        raise ValueError("smoothness must be 0.5, 1.5 or 2.5")
    if covmodel == "esqe":
        s1, r1, s2, r2 = (ft(v) for v in cp)
        e1 = np.exp(-r / r1)
        e2 = np.exp(-(r / r2) ** 2)
        return s1 * e1 + s2 * e2, [e1, s1 * e1 * r / (r1 * r1), e2, s2 * e2 * 2 * r * r / (r2 * r2 * r2)]
    raise ValueError(covmodel)


def _spread(covmodel, ell, dcov, dtau):
    """{l, derivatives} in the layout of the product: NaN for the smoothness of 'matern'."""
    nan = np.full_like(ell, np.nan)
    cols = [ell, dcov[0], dcov[1], nan, dtau] if covmodel == "matern" else [ell] + list(dcov) + [dtau]
    return np.stack(cols, axis=-1)


def _dist(x):
    """pair distances of the points x[..., i, :], summed over the coordinates in order"""
    r2 = np.zeros(x.shape[:-1] + (x.shape[-2],), dtype=x.dtype)
    for t in range(x.shape[-1]):
        df = x[..., :, None, t] - x[..., None, :, t]
        r2 = r2 + df * df
    return np.sqrt(r2)


def _terms(u, w, zJ, dmats):
    ul = u[..., -1]
    q = (u * zJ).sum(-1)
    ell = 0.5 * np.log(ul) - 0.5 * q * q / ul - u.dtype.type(HALF_LOG_2PI)
    out = []
    for D in dmats:
        if D is None:                                   # the nugget: identity
            a, b = (u * u).sum(-1), (w * u).sum(-1)
        else:
            Du = (D * u[..., None, :]).sum(-1)
            a, b = (u * Du).sum(-1), (w * Du).sum(-1)
        out.append(-0.5 * a / ul + q * b / ul - 0.5 * q * q * a / (ul * ul))
    return ell, out


def valid_entries(revNN_row):
    """0-based indices of a row's valid entries in stored order (own point last); 0 / negative / NaN = missing"""
    v = np.nan_to_num(np.asarray(revNN_row, dtype=np.float64), nan=0.0).astype(np.int64)
    return v[v > 0] - 1


def rows_f64(locsord, revNN, z_ord, covmodel, cp, tau):
    """(n, ncols) float64: every row of the plan"""
    locsord = np.asarray(locsord, dtype=np.float64)
    z_ord = np.asarray(z_ord, dtype=np.float64)
    nn = np.nan_to_num(np.asarray(revNN, dtype=np.float64), nan=0.0).astype(np.int64)
    n = nn.shape[0]
    out = np.full((n, ncols(covmodel)), np.nan)
    n0 = (nn > 0).sum(axis=1)
    for g in np.unique(n0):
        rows = np.where(n0 == g)[0]
        idx = np.stack([nn[k][nn[k] > 0] - 1 for k in rows])          # (rows, g)
        x, zJ = locsord[idx], z_ord[idx]
        C, dC = _cov_and_derivs(_dist(x), covmodel, cp)
        S = C + tau * np.eye(g)
        e = np.zeros(g)
        e[-1] = 1.0
        rhs = np.stack([np.broadcast_to(e, zJ.shape), zJ], axis=-1)
        sol = np.linalg.solve(S, rhs)
        ell, d = _terms(sol[..., 0], sol[..., 1], zJ, dC + [None])
        out[rows] = _spread(covmodel, ell, d[:-1], d[-1])
    return out


def _chol_solve_ld(S, rhs):
    """S x = rhs by a hand-written Cholesky and two substitutions, numpy.longdouble throughout"""
    g = S.shape[0]
    Lc = np.zeros((g, g), dtype=np.longdouble)
    for j in range(g):
        d = S[j, j] - (Lc[j, :j] * Lc[j, :j]).sum()
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite")
        Lc[j, j] = np.sqrt(d)
        if j + 1 < g:
            Lc[j + 1:, j] = (S[j + 1:, j] - (Lc[j + 1:, :j] * Lc[j, :j]).sum(axis=1)) / Lc[j, j]
    y = np.zeros_like(rhs)
    for i in range(g):
        y[i] = (rhs[i] - (Lc[i, :i, None] * y[:i]).sum(axis=0)) / Lc[i, i]
    x = np.zeros_like(rhs)
    for i in range(g - 1, -1, -1):
        x[i] = (y[i] - (Lc[i + 1:, i, None] * x[i + 1:]).sum(axis=0)) / Lc[i, i]
    return x


def row_ld(locsord, revNN_row, z_ord, covmodel, cp, tau):
    """(ncols,) numpy.longdouble: one row"""
    idx = valid_entries(revNN_row)
    x = np.asarray(locsord, dtype=np.float64)[idx].astype(np.longdouble)
    zJ = np.asarray(z_ord, dtype=np.float64)[idx].astype(np.longdouble)
    g = len(idx)
    C, dC = _cov_and_derivs(_dist(x), covmodel, [np.longdouble(v) for v in cp])
    S = C + np.longdouble(tau) * np.eye(g, dtype=np.longdouble)
    rhs = np.zeros((g, 2), dtype=np.longdouble)
    rhs[-1, 0] = 1
    rhs[:, 1] = zJ
    sol = _chol_solve_ld(S, rhs)
    ell, d = _terms(sol[:, 0], sol[:, 1], zJ, dC + [None])
    return _spread(covmodel, ell, d[:-1], d[-1])


def total_ld(locsord, revNN, z_ord, covmodel, cp, tau):
    """sum over all rows in numpy.longdouble (for central differences of the value)"""
    tot = np.zeros(ncols(covmodel), dtype=np.longdouble)
    for k in range(np.asarray(revNN).shape[0]):
        tot = tot + row_ld(locsord, np.asarray(revNN)[k], z_ord, covmodel, cp, tau)
    return tot


def dense_mvn(locs, z, covmodel, cp, tau):
    """value and gradient {d/d covparms (NaN for the smoothness), d/d tau} of log N(z; 0, C + tau I), float64"""
    locs = np.asarray(locs, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    n = len(z)
    C, dC = _cov_and_derivs(_dist(locs), covmodel, cp)
    S = C + tau * np.eye(n)
    Lc = np.linalg.cholesky(S)
    alpha = np.linalg.solve(S, z)
    Sinv = np.linalg.inv(S)
    ll = -np.log(np.diag(Lc)).sum() - 0.5 * z @ alpha - n * HALF_LOG_2PI
    g = [-0.5 * np.sum(Sinv * D) + 0.5 * alpha @ D @ alpha for D in dC]
    g.append(-0.5 * np.trace(Sinv) + 0.5 * alpha @ alpha)
    return ll, _spread(covmodel, np.float64(ll), [np.float64(v) for v in g[:-1]], np.float64(g[-1]))[1:]


def scaled_row_error(got, want):
    """max over rows of |got - want|_inf / max(|want|_inf, 1), NaN columns must agree"""
    got, want = np.atleast_2d(np.asarray(got, dtype=np.float64)), np.atleast_2d(np.asarray(want, dtype=np.float64))
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern differs"
    m = ~np.isnan(want[0])
    err = np.abs(got[:, m] - want[:, m]).max(axis=1)
    return err / np.maximum(np.abs(want[:, m]).max(axis=1), 1.0)
