"""Truth for covmodel='matern_scaledim' (one range per coordinate): value, gradient and expected information of the cond.yz='z'
Vecchia log-likelihood per conditioning set, dense algebra in numpy, holding no product code.

covparms = (variance, range_1 .. range_dim, smoothness in {0.5, 1.5, 2.5}).  With d_t = (x_t - x'_t) / range_t and
h = sqrt(sum_t d_t^2), summed in coordinate order, c = sqrt(3) / sqrt(5):
    nu 0.5   C = s2 e^{-h}                       dC/drange_t = s2 e^{-h} d_t^2 / (h range_t), 0 at h = 0
    nu 1.5   C = s2 (1 + ch) e^{-ch}             dC/drange_t = s2 c^2 e^{-ch} d_t^2 / range_t
    nu 2.5   C = s2 (1 + ch + c^2 h^2 / 3) e^{-ch}   dC/drange_t = s2 e^{-ch} (c^2 / 3)(1 + ch) d_t^2 / range_t
The per-set formulas are those of _grad_truth (l_k and its derivatives) and _fisher_truth (the information by its definition).

Rows: {l_k, d/d variance, d/d range_1 .. range_dim, NaN (smoothness, not differentiated), d/d tau}, then for the full rows the upper
triangle, row-major, of the (dim + 3) square information with NaN wherever the smoothness is involved.
(The truth of the EVALUATION is the oracle's isotropic algorithm on locs / ranges at range 1; it is not restated here.)
  rows_f64, row_ld, total_ld, dense_mvn        as in _grad_truth
  info_rows_f64, info_row_ld, full_rows_f64, full_row_ld, rep_rows_f64       as in _fisher_truth; rep: summed over the columns of Z"""
import numpy as np

import _fisher_truth as F
import _grad_truth as T


def ncols(dim):
    return dim + 4


def npar(dim):
    return dim + 3


def cov_and_derivs(x, cp):
    """C and [dC/dvariance, dC/drange_1, ...] for the points x[..., i, :]; any float dtype"""
    ft = x.dtype.type
    dim = x.shape[-1]
    assert len(cp) == dim + 2
    s2, rng, nu = ft(cp[0]), [ft(v) for v in cp[1:1 + dim]], float(cp[dim + 1])
    h2 = np.zeros(x.shape[:-1] + (x.shape[-2],), dtype=x.dtype)
    dq = []
    for t in range(dim):
        d = (x[..., :, None, t] - x[..., None, :, t]) / rng[t]
        dq.append(d * d)
        h2 = h2 + d * d
    h = np.sqrt(h2)
    if nu == 0.5:
        e = np.exp(-h)
        dvar = e
        g = np.where(h > 0, s2 * e / np.where(h > 0, h, ft(1)), ft(0))
    elif nu == 1.5:
        c = np.sqrt(ft(3))
        e = np.exp(-c * h)
        dvar = (1 + c * h) * e
        g = s2 * c * c * e
    elif nu == 2.5:
        c = np.sqrt(ft(5))
        t_ = c * h
        e = np.exp(-t_)
        dvar = (1 + t_ + t_ * t_ / 3) * e
        g = s2 * e * (c * c / 3) * (1 + t_)
    else:
        raise ValueError("smoothness must be 0.5, 1.5 or 2.5")
    return s2 * dvar, [dvar] + [g * dq[t] / rng[t] for t in range(dim)]


def _spread(ell, d):
    """{l, d/d variance, d/d ranges, NaN, d/d tau}; d = derivatives with the nugget's last"""
    return np.stack([ell] + list(d[:-1]) + [np.full_like(ell, np.nan), d[-1]], axis=-1)


def _square(Fm, dim):
    pos = list(range(dim + 1)) + [dim + 2]
    out = np.full(Fm.shape[:-2] + (npar(dim), npar(dim)), np.nan, dtype=Fm.dtype)
    for a, i in enumerate(pos):
        for b, j in enumerate(pos):
            out[..., i, j] = Fm[..., a, b]
    return out


def _blocks(x, cp, tau):
    g = x.shape[-2]
    C, dC = cov_and_derivs(x, cp)
    eye = np.broadcast_to(np.eye(g, dtype=x.dtype), C.shape)
    return C + x.dtype.type(tau) * eye, list(dC) + [eye + np.zeros_like(C)]


def rows_f64(locsord, revNN, z_ord, cp, tau):
    locsord = np.asarray(locsord, dtype=np.float64)
    z_ord = np.asarray(z_ord, dtype=np.float64)
    out = np.full((np.asarray(revNN).shape[0], ncols(locsord.shape[1])), np.nan)
    for g, rows, idx in F._groups(revNN):
        x, zJ = locsord[idx], z_ord[idx]
        S, D = _blocks(x, cp, tau)
        e = np.zeros(g)
        e[-1] = 1.0
        sol = np.linalg.solve(S, np.stack([np.broadcast_to(e, zJ.shape), zJ], axis=-1))
        ell, d = T._terms(sol[..., 0], sol[..., 1], zJ, D[:-1] + [None])
        out[rows] = _spread(ell, d)
    return out


def row_ld(locsord, revNN_row, z_ord, cp, tau):
    idx = T.valid_entries(revNN_row)
    x = np.asarray(locsord, dtype=np.float64)[idx].astype(np.longdouble)
    zJ = np.asarray(z_ord, dtype=np.float64)[idx].astype(np.longdouble)
    S, D = _blocks(x, [np.longdouble(v) for v in cp], np.longdouble(tau))
    rhs = np.zeros((len(idx), 2), dtype=np.longdouble)
    rhs[-1, 0] = 1
    rhs[:, 1] = zJ
    sol = T._chol_solve_ld(S, rhs)
    ell, d = T._terms(sol[:, 0], sol[:, 1], zJ, D[:-1] + [None])
    return _spread(ell, d)


def total_ld(locsord, revNN, z_ord, cp, tau):
    rev = np.asarray(revNN)
    tot = np.zeros(ncols(np.asarray(locsord).shape[1]), dtype=np.longdouble)
    for k in range(rev.shape[0]):
        tot = tot + row_ld(locsord, rev[k], z_ord, cp, tau)
    return tot


def dense_mvn(locs, z, cp, tau):
    """value and gradient {variance, ranges, NaN, tau} of log N(z; 0, C + tau I), float64"""
    locs, z = np.asarray(locs, dtype=np.float64), np.asarray(z, dtype=np.float64)
    n = len(z)
    S, D = _blocks(locs, cp, tau)
    Lc = np.linalg.cholesky(S)
    alpha = np.linalg.solve(S, z)
    Sinv = np.linalg.inv(S)
    ll = -np.log(np.diag(Lc)).sum() - 0.5 * z @ alpha - n * T.HALF_LOG_2PI
    g = [np.float64(-0.5 * np.sum(Sinv * Dm) + 0.5 * alpha @ Dm @ alpha) for Dm in D]
    return ll, _spread(np.float64(ll), g)[1:]


def info_rows_f64(locsord, revNN, cp, tau):
    locsord = np.asarray(locsord, dtype=np.float64)
    dim = locsord.shape[1]
    out = np.full((np.asarray(revNN).shape[0], npar(dim) * (npar(dim) + 1) // 2), np.nan)
    for g, rows, idx in F._groups(revNN):
        S, D = _blocks(locsord[idx], cp, tau)
        Fm = F._half_traces(np.linalg.inv(S), D)
        if g > 1:
            Fm = Fm - F._half_traces(np.linalg.inv(S[..., :-1, :-1]), [d[..., :-1, :-1] for d in D])
        out[rows] = F.tri(_square(Fm, dim))
    return out


def info_row_ld(locsord, revNN_row, cp, tau):
    idx = T.valid_entries(revNN_row)
    x = np.asarray(locsord, dtype=np.float64)[idx].astype(np.longdouble)
    S, D = _blocks(x, [np.longdouble(v) for v in cp], np.longdouble(tau))

    def traces(S_, D_):
        A = [T._chol_solve_ld(S_, np.array(d)) for d in D_]
        return np.array([[(A[i] * A[j].T).sum() / 2 for j in range(len(D_))] for i in range(len(D_))], dtype=np.longdouble)
    Fm = traces(S, D)
    if len(idx) > 1:
        Fm = Fm - traces(S[:-1, :-1], [d[:-1, :-1] for d in D])
    return F.tri(_square(Fm, x.shape[1]))


def full_rows_f64(locsord, revNN, z_ord, cp, tau):
    return np.concatenate([rows_f64(locsord, revNN, z_ord, cp, tau), info_rows_f64(locsord, revNN, cp, tau)], axis=1)


def full_row_ld(locsord, revNN_row, z_ord, cp, tau):
    return np.concatenate([row_ld(locsord, revNN_row, z_ord, cp, tau), info_row_ld(locsord, revNN_row, cp, tau)])


def rep_rows_f64(locsord, revNN, Z_ord, cp, tau):
    """full rows summed over the columns of Z_ord (n, R): the information is R times one column's"""
    Z = np.asarray(Z_ord, dtype=np.float64)
    lead = sum(rows_f64(locsord, revNN, Z[:, r], cp, tau) for r in range(Z.shape[1]))
    return np.concatenate([lead, Z.shape[1] * info_rows_f64(locsord, revNN, cp, tau)], axis=1)
