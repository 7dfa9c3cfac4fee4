"""Truth for the expected Fisher information of the cond.yz='z' Vecchia log-likelihood: a restatement of its DEFINITION in numpy,
holding no product code.

Per conditioning set with valid entries J (own point last) and c = J without the own point, S' = C(J, J) + tau I, D_i = dS'/dtheta_i
elementwise (the identity for the nugget), S'_c and D_i,c their leading blocks:
    F_k[i, j] = 1/2 tr(S'^-1 D_i S'^-1 D_j) - 1/2 tr(S'_c^-1 D_i,c S'_c^-1 D_j,c)
the information of N(z_J; 0, S') minus that of N(z_c; 0, S'_c); the total is the sum over the rows.

Rows are returned as the upper triangle, row-major with i <= j, over {covparms..., tau}; every entry that involves the smoothness of
'matern' is NaN (not differentiated).
  rows_f64        every row of a plan by the definition, float64, batched by row length (numpy.linalg.inv)
  row_ld          one row by the definition over numpy.longdouble, with the Cholesky of _grad_truth: the adjudicator
  rows_form_f64   every row by the form the product computes (t_i'y_j / u_last - 1/2 a_i a_j / u_last^2), float64
  dense           1/2 tr(S^-1 D_i S^-1 D_j) of the whole field as a square matrix (what m = n - 1 must sum to)
  full_rows_f64, full_row_ld   {l_k, its derivatives} of _grad_truth followed by the triangle: a row of the product's row_terms"""
import numpy as np

import _grad_truth as T


def npar(covmodel):
    return 4 if covmodel == "matern" else 5


def ntri(covmodel):
    return npar(covmodel) * (npar(covmodel) + 1) // 2


def _positions(covmodel):
    """position of each differentiated parameter (the nugget last) among {covparms..., tau}"""
    return [0, 1, 3] if covmodel == "matern" else [0, 1, 2, 3, 4]


def square(covmodel, F):
    """(..., k, k) over the differentiated parameters -> (..., npar, npar) with NaN for the smoothness"""
    F = np.asarray(F)
    pos, n_ = _positions(covmodel), npar(covmodel)
    out = np.full(F.shape[:-2] + (n_, n_), np.nan, dtype=F.dtype)
    for a, i in enumerate(pos):
        for b, j in enumerate(pos):
            out[..., i, j] = F[..., a, b]
    return out


def tri(M):
    """upper triangle of (..., n, n), row-major with i <= j"""
    n_ = M.shape[-1]
    return np.stack([M[..., i, j] for i in range(n_) for j in range(i, n_)], axis=-1)


def untri(t, n_):
    M = np.zeros((n_, n_), dtype=np.asarray(t).dtype)
    s = 0
    for i in range(n_):
        for j in range(i, n_):
            M[i, j] = M[j, i] = t[s]
            s += 1
    return M


def _half_traces(Sinv, dmats):
    """1/2 tr(S^-1 D_i S^-1 D_j) for all pairs; Sinv (..., g, g), dmats a list of (..., g, g); g = 0 gives zeros"""
    A = [Sinv @ D for D in dmats]
    k = len(dmats)
    out = np.zeros(Sinv.shape[:-2] + (k, k), dtype=Sinv.dtype)
    for i in range(k):
        for j in range(k):
            out[..., i, j] = (A[i] * np.swapaxes(A[j], -1, -2)).sum(axis=(-1, -2)) / 2
    return out


def _blocks(x, covmodel, cp, tau):
    """S' and the list of its derivative matrices (the nugget's last) for the points x[..., i, :]"""
    g = x.shape[-2]
    C, dC = T._cov_and_derivs(T._dist(x), covmodel, cp)
    eye = np.broadcast_to(np.eye(g, dtype=x.dtype), C.shape)
    return C + x.dtype.type(tau) * eye, list(dC) + [eye + np.zeros_like(C)]


def _groups(revNN):
    nn = np.nan_to_num(np.asarray(revNN, dtype=np.float64), nan=0.0).astype(np.int64)
    n0 = (nn > 0).sum(axis=1)
    for g in np.unique(n0):
        rows = np.where(n0 == g)[0]
        yield g, rows, np.stack([nn[k][nn[k] > 0] - 1 for k in rows])


def rows_f64(locsord, revNN, covmodel, cp, tau):
    """(n, ntri) float64: every row of the plan, by the definition"""
    locsord = np.asarray(locsord, dtype=np.float64)
    out = np.full((np.asarray(revNN).shape[0], ntri(covmodel)), np.nan)
    for g, rows, idx in _groups(revNN):
        S, D = _blocks(locsord[idx], covmodel, cp, tau)
        F = _half_traces(np.linalg.inv(S), D)
        if g > 1:
            F = F - _half_traces(np.linalg.inv(S[..., :-1, :-1]), [d[..., :-1, :-1] for d in D])
        out[rows] = tri(square(covmodel, F))
    return out


def rows_form_f64(locsord, revNN, covmodel, cp, tau):
    """(n, ntri) float64: every row by t_i'y_j / u_last - 1/2 a_i a_j / u_last^2 (solves with S' only)"""
    locsord = np.asarray(locsord, dtype=np.float64)
    out = np.full((np.asarray(revNN).shape[0], ntri(covmodel)), np.nan)
    for g, rows, idx in _groups(revNN):
        S, D = _blocks(locsord[idx], covmodel, cp, tau)
        e = np.zeros((len(rows), g, 1))
        e[:, -1, 0] = 1.0
        u = np.linalg.solve(S, e)
        t = np.concatenate([d @ u for d in D], axis=-1)              # (rows, g, k)
        y = np.linalg.solve(S, t)
        ul = u[:, -1, 0]
        a = (u * t).sum(axis=1)                                       # (rows, k)
        F = np.swapaxes(t, -1, -2) @ y / ul[:, None, None] - 0.5 * a[:, :, None] * a[:, None, :] / (ul * ul)[:, None, None]
        out[rows] = tri(square(covmodel, F))
    return out


def row_ld(locsord, revNN_row, covmodel, cp, tau):
    """(ntri,) numpy.longdouble: one row, by the definition"""
    idx = T.valid_entries(revNN_row)
    x = np.asarray(locsord, dtype=np.float64)[idx].astype(np.longdouble)
    S, D = _blocks(x, covmodel, [np.longdouble(v) for v in cp], np.longdouble(tau))
    g = len(idx)

    def traces(S_, D_):
        A = [T._chol_solve_ld(S_, np.array(d)) for d in D_]
        return np.array([[(A[i] * A[j].T).sum() / 2 for j in range(len(D_))] for i in range(len(D_))], dtype=np.longdouble)
    F = traces(S, D)
    if g > 1:
        F = F - traces(S[:-1, :-1], [d[:-1, :-1] for d in D])
    return tri(square(covmodel, F))


def dense(locs, covmodel, cp, tau):
    """(npar, npar) float64: 1/2 tr(S^-1 D_i S^-1 D_j) of log N(z; 0, C + tau I), NaN for the smoothness"""
    S, D = _blocks(np.asarray(locs, dtype=np.float64), covmodel, cp, tau)
    return square(covmodel, _half_traces(np.linalg.inv(S), D))


def full_rows_f64(locsord, revNN, z_ord, covmodel, cp, tau):
    return np.concatenate([T.rows_f64(locsord, revNN, z_ord, covmodel, cp, tau), rows_f64(locsord, revNN, covmodel, cp, tau)], axis=1)


def full_row_ld(locsord, revNN_row, z_ord, covmodel, cp, tau):
    return np.concatenate([T.row_ld(locsord, revNN_row, z_ord, covmodel, cp, tau), row_ld(locsord, revNN_row, covmodel, cp, tau)])
