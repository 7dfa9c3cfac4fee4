"""Truth for the transposed whitening operator, the precision products and the leave-one-out cross-validation
(gpv_plan_whiten_t / gpv_plan_precision / gpv_plan_loo): the DEFINITION restated in numpy.longdouble, holding no product code and
never looking at Lentries.

Row k of the whitening operator T, with valid entries J (own point last) and S = C(J, J) + diag(tau_J) = R R', is the last row
of R^-1 spread over the columns J: e_k(b) = (R^-1 b_J)_last (tests/_whiten_truth.py).  The rows come from the hand-written
Cholesky of _whiten_truth with an identity right-hand side of the row's own size (r x g x g per group of rows of equal length),
and T is kept sparse: per group (rows, idx, w) with T[rows[a], idx[a, j]] = w[a, j].

  factor_ld     the groups of a plan
  apply_T / apply_Tt / qdiag     T B, T'E, diag(T'T)
  dense_T       T as a dense matrix (small plans)
  loo_ld        leave-one-out mean, variance, standardised residual, the six score sums and the sums of their |terms|
  dense_loo     the same mean and variance from inv(C + tau I), dense (what m = n - 1 must equal)
  spd_inv_ld    inverse of a symmetric positive definite matrix by the written-out Cholesky
  index_py      the transposed index of a plan's index arrays, restated (gpv_loo_index_host)"""
import math

import numpy as np

from _grad_truth import _cov_and_derivs, _dist
from _whiten_truth import _chol_forward_ld

LD = np.longdouble
Z95 = 1.959963984540054


def factor_ld(locsord, revNN, covmodel, cp, tau):
    """locsord (n, d); revNN (n, p) 1-based, 0 / NaN = missing, own point last; tau a constant or (n,) ordered nuggets."""
    locs = np.asarray(locsord, dtype=np.float64).astype(LD)
    nn = np.nan_to_num(np.asarray(revNN, dtype=np.float64), nan=0.0).astype(np.int64)
    n = nn.shape[0]
    tv = np.broadcast_to(np.asarray(tau, dtype=np.float64), (n,)).astype(LD)
    cpl = [LD(v) for v in cp]
    n0 = (nn > 0).sum(axis=1)
    groups = []
    for g in np.unique(n0):
        rows = np.where(n0 == g)[0]
        idx = np.stack([nn[k][nn[k] > 0] - 1 for k in rows])
        C, _ = _cov_and_derivs(_dist(locs[idx]), covmodel, cpl)
        S = C + tv[idx][:, :, None] * np.eye(g, dtype=LD)
        eye = np.broadcast_to(np.eye(g, dtype=LD), (len(rows), g, g)).copy()
        w, _ = _chol_forward_ld(S, eye)                # last row of R^-1: (r, g)
        groups.append((rows, idx, w))
    return groups


def _cols(A):
    A = np.asarray(A)
    return (A[:, None] if A.ndim == 1 else A).astype(LD)


def apply_T(F, B):
    B = _cols(B)
    E = np.zeros_like(B)
    for rows, idx, w in F:
        E[rows] = (w[:, :, None] * B[idx]).sum(axis=1)
    return E


def apply_Tt(F, E):
    E = _cols(E)
    out = np.zeros_like(E)
    for rows, idx, w in F:
        for j in range(idx.shape[1]):
            np.add.at(out, idx[:, j], w[:, j, None] * E[rows])
    return out


def qdiag(F, n):
    q = np.zeros(n, dtype=LD)
    for rows, idx, w in F:
        for j in range(idx.shape[1]):
            np.add.at(q, idx[:, j], w[:, j] * w[:, j])
    return q


def dense_T(F, n):
    T = np.zeros((n, n), dtype=LD)
    for rows, idx, w in F:
        for j in range(idx.shape[1]):
            np.add.at(T, (rows, idx[:, j]), w[:, j])
    return T


_erf = np.vectorize(math.erf, otypes=[np.float64])


def loo_from(Z, r, q):
    """mean, var, s and the score sums from r = Q z and q = diag Q (long double; erf in double: 1e-16 of a term)."""
    Z, r = _cols(Z), _cols(r)
    q = np.asarray(q, dtype=LD)[:, None]
    d = r / q
    v = 1 / q
    s = r / np.sqrt(q)
    s64 = s.astype(np.float64)
    Phi2m1 = _erf(s64 / math.sqrt(2.0)).astype(LD)
    phi = np.exp(-s * s / 2) / np.sqrt(2 * LD(np.pi))
    crps = np.sqrt(v) * (s * Phi2m1 + 2 * phi - 1 / np.sqrt(LD(np.pi)))
    terms = [d * d, np.abs(d), s * s, np.broadcast_to(np.log(v), d.shape), crps, (np.abs(s) <= LD(Z95)).astype(LD)]
    scores = np.stack([t.sum(axis=0) for t in terms], axis=1)
    sabs = np.stack([np.abs(t).sum(axis=0) for t in terms], axis=1)
    return dict(mean=Z - d, var=v[:, 0], s=s, scores=scores, sabs=sabs, margin=np.abs(np.abs(s) - LD(Z95)).min())


def loo_ld(F, Z):
    Z = _cols(Z)
    return loo_from(Z, apply_Tt(F, apply_T(F, Z)), qdiag(F, Z.shape[0]))


def spd_inv_ld(S):
    S = np.asarray(S, dtype=LD)
    n = S.shape[0]
    Rm = np.zeros_like(S)
    for j in range(n):
        d = S[j, j] - (Rm[j, :j] * Rm[j, :j]).sum()
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite")
        Rm[j, j] = np.sqrt(d)
        if j + 1 < n:
            Rm[j + 1:, j] = (S[j + 1:, j] - (Rm[j + 1:, :j] * Rm[j, :j]).sum(axis=1)) / Rm[j, j]
    y = np.zeros_like(S)
    eye = np.eye(n, dtype=LD)
    for i in range(n):
        y[i] = (eye[i] - (Rm[i, :i, None] * y[:i]).sum(axis=0)) / Rm[i, i]
    return y.T @ y


def dense_loo(locs, z, covmodel, cp, tau):
    """leave-one-out mean and variance of the exact Gaussian process: from inv(C + tau I), long double"""
    locs = np.asarray(locs, dtype=np.float64).astype(LD)
    n = locs.shape[0]
    C, _ = _cov_and_derivs(_dist(locs), covmodel, [LD(v) for v in cp])
    Q = spd_inv_ld(C + np.diag(np.broadcast_to(np.asarray(tau, dtype=np.float64), (n,)).astype(LD)))
    z = np.asarray(z, dtype=np.float64).astype(LD)
    q = np.diag(Q)
    return z - (Q @ z) / q, 1 / q


def index_py(nn, rowid, n):
    """nn [rows][P] internal positions, valid entries right-aligned, -1 = missing, own point last; rowid [rows] output rows.
    Returns (colptr, owner, col): flat offsets = output row * P + left-aligned slot, columns ascending in stored-set order,
    the own entry of the FIRST set that ends in a position in owner, of every further one in the position's column."""
    nn = np.asarray(nn)
    rows, P = nn.shape
    owner = [-1] * n
    cols = [[] for _ in range(n)]
    for s in range(rows):
        miss = int((nn[s] < 0).sum())
        for q in range(miss, P):
            off = int(rowid[s]) * P + (q - miss)
            i = int(nn[s, q])
            if q == P - 1 and owner[i] < 0:
                owner[i] = off
            else:
                cols[i].append(off)
    colptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    col = np.array([o for c in cols for o in c], dtype=np.int32)
    return colptr, np.array(owner, dtype=np.int32), col
