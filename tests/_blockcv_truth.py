"""Truth for the leave-block-out cross-validation (gpv_plan_set_blocks / gpv_plan_block_cv): the DEFINITION restated in
numpy.longdouble, holding no product code and never looking at Lentries.

With T the whitening operator of tests/_loo_truth.py (factor_ld -> dense_T) and Q = T'T, a held-out block B of ordered rows has
    z_B | z_-B ~ N(z_B - Q_BB^-1 (Q z)_B, Q_BB^-1):
Q_BB is cut from the dense Q, inverted by the written-out Cholesky (spd_inv_ld), and its pivots come from the same recursion.

  blockcv_ld    mean, var, standardised residual (NaN where not held out), the eight score sums per column and the sums of
                their |terms|: [0] .. [5] the terms of _loo_truth.loo_from with this mean and variance over the held-out
                locations, [6] one term r_B' Q_BB^-1 r_B per block, [7] one term -log(pivot^2) per pivot of the factor of Q_BB
  chol_pivots   the diagonal of R, S = R R'
  index_py      the block index of a plan's index arrays, restated (gpv_blocks_index_host)
  exact_blocks  the same conditional of the exact Gaussian process, from C + tau I partitioned directly"""
import math

import numpy as np

import _loo_truth as T
from _grad_truth import _cov_and_derivs, _dist

LD = np.longdouble
Z95 = T.Z95


def chol_pivots(S):
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
    return np.diag(Rm).copy()


def block_lists(block_of):
    """the member lists (ascending ordered row) of the labels >= 0, in ascending label"""
    lab = np.asarray(block_of, dtype=np.int64)
    return [np.where(lab == b)[0] for b in np.unique(lab[lab >= 0])]


def from_Q(Q, Z, block_of):
    """the whole truth from a dense long-double precision matrix Q"""
    Z = T._cols(Z)
    n, nc = Z.shape
    r = Q @ Z
    mean, s = np.full((n, nc), np.nan, dtype=LD), np.full((n, nc), np.nan, dtype=LD)
    var = np.full(n, np.nan, dtype=LD)
    t6, t7 = [], []
    for B in block_lists(block_of):
        QBB = Q[np.ix_(B, B)]
        K = T.spd_inv_ld(QBB)
        delta = K @ r[B]
        mean[B] = Z[B] - delta
        var[B] = np.diag(K)
        s[B] = delta / np.sqrt(var[B])[:, None]
        t6.append((r[B] * delta).sum(axis=0))
        piv = chol_pivots(QBB)
        t7.extend(-np.log(piv * piv))
    held = ~np.isnan(var)
    d, v, sh = (Z - mean)[held], var[held][:, None], s[held]
    Phi2m1 = T._erf(sh.astype(np.float64) / math.sqrt(2.0)).astype(LD)
    phi = np.exp(-sh * sh / 2) / np.sqrt(2 * LD(np.pi))
    crps = np.sqrt(v) * (sh * Phi2m1 + 2 * phi - 1 / np.sqrt(LD(np.pi)))
    t7 = np.broadcast_to(np.asarray(t7, dtype=LD)[:, None], (len(t7), nc))
    terms = [d * d, np.abs(d), sh * sh, np.broadcast_to(np.log(v), d.shape), crps, (np.abs(sh) <= LD(Z95)).astype(LD),
             np.stack(t6), t7]
    scores = np.stack([t.sum(axis=0) for t in terms], axis=1)
    sabs = np.stack([np.abs(t).sum(axis=0) for t in terms], axis=1)
    return dict(mean=mean, var=var, s=s, scores=scores, sabs=sabs, n_heldout=int(held.sum()),
                margin=np.abs(np.abs(sh) - LD(Z95)).min())


def precision_ld(F, n):
    Tm = T.dense_T(F, n)
    return Tm.T @ Tm


def blockcv_ld(F, Z, block_of):
    """F: the groups of _loo_truth.factor_ld; Z (n, c) ordered columns; block_of (n,) labels of the ORDERED rows, -1 = kept"""
    Z = T._cols(Z)
    return from_Q(precision_ld(F, Z.shape[0]), Z, block_of)


def exact_blocks(locs, z, covmodel, cp, tau, block_of):
    """block mean and variance of the exact Gaussian process, from S = C + tau I partitioned directly:
    E[z_B | z_R] = S_BR S_RR^-1 z_R, Var = diag(S_BB - S_BR S_RR^-1 S_RB), R the complement of B"""
    locs = np.asarray(locs, dtype=np.float64).astype(LD)
    n = locs.shape[0]
    C, _ = _cov_and_derivs(_dist(locs), covmodel, [LD(v) for v in cp])
    S = C + np.diag(np.broadcast_to(np.asarray(tau, dtype=np.float64), (n,)).astype(LD))
    z = np.asarray(z, dtype=np.float64).astype(LD)
    mean, var = np.full(n, np.nan, dtype=LD), np.full(n, np.nan, dtype=LD)
    for B in block_lists(block_of):
        rest = np.setdiff1d(np.arange(n), B)
        if rest.size == 0:
            mean[B], var[B] = 0, np.diag(S)[B]
            continue
        W = S[np.ix_(B, rest)] @ T.spd_inv_ld(S[np.ix_(rest, rest)])
        mean[B] = W @ z[rest]
        var[B] = np.diag(S[np.ix_(B, B)] - W @ S[np.ix_(rest, B)])
    return mean, var


def index_py(nn, rowid, n, newpos, block_of_ord):
    """nn [rows][P] internal positions, valid entries right-aligned, -1 = missing, own point last; newpos [n] the internal position
    of each ordered row (None: the identity); block_of_ord [n] labels.  Returns (memptr, members, setptr, sets, blkloc): blocks in
    ascending label with empty labels skipped, members in ascending ordered row as internal positions, per block the stored sets
    that hold at least one member (the own entry counts), ascending, and per internal position (block, local index) or (-1, -1)."""
    nn = np.asarray(nn)
    lab = np.asarray(block_of_ord, dtype=np.int64)
    pos = np.arange(n) if newpos is None else np.asarray(newpos, dtype=np.int64)
    members = [[int(pos[i]) for i in rows] for rows in block_lists(lab)]
    blkloc = np.full((n, 2), -1, dtype=np.int32)
    for b, mem in enumerate(members):
        for a, p in enumerate(mem):
            blkloc[p] = (b, a)
    sets = [[s for s in range(nn.shape[0]) if any(int(v) >= 0 and blkloc[int(v), 0] == b for v in nn[s])] for b in range(len(members))]
    memptr = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int32)
    setptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    return (memptr, np.array([p for m in members for p in m], dtype=np.int32), setptr,
            np.array([s for l in sets for s in l], dtype=np.int32), blkloc)
