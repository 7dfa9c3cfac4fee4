"""Truth for the Vecchia colouring operator (gpv_plan_unwhiten, gpv_plan_simulate): the DEFINITION restated in numpy.longdouble,
holding no product code and never looking at Lentries.

For ordered row k with valid entries J (own point last), c = J without k and S = C(J, J) + diag(tau_J), the conditional law of
the own point given the others has weights w = S_cc^-1 S_ck and variance v = S_kk - S_kc S_cc^-1 S_ck, and a standard column e
colours, in the ordered row sequence, to
    b_k = sqrt(v) e_k + w . b_c.
Both come from the Cholesky factorisation S = R R' of tests/_whiten_truth.py applied to identity right-hand sides: the last row
of R^-1 gives w_c = -R_ll (R^-1)_lc, and v = R_ll^2.  Batched over the rows of equal length; the recursion is a plain loop.

  weights_ld    (idx (n, p) with -1 in front, w (n, p - 1) long double, sd (n,) long double) of a plan
  unwhiten_ld   B (n, c) long double from E (n, c)
  levels        level(k) = 0 without neighbours, else 1 + max_j level(j), from revNNarray alone
  levels_brute  the same by the definition as the longest chain below k, relaxed until nothing moves
  launches      how many launches a schedule takes: maximal runs of consecutive narrow levels plus the wide levels"""
import numpy as np

from _grad_truth import _cov_and_derivs, _dist
from _whiten_truth import _chol_forward_ld

LD = np.longdouble


def _rows(revNN):
    return np.nan_to_num(np.asarray(revNN, dtype=np.float64), nan=0.0).astype(np.int64)


def weights_ld(locsord, revNN, covmodel, cp, tau):
    locs = np.asarray(locsord, dtype=np.float64).astype(LD)
    nn = _rows(revNN)
    n, p = nn.shape
    tv = np.broadcast_to(np.asarray(tau, dtype=np.float64), (n,)).astype(LD)
    cpl = [LD(v) for v in cp]
    idx_all = np.full((n, p), -1, dtype=np.int64)
    w_all = np.zeros((n, max(p - 1, 1)), dtype=LD)
    sd = np.zeros(n, dtype=LD)
    n0 = (nn > 0).sum(axis=1)
    for g in np.unique(n0):
        rows = np.where(n0 == g)[0]
        idx = np.stack([nn[k][nn[k] > 0] - 1 for k in rows])
        C, _ = _cov_and_derivs(_dist(locs[idx]), covmodel, cpl)
        S = C + tv[idx][:, :, None] * np.eye(g, dtype=LD)
        eye = np.broadcast_to(np.eye(g, dtype=LD), (len(rows), g, g)).copy()
        last, rl = _chol_forward_ld(S, eye)                      # last: (rows, g) = the last row of R^-1
        idx_all[rows, p - g:] = idx
        if g > 1:
            w_all[rows, p - g:p - 1] = -rl[:, None] * last[:, :g - 1]
        sd[rows] = rl
    return idx_all, w_all, sd


def unwhiten_ld(locsord, revNN, E_ord, covmodel, cp, tau):
    """locsord (n, d); revNN (n, p) 1-based, 0 / NaN = missing, own point last; E_ord (n, c) ordered columns; tau a constant or
    (n,) ordered nuggets.  Returns B (n, c) in numpy.longdouble."""
    idx, w, sd = weights_ld(locsord, revNN, covmodel, cp, tau)
    E = np.asarray(E_ord, dtype=np.float64)
    E = (E[:, None] if E.ndim == 1 else E).astype(LD)
    n, p = idx.shape
    B = np.zeros_like(E)
    first = (idx >= 0).argmax(axis=1)
    for k in range(n):
        b = sd[k] * E[k]
        f = first[k]
        if f < p - 1:
            b = b + w[k, f:p - 1] @ B[idx[k, f:p - 1]]
        B[idx[k, p - 1]] = b
    return B


def levels(revNN):
    """level of every ROW.  Where every row ends in a point of its own this is the definition and nothing else.  A row whose
    last entry is a point that an earlier row has read or written (the nearest-neighbour search can name a coincident earlier
    point as a row's last entry) overwrites that point's value in the ordered row sequence, so it also comes after every such
    row: its level exceeds theirs."""
    nn = _rows(revNN)
    n, p = nn.shape
    wrote = np.full(n, -1, dtype=np.int64)                      # level of the row that wrote a point last
    touch = np.full(n, -1, dtype=np.int64)                      # highest level of a row that read or wrote it
    lev = np.zeros(n, dtype=np.int64)
    for k in range(n):
        j = nn[k, :p - 1]
        j = j[j > 0] - 1
        own = nn[k, p - 1] - 1
        lev[k] = max(touch[own] + 1, 0 if j.size == 0 else 1 + wrote[j].max())
        touch[j] = np.maximum(touch[j], lev[k])
        wrote[own] = touch[own] = lev[k]
    return lev


def levels_brute(revNN):
    nn = _rows(revNN)
    n, p = nn.shape
    lev = np.zeros(n, dtype=np.int64)
    while True:
        new = lev.copy()
        for k in range(n):
            for j in nn[k, :p - 1]:
                if j > 0:
                    new[nn[k, p - 1] - 1] = max(new[nn[k, p - 1] - 1], lev[j - 1] + 1)
        if np.array_equal(new, lev):
            return lev
        lev = new


def launches(lev, narrow):
    width = np.bincount(lev)
    is_narrow = width <= narrow
    runs = int(is_narrow[0]) + int(np.sum(is_narrow[1:] & ~is_narrow[:-1]))
    return int(len(width)), runs + int(np.sum(~is_narrow))
