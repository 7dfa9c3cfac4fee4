"""Dense numpy restatement of the Takahashi recursion behind gpv_plan_selinv (gpv_selinv.hip), for the tests.

W = R R^T with R upper triangular; column c of R holds the rows N(c) = {i < c: pattern[i, c]} and itself.  With Sigma = W^-1,
Sigma R = R^-T (lower triangular, diagonal 1 / R_cc) gives, column by column in ascending order,

    Sigma_ic = -(1 / R_cc) sum_{k in N(c)} Sigma_ik R_kc            i in N(c)
    Sigma_cc = 1 / R_cc^2 - (1 / R_cc) sum_{k in N(c)} Sigma_ck R_kc .

Sigma_ik, i < k both in N(c), is entry (i, k) of the pattern; where the pattern has no such entry the term is 0 (the zero-fill
rule) and the triple (i, k, c) is counted as dropped.  Nothing is dropped on a pattern that is closed under the factorisation's
fill, and the diagonal is then diag(W^-1) exactly."""
import numpy as np


def ul_cholesky(W):
    """R upper triangular with W = R R^T: the reversed lower Cholesky factor of the reversed matrix (R/vecchia_prediction.R:80)."""
    W = np.asarray(W, dtype=np.float64)
    return np.linalg.cholesky(W[::-1, ::-1])[::-1, ::-1]


def filled_pattern(pattern):
    """The pattern of the UL factor of a matrix whose upper triangle has `pattern`: symbolic elimination, last column first
    (eliminating column k couples every two of its rows)."""
    F = np.triu(np.asarray(pattern, dtype=bool)).copy()
    n = F.shape[0]
    F[np.arange(n), np.arange(n)] = True
    for k in range(n - 1, -1, -1):
        rows = np.where(F[:k, k])[0]
        if rows.size > 1:
            sub = F[np.ix_(rows, rows)]
            sub |= np.triu(np.ones((rows.size, rows.size), dtype=bool))
            F[np.ix_(rows, rows)] = sub
    return F


def selinv_truth(R, pattern):
    """(diag(Sigma), n_dropped) of the recursion on the structural `pattern` (boolean, its upper triangle is used, the diagonal
    counts as set) with the zero-fill rule.  Entries of R outside the pattern are ignored."""
    R = np.asarray(R, dtype=np.float64)
    n = R.shape[0]
    P = np.triu(np.asarray(pattern, dtype=bool)).copy()
    P[np.arange(n), np.arange(n)] = True
    Psym = P | P.T
    S = np.zeros((n, n))
    dropped = 0
    for c in range(n):
        N = np.where(P[:c, c])[0]
        rcc = R[c, c]
        if N.size == 0:
            S[c, c] = 1.0 / rcc ** 2
            continue
        r = R[N, c]
        inside = Psym[np.ix_(N, N)]
        dropped += int((~inside).sum()) // 2                         # every pair i < k once
        M = np.where(inside, S[np.ix_(N, N)], 0.0)
        sig = -(M @ r) / rcc
        S[N, c] = sig
        S[c, N] = sig
        S[c, c] = (1.0 / rcc - sig @ r) / rcc
    return np.diag(S).copy(), dropped


def latent_factor(U_obj):
    """(R, pattern) of an oracle createU result (dense U): for cond.yz = 'zy' R = B, the latent block itself; otherwise the UL
    Cholesky factor of W = U_y U_y^T.  The pattern is that of the latent block B."""
    U = np.asarray(U_obj["U"], dtype=np.float64)
    lat = np.asarray(U_obj["latent"], dtype=bool)
    B = U[np.ix_(lat, lat)]
    pattern = B != 0.0
    if U_obj["cond_yz"] == "zy":
        return B, pattern
    Uy = U[lat, :]
    return ul_cholesky(Uy @ Uy.T), pattern
