"""Truth for the Vecchia whitening operator (gpv_plan_whiten): the DEFINITION restated in numpy.longdouble, holding no product
code and never looking at Lentries.

For ordered row k with valid entries J (own point last) and S = C(J, J) + diag(tau_J), the whitened value of a column b is the
standardised conditional residual of the own point given the others,
    e_k(b) = (b_k - S_kc S_cc^-1 b_c) / sqrt(S_kk - S_kc S_cc^-1 S_ck),        c = J without k,
and the row's log term is the logarithm of that conditional variance.  With the own point last both are the last entries of
the Cholesky factorisation S = R R': e_k(b) = (R^-1 b_J)_last, variance = R_last,last^2.  The Cholesky and the substitution are
written out here over numpy.longdouble, batched over the rows of equal length.

  whiten_ld     E (n, c) and the log terms (n,) of a plan, long double
  dense_gram    B'(C + tau I)^-1 B and log det(C + tau I), dense, long double (what m = n - 1 must equal)
  dense_gls     the dense GLS profile (beta_hat, beta_cov, quadform, logdet, loglik), float64 from the long-double pieces"""
import numpy as np

from _grad_truth import _cov_and_derivs, _dist

LD = np.longdouble


def _chol_forward_ld(S, rhs):
    """S: (r, g, g), rhs: (r, g, c), long double.  Returns (last row of R^-1 rhs: (r, c), R_last,last: (r,))."""
    r, g, _ = S.shape
    Rm = np.zeros_like(S)
    for j in range(g):
        d = S[:, j, j] - (Rm[:, j, :j] * Rm[:, j, :j]).sum(axis=1)
        if not np.all(d > 0):
            raise np.linalg.LinAlgError("not positive definite")
        Rm[:, j, j] = np.sqrt(d)
        if j + 1 < g:
            Rm[:, j + 1:, j] = (S[:, j + 1:, j] - (Rm[:, j + 1:, :j] * Rm[:, None, j, :j]).sum(axis=2)) / Rm[:, j, j, None]
    y = np.zeros_like(rhs)
    for i in range(g):
        y[:, i] = (rhs[:, i] - (Rm[:, i, :i, None] * y[:, :i]).sum(axis=1)) / Rm[:, i, i, None]
    return y[:, g - 1], Rm[:, g - 1, g - 1]


def whiten_ld(locsord, revNN, B_ord, covmodel, cp, tau):
    """locsord (n, d); revNN (n, p) 1-based, 0 / NaN = missing, own point last; B_ord (n, c) ordered columns; tau a constant or
    (n,) ordered nuggets.  Returns (E (n, c), logterm (n,)) in numpy.longdouble."""
    locs = np.asarray(locsord, dtype=np.float64).astype(LD)
    B = np.asarray(B_ord, dtype=np.float64)
    B = (B[:, None] if B.ndim == 1 else B).astype(LD)
    nn = np.nan_to_num(np.asarray(revNN, dtype=np.float64), nan=0.0).astype(np.int64)
    n = nn.shape[0]
    tv = np.broadcast_to(np.asarray(tau, dtype=np.float64), (n,)).astype(LD)
    cpl = [LD(v) for v in cp]
    E = np.zeros((n, B.shape[1]), dtype=LD)
    logterm = np.zeros(n, dtype=LD)
    n0 = (nn > 0).sum(axis=1)
    for g in np.unique(n0):
        rows = np.where(n0 == g)[0]
        idx = np.stack([nn[k][nn[k] > 0] - 1 for k in rows])
        C, _ = _cov_and_derivs(_dist(locs[idx]), covmodel, cpl)
        S = C + tv[idx][:, :, None] * np.eye(g, dtype=LD)
        last, rl = _chol_forward_ld(S, B[idx])
        E[rows] = last
        logterm[rows] = 2 * np.log(rl)
    return E, logterm


def dense_gram(locs, B, covmodel, cp, tau):
    """B'(C + tau I)^-1 B and log det(C + tau I) in long double; locs and B in any one common order; tau constant or (n,)."""
    locs = np.asarray(locs, dtype=np.float64).astype(LD)
    B = np.asarray(B, dtype=np.float64)
    B = (B[:, None] if B.ndim == 1 else B).astype(LD)
    n = locs.shape[0]
    C, _ = _cov_and_derivs(_dist(locs), covmodel, [LD(v) for v in cp])
    S = C + np.diag(np.broadcast_to(np.asarray(tau, dtype=np.float64), (n,)).astype(LD))
    Rm = np.zeros_like(S)
    for j in range(n):
        d = S[j, j] - (Rm[j, :j] * Rm[j, :j]).sum()
        Rm[j, j] = np.sqrt(d)
        if j + 1 < n:
            Rm[j + 1:, j] = (S[j + 1:, j] - (Rm[j + 1:, :j] * Rm[j, :j]).sum(axis=1)) / Rm[j, j]
    y = np.zeros_like(B)
    for i in range(n):
        y[i] = (B[i] - (Rm[i, :i, None] * y[:i]).sum(axis=0)) / Rm[i, i]
    return y.T @ y, 2 * np.log(np.diag(Rm)).sum()


def profile_from(G, logdet, n):
    """the profile algebra once more, in numpy alone: G the Gram matrix of [X | z]"""
    G = np.asarray(G, dtype=np.float64)
    q = G.shape[0] - 1
    Ai = np.linalg.inv(G[:q, :q])
    beta = Ai @ G[:q, q]
    quad = G[q, q] - G[:q, q] @ beta
    return dict(beta_hat=beta, beta_cov=Ai, quadform=float(quad), logdet=float(logdet),
                loglik=float(-0.5 * logdet - 0.5 * quad - 0.5 * n * np.log(2 * np.pi)))


def dense_gls(locs, X, z, covmodel, cp, tau):
    G, logdet = dense_gram(locs, np.column_stack([X, z]), covmodel, cp, tau)
    return profile_from(G.astype(np.float64), float(logdet), len(z))
