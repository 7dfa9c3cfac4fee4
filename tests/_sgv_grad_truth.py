"""Truth for the analytic gradient of the Vecchia log-likelihood with latent conditioning (cond.yz='SGV'): a dense numpy
restatement that holds no product code, in the DIRECT form (one solve and one dM_p per parameter, dense W, dense W^-1 masked to
W's pattern), so that it shares nothing with the adjoint form of the kernel.

Set k with valid entries J (own point l last) and flags c_j (True: conditioned on as latent y, c_l True):
    S = C(J, J) + tau diag(1 - c),  u = S^-1 e_l,  M = u / sqrt(u_l),  a_k = sum_{c_j = 0} M_j z_j,  m_k = the latent part of M
    W = sum_k m_k m_k' + I / tau,  z2 = sum_k m_k a_k - z / tau,  mu~ = W^-1 z2,  Sigma = W^-1 on the pattern of W
    -2 l = n log 2 pi - 2 sum_k log M_kl + n log tau + log det W + sum_k a_k^2 + z'z / tau - z2'mu~
With D_p = dS/dtheta_p elementwise (the nugget: diag(1 - c)), y_p = S^-1 D_p u, dM_p = -y_p / sqrt(u_l) + 1/2 u (y_p)_l / u_l^{3/2},
da = sum_{c_j = 0} dM_j z_j, dm = the latent part of dM, s_k = m_k'mu~, the summands of column k of d(-2 l)/dtheta_p are
    -2 dM_l / M_l,   2 m_k' Sigma_LL dm,   2 a_k da,   -2 a_k dm'mu~,   -2 s_k da,   2 s_k dm'mu~
and for the nugget also 1/tau, -Sigma_kk/tau^2, -z_k^2/tau^2, -2 mu~_k z_k/tau^2, -mu~_k^2/tau^2.  col_terms[k] is -1/2 their sum,
scale[k] 1/2 the sum of their absolute values; the columns are laid out as the product's grad (covparms, then the nugget; NaN
for the smoothness of 'matern').

    sgv_truth(...)   -> dict(loglik, grad, col_terms, scale), in float64 or numpy.longdouble (hand-written Cholesky, as _grad_truth)
    sgv_value(...)   -> the value alone (for central differences)"""
import numpy as np

import _grad_truth as T


def _chol(S):
    g = S.shape[0]
    Lc = np.zeros((g, g), dtype=S.dtype)
    for j in range(g):
        d = S[j, j] - (Lc[j, :j] * Lc[j, :j]).sum()
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite")
        Lc[j, j] = np.sqrt(d)
        if j + 1 < g:
            Lc[j + 1:, j] = (S[j + 1:, j] - (Lc[j + 1:, :j] * Lc[j, :j]).sum(axis=1)) / Lc[j, j]
    return Lc


def _chol_solve(Lc, rhs):
    g = Lc.shape[0]
    y = np.zeros_like(rhs)
    for i in range(g):
        y[i] = (rhs[i] - (Lc[i, :i, None] * y[:i]).sum(axis=0)) / Lc[i, i]
    x = np.zeros_like(rhs)
    for i in range(g - 1, -1, -1):
        x[i] = (y[i] - (Lc[i + 1:, i, None] * x[i + 1:]).sum(axis=0)) / Lc[i, i]
    return x


def _sets(revNN, revCond):
    """per row: 0-based valid entries (own point last) and their latent flags (the LAST n0 entries of the cond row)"""
    out = []
    rc = np.nan_to_num(np.asarray(revCond, dtype=np.float64), nan=0.0)
    for k in range(np.asarray(revNN).shape[0]):
        idx = T.valid_entries(np.asarray(revNN)[k])
        c = rc[k][len(rc[k]) - len(idx):] > 0
        assert len(idx) > 0 and idx[-1] == k and c[-1], "the own point stands last and is latent"
        out.append((idx, c))
    return out


def _forward(locsord, sets, z, covmodel, cp, tau, ft, want_derivs):
    n = len(sets)
    one, half = ft(1), ft(0.5)
    W = np.zeros((n, n), dtype=ft)
    pattern = np.eye(n, dtype=bool)
    z2 = -z / tau
    per = []
    logM = ft(0)
    a2 = ft(0)
    for k, (idx, c) in enumerate(sets):
        x = np.asarray(locsord, dtype=np.float64)[idx].astype(ft)
        g = len(idx)
        Cm, dC = T._cov_and_derivs(T._dist(x), covmodel, [ft(v) for v in cp])
        obs = (~c).astype(ft)
        Lc = _chol(Cm + tau * np.diag(obs))
        e = np.zeros((g, 1), dtype=ft)
        e[-1, 0] = one
        u = _chol_solve(Lc, e)[:, 0]
        ul = u[-1]
        M = u / np.sqrt(ul)
        zJ = z[idx]
        a = (M * obs * zJ).sum()
        lat = idx[c]
        m = M[c]
        W[np.ix_(lat, lat)] += np.outer(m, m)
        pattern[np.ix_(lat, lat)] = True
        z2[lat] += m * a
        logM += np.log(M[-1])
        a2 += a * a
        dM = []
        if want_derivs:
            Du = np.stack([(D * u[None, :]).sum(-1) for D in dC] + [obs * u], axis=1)
            Y = _chol_solve(Lc, Du)
            for p in range(Y.shape[1]):
                dM.append(-Y[:, p] / np.sqrt(ul) + half * u * Y[-1, p] / (ul * np.sqrt(ul)))
        per.append((idx, c, M, a, dM))
    W[np.diag_indices(n)] += one / tau
    LW = _chol(W)
    mu = _chol_solve(LW, z2[:, None])[:, 0]
    logdetW = 2 * np.log(np.diag(LW)).sum()
    m2l = n * np.log(2 * ft(np.pi)) - 2 * logM + n * np.log(tau) + logdetW + a2 + (z * z).sum() / tau - (z2 * mu).sum()
    return -half * m2l, per, pattern, LW, mu


def sgv_value(locsord, revNN, revCond, z_ord, covmodel, cp, tau, dtype=np.float64):
    ft = np.dtype(dtype).type
    z = np.asarray(z_ord, dtype=np.float64).astype(ft)
    return _forward(locsord, _sets(revNN, revCond), z, covmodel, cp, ft(tau), ft, False)[0]


def sgv_truth(locsord, revNN, revCond, z_ord, covmodel, cp, tau, dtype=np.float64):
    ft = np.dtype(dtype).type
    tau = ft(tau)
    z = np.asarray(z_ord, dtype=np.float64).astype(ft)
    sets = _sets(revNN, revCond)
    n = len(sets)
    ll, per, pattern, LW, mu = _forward(locsord, sets, z, covmodel, cp, tau, ft, True)
    Sig = _chol_solve(LW, np.eye(n, dtype=ft))
    Sig = np.where(pattern, Sig, ft(0))                              # only what the selected inverse holds
    npar = len(per[0][4])
    terms = np.zeros((n, npar), dtype=ft)
    scale = np.zeros((n, npar), dtype=ft)
    for k, (idx, c, M, a, dM) in enumerate(per):
        lat = idx[c]
        obs = (~c).astype(ft)
        m = M[c]
        s = (m * mu[lat]).sum()
        Sm = Sig[np.ix_(lat, lat)] @ m
        for p in range(npar):
            dm = dM[p][c]
            da = (dM[p] * obs * z[idx]).sum()
            dmu = (dm * mu[lat]).sum()
            summ = [-2 * dM[p][-1] / M[-1], 2 * (Sm * dm).sum(), 2 * a * da, -2 * a * dmu, -2 * s * da, 2 * s * dmu]
            if p == npar - 1:
                t2 = tau * tau
                summ += [1 / tau, -Sig[k, k] / t2, -z[k] * z[k] / t2, -2 * mu[k] * z[k] / t2, -mu[k] * mu[k] / t2]
            terms[k, p] = -sum(summ) / 2
            scale[k, p] = sum(abs(v) for v in summ) / 2
    def spread(A):
        nan = np.full((n,), np.nan, dtype=ft)
        cols = [A[:, 0], A[:, 1], nan, A[:, 2]] if covmodel == "matern" else [A[:, p] for p in range(npar)]
        return np.stack(cols, axis=1)
    ct, sc = spread(terms), spread(scale)
    return dict(loglik=ll, grad=ct.sum(axis=0), col_terms=ct, scale=sc)
