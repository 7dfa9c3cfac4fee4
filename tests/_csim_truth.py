"""Truth for the conditional simulation of a map under the cond.yz='z' model (gpv_plan_cond_sim), restated in numpy, holding no
product code.

The model.  The prediction locations s_0 .. s_{nq-1} come after all observations, in the order given (the sweep order).  s_i
conditions on N_i, the m nearest points among {the eligible observations} u {s_j : j < i}: its observations J_i through z (the
nugget on the diagonal), its earlier prediction locations P_i through the latent y (no nugget).  With s_i as the LAST row,
    S = C(N_i u s_i, N_i u s_i) + diag(tau_J, 0_P, 0),   u = S^-1 e_last,
    c_ij = -u_j / u_last,   sd_i = 1 / sqrt(u_last),   y_i = sum_J c_ij z_j + sum_P c_ip y_p + sd_i eps_i.

The search.  Ids: 1 .. n an observation, n + 1 + p the sweep row p; 0 = none.  Distances in the arithmetic of tests/_nn_truth.py
(ssq + df*df coordinate by coordinate in float64, NumPy's sqrt), on the coordinates divided by `scale` when given; ascending
distance, ties to the lower id; a point at a NaN or infinite distance never enters a list.

The solve.  A square-root-free Cholesky (L D L') over numpy.longdouble, the covariances of tests/_krige_truth.py: the pivots
d_j are the squares of the Cholesky pivots, and "a pivot not > 0, or u_last not > 0" is a failure.  It is written without the
square root for one reason: a location that coincides with an earlier prediction location of its list has a row of the same
bits, its multiplier is then exactly 1, the row cancels to exact zeros and the pivot is exactly 0 in ANY precision, so the set
of failed locations is a property of the input, not of the rounding.  A failed location is NaN in sd, a and coef; the
sequential substitution hands the NaN on to every location that depends on it.

  ordered_search      the lists, brute force
  levels              level(i) = 0 if P_i is empty else 1 + max level over P_i; (level, order, levptr)
  factor_ld           per location: coef (nq, m), sd (nq,), a (nq, R), failed (nq,); long double
  substitute          x_i = r_i + sum_P coef x_p, sequential, long double
  truth               mean, sd, failed and a function colouring standard normals into deviation fields
  dense_joint         the dense GP conditional mean and the lower Cholesky factor of the conditional covariance"""
import numpy as np

import _krige_truth as KT

LD = np.longdouble


def ordered_search(locs, qlocs, m, eligible=None, scale=None):
    """int32 (nq, m) ids of the definition"""
    locs = np.asarray(locs, dtype=np.float64)
    n, dim = locs.shape
    q = np.asarray(qlocs, dtype=np.float64).reshape(-1, dim)
    sc = np.ones(dim) if scale is None else np.asarray(scale, dtype=np.float64)
    el = np.ones(n, dtype=bool) if eligible is None else np.asarray(eligible).astype(bool)
    allp = np.vstack([locs, q]) / sc
    ok = np.concatenate([el, np.ones(q.shape[0], dtype=bool)])
    nq = q.shape[0]
    out = np.zeros((nq, m), dtype=np.int32)
    for i in range(nq):
        k = n + i
        ssq = np.zeros(k)
        with np.errstate(invalid="ignore", over="ignore"):
            for c in range(dim):
                df = allp[k, c] - allp[:k, c]
                ssq = ssq + df * df
            d = np.sqrt(ssq)
        d = np.where(ok[:k] & np.isfinite(d), d, np.inf)
        if k > 4 * m:                                                  # (the m smallest, ties included, before the full sort)
            cut = np.partition(d, m - 1)[m - 1]
            cand = np.flatnonzero(d <= cut)
        else:
            cand = np.arange(k)
        o = cand[np.lexsort((cand, d[cand]))][:m]
        o = o[np.isfinite(d[o])]
        out[i, : len(o)] = o + 1
    return out


def levels(NN, n):
    """(level (nq,), order (nq,), levptr (n_levels + 1,)) of a list; ValueError for an id outside [0, n + own row]"""
    NN = np.asarray(NN)
    nq = NN.shape[0]
    level = np.zeros(nq, dtype=np.int64)
    for i in range(nq):
        ids = NN[i]
        if (ids < 0).any() or (ids > n + i).any():
            raise ValueError("id outside [0, n + own row]")
        p = ids[ids > n] - n - 1
        level[i] = 0 if p.size == 0 else 1 + level[p].max()
    order = np.lexsort((np.arange(nq), level))
    nlev = int(level.max()) + 1 if nq else 0
    levptr = np.concatenate([[0], np.cumsum(np.bincount(level, minlength=nlev))]) if nq else np.zeros(1, dtype=np.int64)
    return level, order, levptr


def _last_row_ldl(S):
    """u = S^-1 e_last by S = L D L' (unit lower L), numpy.longdouble throughout; None when a pivot is not > 0"""
    S = S.copy()
    g = S.shape[0]
    Lm = np.eye(g, dtype=LD)
    d = np.zeros(g, dtype=LD)
    for j in range(g):
        d[j] = S[j, j]
        if not d[j] > 0:
            return None
        if j + 1 < g:
            l = S[j + 1:, j] / d[j]
            Lm[j + 1:, j] = l
            S[j + 1:, j:] = S[j + 1:, j:] - l[:, None] * S[j, j:][None, :]
    u = np.zeros(g, dtype=LD)                        # L y = e_last: y = e_last; D w = y; L' u = w from the bottom up
    u[g - 1] = 1 / d[g - 1]
    for j in range(g - 2, -1, -1):
        u[j] = -(Lm[j + 1:, j] @ u[j + 1:])
    return u if u[g - 1] > 0 else None


def factor_ld(locs, nuggets, Z, qlocs, NN, covmodel, cp):
    """coef (nq, m) long double: c_ij on the slots that hold a prediction location, 0 elsewhere; sd (nq,) long double;
    a (nq, R) long double: the sum over the observation slots; failed (nq,) bool.  Failed rows are NaN."""
    locs = np.asarray(locs, dtype=np.float64)
    n = locs.shape[0]
    q = np.asarray(qlocs, dtype=np.float64).reshape(-1, locs.shape[1])
    Z = np.asarray(Z, dtype=np.float64)
    Z = Z[:, None] if Z.ndim == 1 else Z
    tau = np.broadcast_to(np.asarray(nuggets, dtype=np.float64), (n,))
    nq, m = NN.shape
    allp = np.vstack([locs, q])
    coef = np.zeros((nq, m), dtype=LD)
    sd = np.zeros(nq, dtype=LD)
    a = np.zeros((nq, Z.shape[1]), dtype=LD)
    failed = np.zeros(nq, dtype=bool)
    for i in range(nq):
        slots = np.flatnonzero(NN[i] > 0)
        ids = NN[i][slots].astype(np.int64) - 1
        assert (ids < n + i).all()
        obs = ids < n
        x = np.vstack([allp[ids], q[i][None, :]]).astype(LD)
        S = KT.cov_matrix(x, covmodel, cp) + np.diag(np.concatenate([np.where(obs, tau[np.minimum(ids, n - 1)], 0.0), [0.0]]).astype(LD))
        u = _last_row_ldl(S) if np.all(np.isfinite(np.asarray(S, dtype=np.float64))) else None
        if u is None:
            failed[i] = True
            coef[i], sd[i], a[i] = np.nan, np.nan, np.nan
            continue
        c = -u[:-1] / u[-1]
        coef[i, slots[~obs]] = c[~obs]
        a[i] = c[obs] @ Z[ids[obs]].astype(LD)
        sd[i] = 1 / np.sqrt(u[-1])
    return coef, sd, a, failed


def substitute(NN, coef, R, n):
    """X (nq, k) long double: x_i = r_i + sum over the slots with an id > n of coef[i, t] x[id - n - 1], in sweep order"""
    R = np.asarray(R, dtype=LD)
    X = np.zeros_like(R)
    for i in range(R.shape[0]):
        t = np.flatnonzero(NN[i] > n)
        X[i] = R[i] + (coef[i, t] @ X[NN[i][t].astype(np.int64) - n - 1] if t.size else 0)
    return X


def truth(locs, nuggets, Z, qlocs, NN, covmodel, cp):
    """dict(mean (nq, R) float64, sd (nq,) float64, failed (nq,), nan (nq,): the locations whose mean is NaN,
    colour(E (nq, k)) -> dev (nq, k) float64, coef, a)"""
    n = np.asarray(locs).shape[0]
    coef, sd, a, failed = factor_ld(locs, nuggets, Z, qlocs, NN, covmodel, cp)
    mean = substitute(NN, coef, a, n)

    def colour(E):
        return np.asarray(substitute(NN, coef, sd[:, None] * np.asarray(E, dtype=LD), n), dtype=np.float64)
    mean64 = np.asarray(mean, dtype=np.float64)
    return dict(mean=mean64, sd=np.asarray(sd, dtype=np.float64), failed=failed, nan=np.isnan(mean64[:, 0]), colour=colour,
                coef=coef, a=a)


# ---- the inputs the CPU and the GPU tests share ---------------------------------------------------------------------------------
def exact_case():
    """n = 40 observations, nq = 24 locations: m = 63 = n + nq - 1 conditions every location on everything before it"""
    rng = np.random.default_rng(41)
    return dict(locs=rng.random((40, 2)), Z=rng.standard_normal((40, 2)), q=rng.random((24, 2)), tau=0.1, covmodel="matern",
                cp=[1.0, 0.3, 1.5], m=63)


def wide_case():
    """n = 2000 observations, 20 000 uniform locations in the order given, m = 2: a few levels, most of them wider than 256"""
    rng = np.random.default_rng(0)
    return dict(locs=rng.random((2000, 2)), Z=rng.standard_normal(2000), q=rng.random((20000, 2)), m=2)


def deep_case():
    """n = 400 observations, a 40 x 40 raster swept in a random order, m = 30: many levels, all narrow"""
    rng = np.random.default_rng(1)
    g = (np.arange(40) + 0.5) / 40
    q = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    return dict(locs=rng.random((400, 2)), Z=rng.standard_normal(400), q=q[rng.permutation(1600)], m=30)


def _chol_ld(A):
    g = A.shape[0]
    Lc = np.zeros((g, g), dtype=LD)
    for j in range(g):
        d = A[j, j] - Lc[j, :j] @ Lc[j, :j]
        assert d > 0
        Lc[j, j] = np.sqrt(d)
        Lc[j + 1:, j] = (A[j + 1:, j] - Lc[j + 1:, :j] @ Lc[j, :j]) / Lc[j, j]
    return Lc


def _solve_lower(Lc, B):
    X = np.zeros_like(B)
    for j in range(Lc.shape[0]):
        X[j] = (B[j] - Lc[j, :j] @ X[:j]) / Lc[j, j]
    return X


def dense_joint(locs, nuggets, Z, qlocs, covmodel, cp):
    """(mean (nq, R), F (nq, nq)): K_po (K_oo + tau)^-1 z and the lower Cholesky factor of K_pp - K_po (K_oo + tau)^-1 K_op, in the
    order of qlocs; long double, returned as float64"""
    locs = np.asarray(locs, dtype=np.float64)
    n = locs.shape[0]
    q = np.asarray(qlocs, dtype=np.float64).reshape(-1, locs.shape[1])
    Z = np.asarray(Z, dtype=np.float64)
    Z = Z[:, None] if Z.ndim == 1 else Z
    tau = np.broadcast_to(np.asarray(nuggets, dtype=np.float64), (n,)).astype(LD)
    C = KT.cov_matrix(np.vstack([locs, q]).astype(LD), covmodel, cp)
    Lo = _chol_ld(C[:n, :n] + np.diag(tau))
    W = _solve_lower(Lo, C[:n, n:])                                    # Lo^-1 K_op
    mean = W.T @ _solve_lower(Lo, Z.astype(LD))
    F = _chol_ld(C[n:, n:] - W.T @ W)
    return np.asarray(mean, dtype=np.float64), np.asarray(F, dtype=np.float64)
