"""Truth for local kriging under the cond.yz='z' model (gpv_find_query_nn, gpv_plan_krige), restated in numpy, holding no product
code.

The search.  For a query q the min(m, #eligible) eligible points closest to q by ascending
    d = sqrt(ssq),   ssq accumulated coordinate by coordinate as ssq + df*df in float64
(the arithmetic of tests/_nn_truth.py: NumPy's sqrt, products and sums are correctly rounded and nothing is fused), ties to the
lower index; 1-based, 0-padded.  A point at a NaN or infinite distance never enters a list.

The prediction.  With the valid neighbours J of a query and the query itself as the LAST row,
    S = C(J u q, J u q) + diag(tau_J, 0),   u = S^-1 e_last,
    var_y = 1 / u_last,   mean_c = -(sum_{j in J} u_j z_{j,c}) / u_last,
by a hand-written Cholesky over numpy.longdouble (the manner of tests/_grad_truth.py); a pivot that is not > 0 is a failure.
The covariances are evaluated in long double from long-double distances for the closed forms; at a general smoothness the
Bessel function is scipy's (float64, relative error ~1e-15: seven digits below the bar it adjudicates).

  query_nn            the search definition, brute force
  cov_matrix          C over a set of points: 'matern' (any smoothness), 'esqe', 'matern_scaledim'
  krige_ld            per-query kriging: mean (nq, R), var (nq,), l1 = ||u_J / u_last||_1 (nq,), failed (nq,)
  dense_conditional   the dense GP conditional mean and variance (what m = n must equal)
  log_density         log N(z0; mean, var)"""
import numpy as np

LD = np.longdouble


def query_nn(locs, qlocs, m, eligible=None):
    """int32 (nq, m): the array of the definition."""
    locs = np.asarray(locs, dtype=np.float64)
    q = np.asarray(qlocs, dtype=np.float64).reshape(-1, locs.shape[1])
    n = locs.shape[0]
    el = np.ones(n, dtype=bool) if eligible is None else np.asarray(eligible).astype(bool)
    out = np.zeros((q.shape[0], m), dtype=np.int32)
    for k in range(q.shape[0]):
        ssq = np.zeros(n)
        with np.errstate(invalid="ignore", over="ignore"):                     # (Inf - Inf: the non-finite inputs)
            for c in range(locs.shape[1]):
                df = q[k, c] - locs[:, c]
                ssq = ssq + df * df
            d = np.sqrt(ssq)
        d = np.where(el & np.isfinite(d), d, np.inf)
        o = np.lexsort((np.arange(n), d))[: min(m, n)]
        o = o[np.isfinite(d[o])]
        out[k, : len(o)] = o + 1
    return out


def _matern(r, s2, rho, nu):
    """sigma^2-scaled Matern of the library at distance r (any float dtype): closed forms at 0.5, 1.5, 2.5, else the Bessel
    branch WITHOUT the sqrt(2 nu) scaling of the distance (the reference's, reproduced)."""
    ft = r.dtype.type
    s2, rho = ft(s2), ft(rho)
    if nu == 0.5:
        return s2 * np.exp(-r / rho)
    if nu == 1.5:
        t = np.sqrt(ft(3)) * r / rho
        return s2 * (1 + t) * np.exp(-t)
    if nu == 2.5:
        t = np.sqrt(ft(5)) * r / rho
        return s2 * (1 + t + t * t / 3) * np.exp(-t)
    from scipy.special import gamma, kv
    s = np.asarray(r / rho, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        v = s ** nu * kv(nu, s) / (2.0 ** (nu - 1) * gamma(nu))
    return s2 * np.where(s == 0, 1.0, v).astype(r.dtype)


def cov_matrix(x, covmodel, cp):
    """C over the points x (g, dim), in x's dtype; distances summed over the coordinates in order."""
    ft = x.dtype.type
    g, dim = x.shape
    if covmodel == "matern_scaledim":
        assert len(cp) == dim + 2
        rng = [ft(v) for v in cp[1:1 + dim]]
    else:
        rng = [ft(1)] * dim
    r2 = np.zeros((g, g), dtype=x.dtype)
    for t in range(dim):
        df = (x[:, None, t] - x[None, :, t]) / rng[t]
        r2 = r2 + df * df
    r = np.sqrt(r2)
    if covmodel == "matern":
        return _matern(r, cp[0], cp[1], float(cp[2]))
    if covmodel == "matern_scaledim":
        return _matern(r, cp[0], 1.0, float(cp[dim + 1]))
    if covmodel == "esqe":
        s1, r1, s2, r2_ = (ft(v) for v in cp)
        return s1 * np.exp(-r / r1) + s2 * np.exp(-(r / r2_) ** 2)
    raise ValueError(covmodel)


def _last_row_of_inverse(S):
    """u = S^-1 e_last by a hand-written Cholesky, numpy.longdouble throughout; None when a pivot is not > 0"""
    g = S.shape[0]
    Lc = np.zeros((g, g), dtype=LD)
    for j in range(g):
        d = S[j, j] - Lc[j, :j] @ Lc[j, :j]
        if not d > 0:
            return None
        Lc[j, j] = np.sqrt(d)
        Lc[j + 1:, j] = (S[j + 1:, j] - Lc[j + 1:, :j] @ Lc[j, :j]) / Lc[j, j]
    u = np.zeros(g, dtype=LD)                        # L y = e_last: y = e_last / L_gg; then L' u = y from the bottom up
    u[g - 1] = 1 / (Lc[g - 1, g - 1] * Lc[g - 1, g - 1])
    for j in range(g - 2, -1, -1):
        u[j] = -(Lc[j + 1:, j] @ u[j + 1:]) / Lc[j, j]
    return u


def krige_ld(locs, nuggets, Z, qlocs, NN, covmodel, cp):
    """locs (n, dim), nuggets scalar or (n,), Z (n,) or (n, R), qlocs (nq, dim), NN (nq, m) 1-based with 0 = none.
    Returns float64 mean (nq, R), var (nq,), l1 (nq,), failed (nq,) bool; failed rows are NaN."""
    locs = np.asarray(locs, dtype=np.float64)
    q = np.asarray(qlocs, dtype=np.float64).reshape(-1, locs.shape[1])
    Z = np.asarray(Z, dtype=np.float64)
    Z = Z[:, None] if Z.ndim == 1 else Z
    tau = np.broadcast_to(np.asarray(nuggets, dtype=np.float64), (locs.shape[0],))
    nq = q.shape[0]
    mean, var, l1 = np.full((nq, Z.shape[1]), np.nan), np.full(nq, np.nan), np.full(nq, np.nan)
    failed = np.zeros(nq, dtype=bool)
    for k in range(nq):
        J = NN[k][NN[k] > 0].astype(np.int64) - 1
        x = np.vstack([locs[J], q[k][None, :]]).astype(LD)
        S = cov_matrix(x, covmodel, cp) + np.diag(np.concatenate([tau[J], [0.0]]).astype(LD))
        u = _last_row_of_inverse(S) if np.all(np.isfinite(np.asarray(S, dtype=np.float64))) else None
        if u is None:
            failed[k] = True
            continue
        w = u[:-1] / u[-1]
        mean[k] = np.asarray(-(w @ Z[J].astype(LD)), dtype=np.float64)
        var[k] = float(1 / u[-1])
        l1[k] = float(np.abs(w).sum())
    return mean, var, l1, failed


def dense_conditional(locs, nuggets, Z, qlocs, covmodel, cp):
    """The GP conditional of the latent field at each query given ALL observations, long double: mean (nq, R), var (nq,)."""
    locs = np.asarray(locs, dtype=np.float64)
    q = np.asarray(qlocs, dtype=np.float64).reshape(-1, locs.shape[1])
    Z = np.asarray(Z, dtype=np.float64)
    Z = Z[:, None] if Z.ndim == 1 else Z
    n = locs.shape[0]
    NN = np.tile(np.arange(1, n + 1, dtype=np.int32), (q.shape[0], 1))
    mean, var, _, failed = krige_ld(locs, nuggets, Z, q, NN, covmodel, cp)
    assert not failed.any()
    return mean, var


def dense_conditional_f64(locs, nuggets, Z, qlocs, covmodel, cp):
    """The same by the textbook formulas in float64 (numpy.linalg.solve): mean = k'K^-1 z, var = c0 - k'K^-1 k."""
    locs = np.asarray(locs, dtype=np.float64)
    q = np.asarray(qlocs, dtype=np.float64).reshape(-1, locs.shape[1])
    Z = np.asarray(Z, dtype=np.float64)
    Z = Z[:, None] if Z.ndim == 1 else Z
    n = locs.shape[0]
    tau = np.broadcast_to(np.asarray(nuggets, dtype=np.float64), (n,))
    C = cov_matrix(np.vstack([locs, q]), covmodel, cp)
    K = C[:n, :n] + np.diag(tau)
    k = C[:n, n:]
    sol = np.linalg.solve(K, np.hstack([Z, k]))
    mean = k.T @ sol[:, :Z.shape[1]]
    var = np.diag(C[n:, n:]) - np.einsum("ij,ij->j", k, sol[:, Z.shape[1]:])
    return mean, var


def log_density(z0, mean, var):
    """log N(z0; mean, var)"""
    return -0.5 * np.log(2 * np.pi * var) - 0.5 * (z0 - mean) ** 2 / var


# ---- the inputs the CPU and the GPU tests of the search share ----------------------------------------------------------------
def tie_grid():
    """a 12 x 12 regular grid (every distance ties with others) and queries on its points, cell centres and edges"""
    g = np.arange(12) / 8.0                                                   # (exactly representable: exact ties)
    locs = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    h = np.arange(23) / 16.0
    q = np.stack(np.meshgrid(h, h, indexing="ij"), axis=-1).reshape(-1, 2)
    return locs, q


def duplicated(n=300, dim=2, seed=5):
    """random points of which a third are copies of earlier ones; queries among them"""
    rng = np.random.default_rng(seed)
    locs = rng.random((n, dim))
    dup = rng.choice(n, n // 3, replace=False)
    locs[dup] = locs[rng.integers(0, n, dup.size)]
    return locs, rng.random((130, dim))


def on_points(n=300, dim=2, seed=6):
    """queries that coincide with observations"""
    rng = np.random.default_rng(seed)
    locs = rng.random((n, dim))
    return locs, locs[rng.choice(n, 130, replace=False)].copy()


def outside_box(n=300, dim=2, seed=7):
    """queries outside the bounding box of the observations: near, far, along one axis, in a corner"""
    rng = np.random.default_rng(seed)
    locs = rng.random((n, dim))
    q = rng.random((130, dim))
    side = rng.integers(0, 3, (130, dim))                                     # 0: inside along this axis, 1: below, 2: above
    side[side.sum(axis=1) == 0, 0] = 2
    far = 10.0 ** rng.integers(-3, 3, (130, 1))
    q = np.where(side == 1, -far * q, np.where(side == 2, 1.0 + far * q, q))
    return locs, q
