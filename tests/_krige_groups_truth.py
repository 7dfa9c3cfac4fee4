"""Truth for grouped local kriging under the cond.yz='z' model (gpv_plan_krige_groups), restated in numpy, holding no product code.

The model.  A group G of g locations x_0 .. x_{g-1} with weights w (default 1 / g):
    anchor   a = the coordinate-wise mean of the members in float64: s = x_0; s += x_i in member order; s / g, nothing fused
    J        the min(m, #eligible) eligible observations nearest to the anchor (tests/_krige_truth.py query_nn; on the
             coordinates divided by `scale` when given), or given
    S        C(J u G, J u G) + diag(tau_J, 0_G), J in front
    Sigma_G  K_GG - K_GJ (K_JJ + tau_J)^-1 K_JG,   mean = K_GJ (K_JJ + tau_J)^-1 z_J
by a hand-written Cholesky of K_JJ + tau_J over numpy.longdouble; the covariances in long double (tests/_krige_truth.py
cov_matrix).  A group fails when a pivot of K_JJ + tau_J is not > 0 or a diagonal entry of Sigma_G is not > 0.

  anchors          the anchors of the groups, (ngroups, dim) float64
  group_nn         J per group: int32 (ngroups, m), 1-based, 0-padded
  krige_groups_ld  per group: dict(mean (g, R), cov (g, g), l1 (g,), failed) in float64 from long double
  scales           the five error scales of the bar, per group, from the truth
  log_density_mv   log N(x; mean, Sigma) in float64 (numpy.linalg), for the chain rule"""
import numpy as np

from _krige_truth import cov_matrix, query_nn

LD = np.longdouble


def anchors(qlocs, gptr):
    q = np.asarray(qlocs, dtype=np.float64)
    out = np.empty((len(gptr) - 1, q.shape[1]))
    for k in range(len(gptr) - 1):
        s = q[gptr[k]].copy()
        for i in range(gptr[k] + 1, gptr[k + 1]):
            s = s + q[i]
        out[k] = s / float(gptr[k + 1] - gptr[k])
    return out


def group_nn(locs, qlocs, gptr, m, eligible=None, scale=None):
    a = anchors(qlocs, gptr)
    locs = np.asarray(locs, dtype=np.float64)
    if scale is not None:
        sc = np.asarray(scale, dtype=np.float64)
        return query_nn(locs / sc, a / sc, m, eligible=eligible)
    return query_nn(locs, a, m, eligible=eligible)


def _chol_ld(K):
    """lower Cholesky factor, numpy.longdouble throughout; None when a pivot is not > 0"""
    g = K.shape[0]
    Lc = np.zeros((g, g), dtype=LD)
    for j in range(g):
        d = K[j, j] - Lc[j, :j] @ Lc[j, :j]
        if not d > 0:
            return None
        Lc[j, j] = np.sqrt(d)
        Lc[j + 1:, j] = (K[j + 1:, j] - Lc[j + 1:, :j] @ Lc[j, :j]) / Lc[j, j]
    return Lc


def _fwd(Lc, B):
    """L^-1 B by forward substitution in long double"""
    Y = np.array(B, dtype=LD)
    for j in range(Lc.shape[0]):
        Y[j] = (Y[j] - Lc[j, :j] @ Y[:j]) / Lc[j, j]
    return Y


def _bwd(Lc, B):
    """L^-T B by backward substitution in long double"""
    Y = np.array(B, dtype=LD)
    for j in range(Lc.shape[0] - 1, -1, -1):
        Y[j] = (Y[j] - Lc[j + 1:, j] @ Y[j + 1:]) / Lc[j, j]
    return Y


def krige_groups_ld(locs, nuggets, Z, qlocs, gptr, NN, covmodel, cp):
    """locs (n, dim), nuggets scalar or (n,), Z (n,) or (n, R), qlocs (nq, dim) with the members of a group contiguous,
    gptr (ngroups + 1,), NN (ngroups, m) 1-based with 0 = none.  Returns a list with one dict per group:
    mean (g, R), cov (g, g), l1 (g,): ||K_iJ (K_JJ + tau)^-1||_1, failed; everything of a failed group is NaN."""
    locs = np.asarray(locs, dtype=np.float64)
    q = np.asarray(qlocs, dtype=np.float64).reshape(-1, locs.shape[1])
    Z = np.asarray(Z, dtype=np.float64)
    Z = Z[:, None] if Z.ndim == 1 else Z
    tau = np.broadcast_to(np.asarray(nuggets, dtype=np.float64), (locs.shape[0],))
    out = []
    for k in range(len(gptr) - 1):
        x = q[gptr[k]:gptr[k + 1]]
        g = x.shape[0]
        J = NN[k][NN[k] > 0].astype(np.int64) - 1
        nj = J.size
        C = cov_matrix(np.vstack([locs[J], x]).astype(LD), covmodel, cp)
        bad = dict(mean=np.full((g, Z.shape[1]), np.nan), cov=np.full((g, g), np.nan), l1=np.full(g, np.nan), failed=True)
        if not np.all(np.isfinite(np.asarray(C, dtype=np.float64))):
            out.append(bad)
            continue
        if nj:
            Lc = _chol_ld(C[:nj, :nj] + np.diag(tau[J].astype(LD)))
            if Lc is None:
                out.append(bad)
                continue
            W = _bwd(Lc, _fwd(Lc, C[:nj, nj:])).T                     # (g, nj): K_GJ (K_JJ + tau)^-1
            Y = _fwd(Lc, C[:nj, nj:])
            Sig = C[nj:, nj:] - Y.T @ Y
            mean = W @ Z[J].astype(LD)
        else:
            W = np.zeros((g, 0), dtype=LD)
            Sig = C
            mean = np.zeros((g, Z.shape[1]), dtype=LD)
        if not np.all(np.diag(Sig) > 0):
            out.append(bad)
            continue
        out.append(dict(mean=np.asarray(mean, dtype=np.float64), cov=np.asarray(Sig, dtype=np.float64),
                        l1=np.asarray(np.abs(W).sum(axis=1), dtype=np.float64), failed=False))
    return out


def scales(t, w, zmax):
    """the scales the bar is relative to, from a group's truth t and its weights w: mean (g, 1), var (g,), cov (g, g), gmean, gvar"""
    sd = np.sqrt(np.diag(t["cov"]))
    return dict(mean=(t["l1"] * zmax)[:, None], var=np.diag(t["cov"]), cov=np.outer(sd, sd), gmean=float(np.abs(w) @ t["l1"]) * zmax,
                gvar=float(np.abs(w) @ sd) ** 2)


def log_density_mv(x, mean, Sigma):
    """log N(x; mean, Sigma), float64"""
    x, mean = np.asarray(x, dtype=np.float64), np.asarray(mean, dtype=np.float64)
    Lc = np.linalg.cholesky(Sigma)
    y = np.linalg.solve(Lc, x - mean)
    return float(-0.5 * x.size * np.log(2 * np.pi) - np.log(np.diag(Lc)).sum() - 0.5 * y @ y)
