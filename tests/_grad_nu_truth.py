"""Truth for the gradient and the expected Fisher information of the cond.yz='z' Vecchia log-likelihood under the general-nu Matern
covariance, smoothness included.  Holds no product code.

    C(r) = sigma^2 c_nu s^nu K_nu(s),   s = r / rho,   c_nu = 2^(1 - nu) / Gamma(nu)            (no sqrt(2 nu) scaling)
    dC/dsigma^2 = C / sigma^2,   dC/drho = sigma^2 c_nu s^(nu+1) K_(nu-1)(s) / rho,   dC/dnu: the derivative of the line above in nu

Two levels:
  mp_funcs       the per-function adjudicator: mpmath at 40 digits, besselk, and mpmath.diff IN THE ORDER for the smoothness
                 derivative (nothing of the formula for dK_nu/dnu is restated there)
  pair_funcs     the bulk truth for whole plans, numpy float64: scipy.special.kve for K_nu and K_(nu-1), and an own trapezoidal
                 quadrature of dK_nu(x)/dnu = int_0^inf exp(-x cosh t) t sinh(nu t) dt
  rows_f64 / fisher_rows_f64 feed pair_funcs into _grad_truth._terms and the definition in _fisher_truth through their `dmats`;
  row_adj does the same for ONE row with mp_funcs for every pair and the long-double Cholesky of _grad_truth.

The bulk truth is pinned to mpmath on the seeded sample of `sample_s` x SAMPLE_NU (2100 (nu, s) points: pair distances of the GPU
tests' seeded locations over their three ranges, plus s from 1e-10 to 800).  Measured gap, absolute with sigma^2 = rho = 1
(tests/test_loglik_grad_nu_host.py::test_bulk_truth_pinned_to_mpmath prints and asserts it):
    value 2.2e-14   range derivative 2.8e-14   smoothness derivative 4.7e-14
The first two are scipy's K_nu (~5e-14 relative near s = 2); the third adds the cancellation of C (ln s - ln 2 - psi) against
c_nu s^nu dK/dnu at small s, two terms of size ~ln(1/s).  PIN = 5e-13, ten times the measured figure, is asserted.  What matters
for the GPU tests is the rows: there the bulk truth has to stay below 1e-12 max(|row|, 1), 1e-4 of the 1e-8 row bar, and every
GPU test asserts that again on the rows it adjudicates with row_adj (_F64_VS_ADJ; measured there: <= 2e-13).

A departure from the issue that asked for this file: it names a LONG-DOUBLE quadrature of dK_nu/dnu; `_dk_dnu_scaled` is float64.
The quadrature's terms all have one sign, so float64 summation costs a few ulp, far below scipy's K_nu beside it, which bounds
the bulk truth either way; the gap to mpmath is measured and asserted as above instead of being assumed from the number format."""
import functools

import numpy as np

import _fisher_truth as F
import _grad_truth as T

PIN = 5e-13
NCOLS = 5                  # {l_k, d/d variance, d/d range, d/d smoothness, d/d nugget}
NTRI = 10


# ---- the adjudicator ------------------------------------------------------------------------------------------------------------
def mp_funcs(nu, s, dps=40):
    """(C, rho dC/drho, dC/dnu) at sigma^2 = 1 as mpmath numbers; s = 0: (1, 0, 0)"""
    import mpmath as mp
    with mp.workdps(dps):
        nu, s = mp.mpf(float(nu)), mp.mpf(float(s))
        if s == 0:
            return mp.mpf(1), mp.mpf(0), mp.mpf(0)

        def c(v):
            return mp.power(2, 1 - v) / mp.gamma(v) * mp.power(s, v) * mp.besselk(v, s)
        f0 = c(nu)
        f1 = mp.power(2, 1 - nu) / mp.gamma(nu) * mp.power(s, nu + 1) * mp.besselk(nu - 1, s)
        f2 = mp.diff(c, nu)
        return f0, f1, f2


# ---- the bulk truth -------------------------------------------------------------------------------------------------------------
def _dk_dnu_scaled(x, nu):
    """e^x dK_nu(x)/dnu for an array x > 0, float64: the trapezoidal rule on t_j = j h with the weights exp(-x (cosh t - 1)).  The
    integrand is entire and decays doubly exponentially; pushed to Im t = d the rule's error is exp(x (1 - cos d) - 2 pi d / h)
    relative, below 1e-19 for h <= pi^2 / (x + 50) (d = pi / 2) and for h <= 0.6 / sqrt(x) (d = 2 pi / (h x)).  Arguments are
    binned by size so that each bin shares one step."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    edges = [0.0, 6.0, 56.0, 746.0]                                # (beyond: e^-x is 0 in float64, the callers return zeros)
    for lo, hi in zip(edges[:-1], edges[1:]):
        sel = (x > lo) & (x <= hi)
        if not sel.any():
            continue
        xs = x[sel]
        xhi, xlo = xs.max(), xs.min()
        h = min(np.pi ** 2 / (xhi + 50.0), 0.6 / np.sqrt(xhi))
        acc = np.zeros_like(xs)
        j = 0
        while True:
            j += 1
            t = j * h
            q = 2.0 * np.sinh(0.5 * t) ** 2                       # cosh t - 1
            if xlo * q > 745.0:
                break
            term = (t * np.sinh(nu * t)) * np.exp(-xs * q)
            acc += term
            if j > 8 and np.all(term <= 1e-20 * acc):
                break
        out[sel] = h * acc
    return out


def pair_funcs(s, nu):
    """(C, rho dC/drho, dC/dnu) at sigma^2 = 1 for an array s >= 0, float64; s = 0: (1, 0, 0)"""
    from scipy.special import digamma, gammaln, kve
    s = np.asarray(s, dtype=np.float64)
    f0, f1, f2 = np.ones_like(s), np.zeros_like(s), np.zeros_like(s)
    pos = s > 0
    x = s[pos]
    lnc = (1.0 - nu) * np.log(2.0) - gammaln(nu)
    with np.errstate(under="ignore"):
        e = np.exp(lnc + nu * np.log(x) - x)                      # c_nu s^nu e^-s
        v0 = e * kve(nu, x)
        f0[pos] = v0
        f1[pos] = e * x * kve(abs(nu - 1.0), x)
        f2[pos] = v0 * (np.log(x) - np.log(2.0) - digamma(nu)) + e * _dk_dnu_scaled(x, nu)
    dead = pos & (s > 745.0)                                      # e^-s underflows: exact zeros, never 0 * inf
    f0[dead] = f1[dead] = f2[dead] = 0.0
    for f in (f0, f1, f2):                                        # nothing subnormal reaches the matrix products (numpy's BLAS
        f[np.abs(f) < 1e-280] = 0.0                               # returned 2^-31 for a product of subnormal entries)
    return f0, f1, f2


def cov_and_derivs(r, cp, funcs=pair_funcs):
    """C(r) and [dC/dsigma^2, dC/drho, dC/dnu] for cp = (sigma^2, rho, nu)"""
    s2, rho, nu = float(cp[0]), float(cp[1]), float(cp[2])
    f0, f1, f2 = funcs(np.asarray(r) / rho, nu)
    return s2 * f0, [f0, s2 * f1 / rho, s2 * f2]


def _groups(revNN):
    return F._groups(revNN)


def rows_f64(locsord, revNN, z_ord, cp, tau):
    """(n, 5) float64: every row of the plan, {l_k, d/d variance, d/d range, d/d smoothness, d/d nugget}"""
    locsord = np.asarray(locsord, dtype=np.float64)
    z_ord = np.asarray(z_ord, dtype=np.float64)
    out = np.full((np.asarray(revNN).shape[0], NCOLS), np.nan)
    for g, rows, idx in _groups(revNN):
        x, zJ = locsord[idx], z_ord[idx]
        C, dC = cov_and_derivs(T._dist(x), cp)
        S = C + tau * np.eye(g)
        e = np.zeros(g)
        e[-1] = 1.0
        rhs = np.stack([np.broadcast_to(e, zJ.shape), zJ], axis=-1)
        sol = np.linalg.solve(S, rhs)
        ell, d = T._terms(sol[..., 0], sol[..., 1], zJ, dC + [None])
        out[rows] = np.stack([ell] + d, axis=-1)
    return out


def fisher_rows_f64(locsord, revNN, cp, tau):
    """(n, 10) float64: the upper triangle of every row's information over {variance, range, smoothness, nugget}, by the definition
    of _fisher_truth (half traces of the block minus those of its leading block)"""
    locsord = np.asarray(locsord, dtype=np.float64)
    out = np.full((np.asarray(revNN).shape[0], NTRI), np.nan)
    for g, rows, idx in _groups(revNN):
        x = locsord[idx]
        C, dC = cov_and_derivs(T._dist(x), cp)
        eye = np.broadcast_to(np.eye(g), C.shape)
        S, D = C + tau * eye, list(dC) + [eye + np.zeros_like(C)]
        Fm = F._half_traces(np.linalg.inv(S), D)
        if g > 1:
            Fm = Fm - F._half_traces(np.linalg.inv(S[..., :-1, :-1]), [d[..., :-1, :-1] for d in D])
        out[rows] = F.tri(Fm)
    return out


def fisher_rows_form_f64(locsord, revNN, cp, tau):
    """(n, 10) float64: every row by t_i'y_j / u_last - 1/2 a_i a_j / u_last^2 (_fisher_truth.rows_form_f64).  The definition
    subtracts two traces; where a pair of NEIGHBOURS lies much closer than the range while the row's own point is far from all of
    them (range 1e-4 in the tests) both are ~1e6 and float64 leaves 1e-10 of a row whose true entries are ~0.  This form has no such
    difference; the adjudicator (row_adj, the definition in long double) ties the two together on the rows it takes."""
    locsord = np.asarray(locsord, dtype=np.float64)
    out = np.full((np.asarray(revNN).shape[0], NTRI), np.nan)
    for g, rows, idx in _groups(revNN):
        x = locsord[idx]
        C, dC = cov_and_derivs(T._dist(x), cp)
        eye = np.broadcast_to(np.eye(g), C.shape)
        S, D = C + tau * eye, list(dC) + [eye + np.zeros_like(C)]
        e = np.zeros((len(rows), g, 1))
        e[:, -1, 0] = 1.0
        u = np.linalg.solve(S, e)
        t = np.concatenate([d @ u for d in D], axis=-1)
        y = np.linalg.solve(S, t)
        ul = u[:, -1, 0]
        a = (u * t).sum(axis=1)
        Fm = np.swapaxes(t, -1, -2) @ y / ul[:, None, None] - 0.5 * a[:, :, None] * a[:, None, :] / (ul * ul)[:, None, None]
        out[rows] = F.tri(Fm)
    return out


def full_rows_f64(locsord, revNN, z_ord, cp, tau, form=False):
    fi = fisher_rows_form_f64 if form else fisher_rows_f64
    return np.concatenate([rows_f64(locsord, revNN, z_ord, cp, tau), fi(locsord, revNN, cp, tau)], axis=1)


def row_adj(locsord, revNN_row, z_ord, cp, tau):
    """(15,) numpy.longdouble: one row, {l_k, derivatives, information triangle}, every pair function from mpmath (rounded to long
    double), the solves by the long-double Cholesky of _grad_truth"""
    import mpmath as mp
    idx = T.valid_entries(revNN_row)
    x = np.asarray(locsord, dtype=np.float64)[idx].astype(np.longdouble)
    zJ = np.asarray(z_ord, dtype=np.float64)[idx].astype(np.longdouble)
    g = len(idx)
    r = T._dist(x)
    s2, rho, nu = (np.longdouble(v) for v in cp)
    Fs = np.zeros((3, g, g), dtype=np.longdouble)
    with mp.workdps(40):
        for i in range(g):
            for j in range(i + 1):
                vals = mp_funcs(cp[2], float(r[i, j] / rho))
                for q in range(3):                                  # mpf -> long double through two doubles
                    hi = float(vals[q])
                    Fs[q, i, j] = Fs[q, j, i] = np.longdouble(hi) + np.longdouble(float(vals[q] - mp.mpf(hi)))
    eye = np.eye(g, dtype=np.longdouble)
    S = s2 * Fs[0] + np.longdouble(tau) * eye
    D = [Fs[0], s2 * Fs[1] / rho, s2 * Fs[2], eye]
    rhs = np.zeros((g, 2), dtype=np.longdouble)
    rhs[-1, 0] = 1
    rhs[:, 1] = zJ
    sol = T._chol_solve_ld(S, rhs)
    ell, d = T._terms(sol[:, 0], sol[:, 1], zJ, D[:3] + [None])

    def traces(S_, D_):
        A = [T._chol_solve_ld(S_, np.array(d_)) for d_ in D_]
        return np.array([[(A[i] * A[j].T).sum() / 2 for j in range(4)] for i in range(4)], dtype=np.longdouble)
    Fm = traces(S, D)
    if g > 1:
        Fm = Fm - traces(S[:-1, :-1], [d_[:-1, :-1] for d_ in D])
    return np.concatenate([np.array([ell] + d, dtype=np.longdouble), F.tri(Fm)])


def scaled_row_error(got, want):
    """max over rows of |got - want|_inf / max(|want|_inf, 1); both must be finite"""
    got, want = np.atleast_2d(np.asarray(got, dtype=np.float64)), np.atleast_2d(np.asarray(want, dtype=np.float64))
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)), "non-finite entries"
    return np.abs(got - want).max(axis=1) / np.maximum(np.abs(want).max(axis=1), 1.0)


# ---- the seeded sample ------------------------------------------------------------------------------------------------------------
SAMPLE_NU = (0.3, 0.8, 1.2, 2.2, 4.7, 1.5 * (1 + 2.0 ** -30))      # (the host test adds 30)


@functools.lru_cache(maxsize=None)
def sample_s():
    """350 arguments: pair distances of the GPU tests' seeded locations (seed 11, n = 600, d = 2: each point against its ten nearest
    predecessors) divided by the tests' three ranges 0.25, 1e-4 and 50, and 50 values from 1e-10 to 800"""
    rng = np.random.default_rng(11)
    locs = rng.random((600, 2))
    pick = np.random.default_rng(23)
    d = []
    for i in pick.choice(np.arange(11, 600), 100, replace=False):
        dist = np.sqrt(((locs[:i] - locs[i]) ** 2).sum(axis=1))
        d.append(np.sort(dist)[:10][pick.integers(10)])
    d = np.array(d)
    grid = np.concatenate([10.0 ** np.linspace(-10, 2, 37), [3.9, 4.0, 17.0, 55.0, 200.0, 400.0, 511.0, 512.0, 600.0, 700.0, 744.0,
                                                              746.0, 800.0]])
    s = np.concatenate([d / 0.25, d / 1e-4, d / 50.0, grid])
    assert s.size == 350
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def sample_truth(nu):
    """(350, 3) float64 nearest to the mpmath values at sample_s(), and the same as long double for differences"""
    import mpmath as mp
    out = np.zeros((sample_s().size, 3), dtype=np.longdouble)
    with mp.workdps(40):
        for i, s in enumerate(sample_s()):
            vals = mp_funcs(nu, s)
            for q in range(3):
                hi = float(vals[q])
                out[i, q] = np.longdouble(hi) + np.longdouble(float(vals[q] - mp.mpf(hi)))
    out.setflags(write=False)
    return out
