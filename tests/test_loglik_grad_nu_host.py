"""gpv_plan_loglik_grad_nu / gpv_plan_loglik_fisher_nu without a GPU: the exports, the pair functions of the general-nu Matern on
the host (gpv_matern_derivs_host) against 40-digit mpmath, the truth of the GPU tests (tests/_grad_nu_truth.py) against mpmath and
against the dense multivariate normal, and the Python layer's refusals.

Measured (the seeded sample of _grad_nu_truth.sample_s, 350 arguments from 1e-10 to 800 per smoothness; absolute, sigma^2 = 1,
range = 1):
  gpv_matern_derivs_host against mpmath, worst over nu in {0.3, 0.8, 1.2, 2.2, 4.7, 1.5 (1 + 2^-30), 30}:
      value 1.2e-14 (nu = 30; 2.0e-15 for the others)   range derivative 2.7e-15   smoothness derivative 9.5e-14
      (the last one at s ~ 0.25, just above where the cancellation-free form for small s ends: C (ln s - ln 2 - psi) against
      c_nu s^nu dK/dnu; below s = 0.25 the worst is 2e-15)
  HOST_BOUND = 9.5e-13 is ten times the worst figure.
  the bulk truth against mpmath, nu in the first six: value 2.2e-14  range derivative 2.8e-14  smoothness derivative 4.7e-14
      (scipy's K_nu is good to ~5e-14 relative near s = 2); _grad_nu_truth.PIN = 5e-13 is asserted."""
import ctypes as C

import numpy as np
import pytest

import _grad_nu_truth as N
import _grad_truth as T

TAU = 0.1
HOST_NU = N.SAMPLE_NU + (30.0,)
HOST_BOUND = 9.5e-13


def _host(nu, s, rng_=1.0):
    from gpvecchia_amd import _lib
    s = np.ascontiguousarray(s, dtype=np.float64)
    out = np.zeros((s.size, 3))
    st = _lib.lib().gpv_matern_derivs_host(float(nu), float(rng_), _lib.dptr(s), s.size, _lib.dptr(out))
    assert st == 0
    return out


def _rev_nn(locs, m):
    from oracle import r_side as R
    return np.nan_to_num(R.findOrderedNN(locs, m)[:, ::-1], nan=0.0).astype(np.int64)


def test_symbols_are_exported():
    from gpvecchia_amd import _lib
    import gpvecchia_amd as G
    for name in ("gpv_plan_loglik_grad_nu", "gpv_plan_loglik_fisher_nu", "gpv_matern_derivs_host"):
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib(), name) is not None
    import inspect
    for fn in (G.Plan.loglik_grad, G.Plan.loglik_fisher, G.vecchia_likelihood_grad, G.vecchia_likelihood_fisher, G.vecchia_estimate):
        assert inspect.signature(fn).parameters["smoothness_grad"].default is False


def test_argument_checks_before_the_device():
    from gpvecchia_amd import _lib
    L = _lib.lib()
    cp, grad, info = np.array([1.0, 0.1, 0.8]), np.zeros(4), np.zeros(16)
    ll, nf = C.c_double(), C.c_int64()
    assert L.gpv_plan_loglik_grad_nu(None, b"matern", _lib.dptr(cp), 3, 0.1, C.byref(ll), _lib.dptr(grad), C.byref(nf), None) == 2
    assert L.gpv_plan_loglik_fisher_nu(None, b"matern", _lib.dptr(cp), 3, 0.1, C.byref(ll), _lib.dptr(grad), _lib.dptr(info),
                                       C.byref(nf), None) == 2
    s, out = np.array([1.0]), np.zeros(3)
    assert L.gpv_matern_derivs_host(0.8, 1.0, None, 1, _lib.dptr(out)) == 2
    assert L.gpv_matern_derivs_host(0.8, 1.0, _lib.dptr(s), 1, None) == 2
    assert L.gpv_matern_derivs_host(0.8, 1.0, _lib.dptr(s), -1, _lib.dptr(out)) == 2
    assert L.gpv_matern_derivs_host(0.8, 0.0, _lib.dptr(s), 1, _lib.dptr(out)) == 2
    assert L.gpv_matern_derivs_host(0.0, 1.0, _lib.dptr(s), 1, _lib.dptr(out)) == 4
    assert L.gpv_matern_derivs_host(61.0, 1.0, _lib.dptr(s), 1, _lib.dptr(out)) == 4
    assert L.gpv_matern_derivs_host(float("nan"), 1.0, _lib.dptr(s), 1, _lib.dptr(out)) == 4
    assert L.gpv_matern_derivs_host(0.8, 1.0, None, 0, None) == 0


@pytest.mark.parametrize("nu", HOST_NU)
def test_host_functions_against_mpmath(nu):
    s = N.sample_s()
    got = _host(nu, s)
    want = N.sample_truth(nu)
    err = np.abs(got.astype(np.longdouble) - want).max(axis=0).astype(np.float64)
    print(f"nu = {nu!r}: value {err[0]:.2e}  range derivative {err[1]:.2e}  smoothness derivative {err[2]:.2e}")
    assert np.all(err <= HOST_BOUND), err
    # the range enters as 1 / range in the second function only
    assert np.array_equal(_host(nu, s, 4.0), got * np.array([1.0, 0.25, 1.0]))


@pytest.mark.parametrize("nu", HOST_NU)
def test_host_functions_finite_at_the_ends(nu):
    got = _host(nu, [800.0, 1e-10, 0.0, 746.0, 1e-30, 5e3])
    assert np.all(np.isfinite(got)), got
    assert np.array_equal(got[0], [0.0, 0.0, 0.0])                # e^-800 underflows: exact zeros
    assert np.array_equal(got[2], [1.0, 0.0, 0.0])                # r = 0


def test_bulk_truth_pinned_to_mpmath():
    s = N.sample_s()
    assert len(N.SAMPLE_NU) * s.size >= 2000
    worst = np.zeros(3)
    for nu in N.SAMPLE_NU:
        got = np.stack(N.pair_funcs(s, nu), axis=1)
        assert np.all(np.isfinite(got))
        worst = np.maximum(worst, np.abs(got.astype(np.longdouble) - N.sample_truth(nu)).max(axis=0).astype(np.float64))
    print(f"bulk truth against mpmath: value {worst[0]:.2e}  range derivative {worst[1]:.2e}  smoothness derivative {worst[2]:.2e}")
    assert np.all(worst <= N.PIN), worst


@pytest.mark.parametrize("nu", (0.3, 0.8, 2.2))
def test_truth_rows_sum_to_the_dense_mvn(nu):
    """m = n - 1: the Vecchia density IS the multivariate normal; its derivative in nu by mpmath differentiation of the dense
    log-density, the other three by the closed expressions -1/2 tr(S^-1 D) + 1/2 a'D a in long double."""
    import mpmath as mp
    rng = np.random.default_rng(1)
    n = 40
    locs, z = rng.random((n, 2)), rng.standard_normal(n)
    cp = [1.3, 0.25, nu]
    rows = N.rows_f64(locs, _rev_nn(locs, n - 1), z, cp, TAU)
    tot, scale = rows.sum(axis=0), np.abs(rows).sum(axis=0)
    r = T._dist(locs)

    with mp.workdps(30):
        rm = [[mp.mpf(float(r[i, j])) for j in range(n)] for i in range(n)]
        zm = mp.matrix([float(v) for v in z])

        def logdens(s2, rho, v, tau):
            cst = mp.power(2, 1 - v) / mp.gamma(v)
            S = mp.matrix(n, n)
            for i in range(n):
                S[i, i] = s2 + tau
                for j in range(i):
                    x = rm[i][j] / rho
                    S[i, j] = S[j, i] = s2 * cst * mp.power(x, v) * mp.besselk(v, x)
            Lc = mp.cholesky(S)
            y = mp.lu_solve(S, zm)
            return -sum(mp.log(Lc[i, i]) for i in range(n)) - (zm.T * y)[0] / 2 - n * mp.log(2 * mp.pi) / 2
        th = [mp.mpf(cp[0]), mp.mpf(cp[1]), mp.mpf(cp[2]), mp.mpf(TAU)]
        ll = logdens(*th)
        d_nu = mp.diff(lambda v: logdens(th[0], th[1], v, th[3]), th[2], h=mp.mpf("1e-10"))
    C_, dC = N.cov_and_derivs(r, cp)
    S = (C_ + TAU * np.eye(n)).astype(np.longdouble)
    rhs = np.concatenate([np.eye(n, dtype=np.longdouble), z.astype(np.longdouble)[:, None]], axis=1)
    sol = T._chol_solve_ld(S, rhs)
    Sinv, alpha = sol[:, :n], sol[:, n]
    g = [float(-0.5 * (Sinv * D).sum() + 0.5 * alpha @ D.astype(np.longdouble) @ alpha) for D in (dC[0], dC[1])]
    g_tau = float(-0.5 * np.trace(Sinv) + 0.5 * alpha @ alpha)
    want = np.array([float(ll), g[0], g[1], float(d_nu), g_tau])
    off = np.abs(tot - want) / scale
    print("value and gradient (variance, range, smoothness, nugget) off by", off, "of sum |term|")
    assert np.all(off <= 1e-10), (tot, want)


def test_python_layer_refusals():
    import gpvecchia_amd as G
    rng = np.random.default_rng(0)
    locs, z = rng.random((60, 2)), rng.standard_normal(60)
    # every existing refusal with smoothness_grad left at its default
    with pytest.raises(ValueError, match="smoothness"):
        G.vecchia_estimate(z, locs, m=5, method="L-BFGS-B", cond_yz="z", output_level=0)
    with pytest.raises(ValueError, match="smoothness"):
        G.vecchia_estimate(z, locs, m=5, method="L-BFGS-B", smoothness=0.8, cond_yz="z", output_level=0)
    with pytest.raises(ValueError, match="smoothness"):
        G.vecchia_estimate(z, locs, m=5, method="fisher", smoothness=0.8, cond_yz="z", output_level=0)
    with pytest.raises(ValueError, match="cond_yz"):
        G.vecchia_estimate(z, locs, m=5, method="L-BFGS-B", smoothness=1.5, output_level=0)
    with pytest.raises(ValueError, match="not defined"):
        G.vecchia_estimate(z, locs, m=5, method="BFGS", output_level=0)
    # the new ones
    with pytest.raises(ValueError, match="gls"):
        G.vecchia_estimate(z, locs, m=5, method="L-BFGS-B", smoothness_grad=True, trend="gls", cond_yz="z", output_level=0)
    with pytest.raises(ValueError, match="matern"):
        G.vecchia_estimate(z, locs, m=5, method="L-BFGS-B", smoothness_grad=True, covmodel="esqe", cond_yz="z", output_level=0,
                           theta_ini=[1.0, 0.1, 1.0, 0.1, 0.1])
    with pytest.raises(ValueError, match="cond_yz"):
        G.vecchia_estimate(z, locs, m=5, method="fisher", smoothness_grad=True, output_level=0)
    va_sgv = G.vecchia_specify(locs, 5, ordering="none", cond_yz="SGV", nn_backend="host")
    with pytest.raises(ValueError, match="cond_yz"):
        G.vecchia_likelihood_grad(z, va_sgv, [1.0, 0.2, 0.8], TAU, smoothness_grad=True)
    with pytest.raises(ValueError, match="cond_yz"):
        G.vecchia_likelihood_fisher(z, va_sgv, [1.0, 0.2, 0.8], TAU, smoothness_grad=True)


def test_nan_smoothness_derivative_names_another_start(monkeypatch):
    """A free smoothness sitting exactly on a closed form: the entries return NaN in its slot and the driver says what to do.  The
    likelihood call is replaced by its documented answer there (no device in this test)."""
    import gpvecchia_amd as G
    from gpvecchia_amd import wrappers as W
    rng = np.random.default_rng(0)
    locs, z = rng.random((60, 2)), rng.standard_normal(60)
    seen = []

    def grad_at_closed_form(z_, va, cp, nug, covmodel="matern", device=0, smoothness_grad=False):
        seen.append((float(cp[2]), smoothness_grad))
        return -80.0, np.array([0.1, -0.2, np.nan, 0.3])

    def fisher_at_closed_form(z_, va, cp, nug, covmodel="matern", device=0, smoothness_grad=False):
        seen.append((float(cp[2]), smoothness_grad))
        info = np.eye(4)
        info[2, :] = info[:, 2] = np.nan
        return -80.0, np.array([0.1, -0.2, np.nan, 0.3]), info
    monkeypatch.setattr(W.A, "vecchia_likelihood_grad", grad_at_closed_form)
    monkeypatch.setattr(W.A, "vecchia_likelihood_fisher", fisher_at_closed_form)
    kw = dict(m=5, cond_yz="z", output_level=0, smoothness_grad=True, theta_ini=[1.0, 0.2, 1.5, 0.1], nn_backend="host")
    for method in ("L-BFGS-B", "fisher"):
        with pytest.raises(ValueError, match="different starting value"):
            G.vecchia_estimate(z, locs, method=method, **kw)
    assert seen == [(1.5, True), (1.5, True)]


def test_fisher_scoring_rejects_a_step_past_the_smoothness_guard(monkeypatch):
    """Fisher scoring with a free smoothness keeps the reference's guard (smoothness in (0.01, 10], L-BFGS-B's box): a trial step
    past it is a rejected step that the halving loop shortens, never a call of the library nor an error out of the driver.  The
    likelihood call is replaced by a concave quadratic in the log-parameters whose maximum lies at smoothness 20 (no device in
    this test)."""
    import gpvecchia_amd as G
    from gpvecchia_amd import wrappers as W
    rng = np.random.default_rng(0)
    locs, z = rng.random((60, 2)), rng.standard_normal(60)
    target = np.log([1.0, 0.2, 20.0, 0.1])
    seen = []

    def fisher_quadratic(z_, va, cp, nug, covmodel="matern", device=0, smoothness_grad=False):
        th = np.concatenate([cp, [nug]])
        seen.append(float(cp[2]))
        e = target - np.log(th)
        return -100.0 - 0.5 * float(e @ e), e / th, np.eye(4) / np.outer(th, th)
    monkeypatch.setattr(W.A, "vecchia_likelihood_fisher", fisher_quadratic)
    est = G.vecchia_estimate(z, locs, m=5, method="fisher", cond_yz="z", output_level=0, smoothness_grad=True,
                             theta_ini=[1.0, 0.2, 8.0, 0.1], nn_backend="host", maxit=40)
    assert len(seen) > 1 and max(seen) <= 10.0
    assert 8.0 < est["theta_hat"][2] <= 10.0                          # it moved towards the maximum and stopped inside the guard
    assert est["n_evals"] > len(seen)                                 # rejected trial steps count as evaluations
    with pytest.raises(RuntimeError, match="initial parameters"):     # a start outside the guard is said so at once
        G.vecchia_estimate(z, locs, m=5, method="fisher", cond_yz="z", output_level=0, smoothness_grad=True,
                           theta_ini=[1.0, 0.2, 12.0, 0.1], nn_backend="host")
