"""Host side of the whitening feature (no GPU): the long-double truth of tests/_whiten_truth.py against dense algebra, the pure
profile algebra, the refusals that need no device, and vecchia_estimate(trend="ols") against the call without the argument."""
import ctypes as C

import numpy as np
import pytest

import _whiten_truth as W

CASES = {"nu0.5": ("matern", [1.3, 0.25, 0.5]), "nu1.5": ("matern", [1.3, 0.25, 1.5]), "nu2.5": ("matern", [1.3, 0.25, 2.5]),
         "esqe": ("esqe", [0.8, 0.25, 0.5, 0.2])}


def _full_rows(n):
    """revNNarray of m = n - 1 in the given order: row k holds 1 .. k + 1, own point last, missing entries (0) in front"""
    nn = np.zeros((n, n), dtype=np.int64)
    for k in range(n):
        nn[k, n - 1 - k:] = np.arange(1, k + 2)
    return nn


@pytest.mark.parametrize("vecnug", [False, True])
@pytest.mark.parametrize("fam", sorted(CASES))
def test_truth_equals_dense_precision_at_full_conditioning(fam, vecnug):
    """m = n - 1 (n = 60): E'E of the truth is B'(C + tau I)^-1 B, the log terms sum to log det, and beta_hat is dense GLS"""
    cm, cp = CASES[fam]
    rng = np.random.default_rng(1)
    n = 60
    locs = rng.random((n, 2))
    X = np.column_stack([np.ones(n), locs[:, 0]])
    z = X @ [1.0, -2.0] + rng.standard_normal(n)
    B = np.column_stack([X, z, rng.standard_normal((n, 2))])
    tau = rng.uniform(0.05, 0.3, n) if vecnug else 0.1
    E, logterm = W.whiten_ld(locs, _full_rows(n), B, cm, cp, tau)
    Gd, logdet = W.dense_gram(locs, B, cm, cp, tau)
    Gt = E.T @ E
    scale = np.abs(E).T @ np.abs(E)
    assert float((np.abs(Gt - Gd) / scale).max()) <= 1e-15                       # long double: 64-bit significand
    assert abs(float(logterm.sum() - logdet)) <= 1e-15 * float(np.abs(logterm).sum())
    # dense GLS in float64, the textbook way
    S = np.asarray(W._cov_and_derivs(W._dist(locs), cm, cp)[0]) + np.diag(np.broadcast_to(tau, (n,)))
    Si = np.linalg.inv(S)
    beta = np.linalg.solve(X.T @ Si @ X, X.T @ Si @ z)
    prof = W.profile_from(Gt[:3, :3].astype(np.float64), float(logterm.sum()), n)
    assert np.allclose(prof["beta_hat"], beta, rtol=1e-9, atol=0)
    r = z - X @ beta
    assert np.isclose(prof["quadform"], r @ Si @ r, rtol=1e-9)
    assert np.isclose(prof["logdet"], np.linalg.slogdet(S)[1], rtol=1e-12)


def test_profile_algebra_against_numpy():
    import gpvecchia_amd as G
    rng = np.random.default_rng(3)
    for q in (1, 2, 5, 15):
        M = rng.standard_normal((40, q + 1))
        Gm = M.T @ M + 0.1 * np.eye(q + 1)
        logdet, n = 12.5, 40
        got = G.profile_from_gram(Gm, logdet, n)
        A, b, s = Gm[:q, :q], Gm[:q, q], Gm[q, q]
        beta = np.linalg.lstsq(A, b, rcond=None)[0]
        assert np.allclose(got["beta_hat"], beta, rtol=1e-9, atol=1e-12)
        assert np.allclose(got["beta_cov"], np.linalg.inv(A), rtol=1e-9, atol=1e-12) and np.array_equal(got["beta_cov"], got["beta_cov"].T)
        assert np.isclose(got["quadform"], s - b @ beta, rtol=1e-10)
        # the Schur complement: quadform = 1 / (G^-1)[q, q]
        assert np.isclose(got["quadform"], 1.0 / np.linalg.inv(Gm)[q, q], rtol=1e-9)
        assert got["logdet"] == logdet
        assert np.isclose(got["loglik"], -0.5 * logdet - 0.5 * got["quadform"] - 0.5 * n * np.log(2 * np.pi), rtol=1e-14)
        ref = W.profile_from(Gm, logdet, n)
        assert np.allclose(got["beta_hat"], ref["beta_hat"], rtol=1e-9) and np.isclose(got["loglik"], ref["loglik"], rtol=1e-12)


def test_profile_algebra_refuses_a_singular_trend():
    import gpvecchia_amd as G
    rng = np.random.default_rng(4)
    M = rng.standard_normal((30, 3))
    M = np.column_stack([M[:, 0], 2.0 * M[:, 0], M[:, 2]])                       # collinear trend columns
    with pytest.raises(ValueError):
        G.profile_from_gram(M.T @ M, 1.0, 30)
    with pytest.raises(ValueError):
        G.profile_from_gram(np.zeros((3, 3)), 1.0, 30)
    with pytest.raises(ValueError):
        G.profile_from_gram(np.full((2, 2), np.nan), 1.0, 30)
    with pytest.raises(ValueError):
        G.profile_from_gram(np.ones((1, 1)), 1.0, 30)                            # no trend column


def test_symbols_are_exported():
    from gpvecchia_amd import _lib
    assert "gpv_plan_whiten" in _lib.EXPORTS and "gpv_whiten_max_cols" in _lib.EXPORTS
    assert _lib.lib().gpv_whiten_max_cols() == 16
    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "gpvecchia.h")).read()
    assert "int gpv_plan_whiten(" in header and "int gpv_whiten_max_cols(void);" in header


def test_null_arguments_are_bad_arguments():
    from gpvecchia_amd import _lib
    B, Gm = np.zeros(4), np.zeros(1)
    ld, nf = C.c_double(0), C.c_int64(0)
    assert _lib.lib().gpv_plan_whiten(None, _lib.dptr(B), 4, 1, None, 0, _lib.dptr(Gm), C.byref(ld), C.byref(nf)) == 2


def test_python_layer_refusals_without_a_device():
    import gpvecchia_amd as G
    rng = np.random.default_rng(0)
    n = 50
    locs, z = rng.random((n, 2)), rng.standard_normal(n)
    X16 = rng.standard_normal((n, 16))
    vz = G.vecchia_specify(locs, 5, cond_yz="z", nn_backend="host")
    with pytest.raises(ValueError, match="at most 15"):
        G.vecchia_profile_likelihood(z, X16, vz, [1.0, 0.1, 1.5], 0.1)            # q + 1 > 16
    with pytest.raises(ValueError):
        G.vecchia_profile_likelihood(z, X16[:-1, :2], vz, [1.0, 0.1, 1.5], 0.1)   # rows do not match
    zn = z.copy()
    zn[3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        G.vecchia_profile_likelihood(zn, X16[:, :2], vz, [1.0, 0.1, 1.5], 0.1)
    with pytest.raises(ValueError, match="NaN"):
        G.vecchia_likelihood_replicates(np.column_stack([z, zn]), vz, [1.0, 0.1, 1.5], 0.1)
    with pytest.raises(ValueError):
        G.vecchia_whiten(z[:-1], vz, [1.0, 0.1, 1.5], 0.1)
    vs = G.vecchia_specify(locs, 5, cond_yz="SGV", nn_backend="host")
    for call in (lambda: G.vecchia_whiten(z, vs, [1.0, 0.1, 1.5], 0.1),
                 lambda: G.vecchia_profile_likelihood(z, X16[:, :2], vs, [1.0, 0.1, 1.5], 0.1),
                 lambda: G.vecchia_likelihood_replicates(z, vs, [1.0, 0.1, 1.5], 0.1)):
        with pytest.raises(ValueError, match="cond_yz='z'"):
            call()
    with pytest.raises(ValueError, match="named covariance"):
        G.vecchia_whiten(z, vz, [1.0, 0.1, 1.5], 0.1, covmodel=np.eye(n))
    with pytest.raises(ValueError, match="nuggets"):
        G.vecchia_whiten(z, vz, [1.0, 0.1, 1.5], np.full(n - 1, 0.1))
    # vecchia_estimate(trend=...)
    with pytest.raises(ValueError, match="trend"):
        G.vecchia_estimate(z, locs, m=5, trend="wls", cond_yz="z", output_level=0)
    with pytest.raises(ValueError, match="cond_yz='z'"):
        G.vecchia_estimate(z, locs, m=5, trend="gls", output_level=0)
    with pytest.raises(ValueError, match="needs a trend"):
        G.vecchia_estimate(z, locs, X=None, m=5, trend="gls", cond_yz="z", output_level=0)


@pytest.mark.parametrize("method", ["Nelder-Mead", "L-BFGS-B", "fisher"])
@pytest.mark.parametrize("xkind", ["missing", "none", "given"])
def test_estimate_trend_ols_is_the_call_without_the_argument(monkeypatch, method, xkind):
    """on a stubbed likelihood (a smooth function of the parameters and of the data it is handed)"""
    import gpvecchia_amd as G
    from gpvecchia_amd import api as A
    rng = np.random.default_rng(5)
    n = 80
    locs = rng.random((n, 2))
    Xm = np.column_stack([np.ones(n), locs[:, 0]])
    data = Xm @ [2.0, -1.5] + rng.standard_normal(n)
    target = np.log([1.4, 0.2, 0.3])

    def parts(z, cp, nug):
        th = np.array([cp[0], cp[1], nug])
        d = np.log(th) - target
        ll = -0.5 * float(z @ z) / len(z) - float(d @ d) - 0.3 * float(d[0] * d[1])
        g = -(2 * d + 0.3 * np.array([d[1], d[0], 0.0])) / th
        info = (2 * np.eye(3) + 0.3 * np.array([[0, 1, 0], [1, 0, 0], [0, 0, 0]])) / np.outer(th, th)
        full = lambda v: np.array([v[0], v[1], np.nan, v[2]])                     # noqa: E731
        info4 = np.full((4, 4), np.nan)
        info4[np.ix_([0, 1, 3], [0, 1, 3])] = info
        return ll, full(g), info4

    monkeypatch.setattr(A, "vecchia_likelihood", lambda z, va, cp, nug, covmodel="matern", device=0: parts(z, cp, nug)[0])
    monkeypatch.setattr(A, "vecchia_likelihood_grad", lambda z, va, cp, nug, covmodel="matern", device=0: parts(z, cp, nug)[:2])
    monkeypatch.setattr(A, "vecchia_likelihood_fisher", lambda z, va, cp, nug, covmodel="matern", device=0: parts(z, cp, nug))
    X = {"missing": "missing", "none": None, "given": Xm}[xkind]
    kw = dict(X=X, m=5, cond_yz="z", output_level=0, smoothness=1.5, method=method, nn_backend="host")
    a = G.vecchia_estimate(data, locs, **kw)
    b = G.vecchia_estimate(data, locs, trend="ols", **kw)
    assert sorted(a) == sorted(b) and "beta_cov" not in a
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k], k
    assert a["trend"] == {"missing": "constant", "none": "none", "given": "userspecified"}[xkind]
    assert np.allclose(a["theta_hat"], np.exp(target), rtol=2e-2)
