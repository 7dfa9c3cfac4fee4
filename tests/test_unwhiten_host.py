"""Host side of the colouring / simulation feature (no GPU): the long-double truth of tests/_unwhiten_truth.py against dense
algebra and against the whitening truth, its level helper against the brute-force definition, the exported symbols, the C
entries' argument checks that come before a device is touched, and the refusals of the Python layer with their messages."""
import ctypes as C

import numpy as np
import pytest

import _unwhiten_truth as U
import _whiten_truth as W


def _full_rows(n):
    """revNNarray of m = n - 1 in the given order: row k holds 1 .. k + 1, own point last, missing entries (0) in front"""
    nn = np.zeros((n, n), dtype=np.int64)
    for k in range(n):
        nn[k, n - 1 - k:] = np.arange(1, k + 2)
    return nn


@pytest.mark.parametrize("vecnug", [False, True])
def test_truth_at_full_conditioning_is_the_cholesky_factor(vecnug):
    """m = n - 1 (n = 40): the colouring of the identity is the lower Cholesky factor of C + tau I"""
    rng = np.random.default_rng(1)
    n = 40
    locs = rng.random((n, 2))
    cm, cp = "matern", [1.3, 0.25, 1.5]
    tau = rng.uniform(0.05, 0.3, n) if vecnug else 0.1
    A = U.unwhiten_ld(locs, _full_rows(n), np.eye(n), cm, cp, tau).astype(np.float64)
    S = np.asarray(W._cov_and_derivs(W._dist(locs), cm, cp)[0], dtype=np.float64) + np.diag(np.broadcast_to(tau, (n,)))
    Lc = np.linalg.cholesky(S)
    assert np.all(np.triu(A, 1) == 0.0)
    assert np.abs(A - Lc).max() <= 1e-13 * np.abs(Lc).max()


def test_truth_is_the_inverse_of_the_whitening_truth():
    import gpvecchia_amd as G
    rng = np.random.default_rng(2)
    n = 120
    locs = rng.random((n, 2))
    va = G.vecchia_specify(locs, 9, cond_yz="z", nn_backend="host")
    E = rng.standard_normal((n, 3))
    tau = rng.uniform(0.05, 0.3, n)
    nn = va["U_prep"]["revNNarray"]
    B = U.unwhiten_ld(va["locsord"], nn, E, "esqe", [0.8, 0.25, 0.5, 0.2], tau)
    # (whiten_ld takes float64 columns: the rounding of B to float64 is all that separates the two)
    E2, _ = W.whiten_ld(va["locsord"], nn, B.astype(np.float64), "esqe", [0.8, 0.25, 0.5, 0.2], tau)
    assert float(np.abs(E2 - E).max()) <= 1e-14 * float(np.abs(E).max())


def test_level_helper_equals_the_brute_force_definition():
    """a 50-row plan; and the launch count of a hand-made level sequence"""
    import gpvecchia_amd as G
    rng = np.random.default_rng(3)
    va = G.vecchia_specify(rng.random((50, 2)), 4, cond_yz="z", nn_backend="host")
    nn = va["U_prep"]["revNNarray"]
    lev = U.levels(nn)
    assert np.array_equal(lev, U.levels_brute(nn))
    assert lev[:5].tolist() == [0, 1, 2, 3, 4] and lev.max() < 50              # the first m + 1 rows are a chain
    # widths 1, 1, 5, 5, 1, 5 at narrow = 2: runs {0, 1} and {4}, wide 2, 3, 5
    hand = np.repeat(np.arange(6), [1, 1, 5, 5, 1, 5])
    assert U.launches(hand, 2) == (6, 5)
    assert U.launches(hand, 5) == (6, 1) and U.launches(hand, 0) == (6, 6)


def test_symbols_are_exported():
    from gpvecchia_amd import _lib
    import gpvecchia_amd as G
    names = ("gpv_unwhiten_narrow", "gpv_plan_unwhiten_levels", "gpv_plan_unwhiten", "gpv_plan_simulate")
    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "gpvecchia.h")).read()
    for nm in names:
        assert nm in _lib.EXPORTS and hasattr(_lib.lib(), nm) and f"int {nm}(" in header
    assert 1 <= _lib.lib().gpv_unwhiten_narrow() <= 1024
    for nm in ("vecchia_unwhiten", "vecchia_simulate"):
        assert callable(getattr(G, nm))
    for nm in ("unwhiten", "unwhiten_levels", "simulate"):
        assert callable(getattr(G.Plan, nm))


def test_null_arguments_are_bad_arguments():
    """before a device is touched: there is none here"""
    from gpvecchia_amd import _lib
    lib = _lib.lib()
    E, B = np.zeros(4), np.zeros(4)
    nf, nl = C.c_int64(0), C.c_int64(0)
    assert lib.gpv_plan_unwhiten(None, _lib.dptr(E), 4, 1, _lib.dptr(B), 4, C.byref(nf)) == 2
    assert lib.gpv_plan_simulate(None, 1, 0, 1, _lib.dptr(B), 4, C.byref(nf)) == 2
    assert lib.gpv_plan_unwhiten_levels(None, C.byref(nl), C.byref(nl)) == 2


def test_python_layer_refusals_without_a_device():
    import gpvecchia_amd as G
    rng = np.random.default_rng(0)
    n = 50
    locs, e = rng.random((n, 2)), rng.standard_normal(n)
    cp = [1.0, 0.1, 1.5]
    vz = G.vecchia_specify(locs, 5, cond_yz="z", nn_backend="host")
    vs = G.vecchia_specify(locs, 5, cond_yz="SGV", nn_backend="host")
    with pytest.raises(ValueError, match="vecchia_unwhiten: the columns must have one row per location"):
        G.vecchia_unwhiten(e[:-1], vz, cp, 0.1)
    en = e.copy()
    en[3] = np.nan
    with pytest.raises(ValueError, match="vecchia_unwhiten needs complete, finite columns"):
        G.vecchia_unwhiten(en, vz, cp, 0.1)
    with pytest.raises(ValueError, match="vecchia_unwhiten needs cond_yz='z'"):
        G.vecchia_unwhiten(e, vs, cp, 0.1)
    with pytest.raises(ValueError, match="vecchia_simulate needs cond_yz='z'"):
        G.vecchia_simulate(vs, cp, 0.1)
    with pytest.raises(ValueError, match="vecchia_unwhiten needs a named covariance"):
        G.vecchia_unwhiten(e, vz, cp, 0.1, covmodel=np.eye(n))
    with pytest.raises(ValueError, match="vecchia_simulate needs a named covariance"):
        G.vecchia_simulate(vz, cp, 0.1, covmodel=lambda x: x)
    with pytest.raises(ValueError, match="vecchia_unwhiten: nuggets"):
        G.vecchia_unwhiten(e, vz, cp, np.full(n - 1, 0.1))
    with pytest.raises(ValueError, match="vecchia_simulate: nuggets"):
        G.vecchia_simulate(vz, cp, np.full(n + 1, 0.1))
    for bad in (0, -3, 1.5):
        with pytest.raises(ValueError, match="vecchia_simulate: nsim"):
            G.vecchia_simulate(vz, cp, 0.1, nsim=bad)
    for bad in (np.zeros(n - 1), np.zeros(n + 1), np.zeros((n, 2))):
        with pytest.raises(ValueError, match="vecchia_simulate: mean"):
            G.vecchia_simulate(vz, cp, 0.1, mean=bad)
    obs = np.ones(n, dtype=bool)
    obs[:5] = False
    vp = dict({k: v for k, v in vz.items() if isinstance(k, str)}, obs=obs)
    with pytest.raises(ValueError, match="vecchia_unwhiten does not take plans with prediction locations"):
        G.vecchia_unwhiten(e, vp, cp, 0.1)
    with pytest.raises(ValueError, match="vecchia_simulate does not take plans with prediction locations"):
        G.vecchia_simulate(vp, cp, 0.1)
