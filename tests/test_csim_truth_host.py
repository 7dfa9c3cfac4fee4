"""The long-double truth of the conditional-simulation tests (tests/_csim_truth.py) against independent statements of the same
quantities, and the host builder of the level schedule (gpv_csim_levels_host) against a Python restatement.  CPU only.

Bars: the truth is long double (unit roundoff 5.4e-20); the matrices of the exact case have condition numbers below 1e4, so
1e-12 of the largest entry leaves room over the 1e-15 to 1e-14 the identities show (printed)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _csim_truth as T
import _krige_truth as KT

GPV_OK, GPV_ERR_BAD_ARG, GPV_ERR_INDEX = 0, 2, 8


def test_full_conditioning_is_the_exact_gp_conditional():
    c = T.exact_case()
    n, nq = c["locs"].shape[0], c["q"].shape[0]
    NN = T.ordered_search(c["locs"], c["q"], c["m"])
    assert all(np.count_nonzero(NN[i]) == n + i for i in range(nq))         # everything before the row
    t = T.truth(c["locs"], c["tau"], c["Z"], c["q"], NN, c["covmodel"], c["cp"])
    assert not t["failed"].any()
    F = t["colour"](np.eye(nq))
    mean, Fd = T.dense_joint(c["locs"], c["tau"], c["Z"], c["q"], c["covmodel"], c["cp"])
    em = float(np.abs(t["mean"] - mean).max() / np.abs(mean).max())
    ef = float(np.abs(F - Fd).max() / np.abs(Fd).max())
    print(f"m = n + nq - 1: mean {em:.2e}, factor of the conditional covariance {ef:.2e} (of the largest entry)")
    assert np.all(np.triu(F, 1) == 0)
    assert em <= 1e-12 and ef <= 1e-12


def test_rows_without_predicted_neighbours_are_local_kriging():
    rng = np.random.default_rng(3)
    locs, Z, q = rng.random((300, 2)), rng.standard_normal((300, 3)), rng.random((60, 2))
    cp = [1.2, 0.07, 1.5]
    NN = T.ordered_search(locs, q, 10)
    lev, _, _ = T.levels(NN, 300)
    rows = np.flatnonzero(lev == 0)
    assert 5 <= rows.size < 60
    t = T.truth(locs, 0.1, Z, q, NN, "matern", cp)
    mean, var, _, failed = KT.krige_ld(locs, 0.1, Z, q[rows], NN[rows], "matern", cp)
    assert not failed.any() and not t["failed"].any()
    em = float(np.abs(t["mean"][rows] - mean).max() / np.abs(mean).max())
    ev = float((np.abs(t["sd"][rows] ** 2 - var) / var).max())
    print(f"{rows.size} rows of level 0: mean {em:.2e}, sd^2 against the kriging variance {ev:.2e}")
    assert em <= 1e-12 and ev <= 1e-12


def test_a_duplicate_location_fails_and_its_nan_spreads():
    rng = np.random.default_rng(4)
    locs, Z, q = rng.random((200, 2)), rng.standard_normal(200), rng.random((50, 2))
    q[20] = q[7]                                                               # a copy of an earlier prediction location
    q[3] = locs[11]                                                            # on an observation that has a nugget: legal
    NN = T.ordered_search(locs, q, 8)
    t = T.truth(locs, 0.1, Z, q, NN, "matern", [1.2, 0.07, 1.5])
    assert t["failed"][20] and not t["failed"][3] and not t["failed"][7]
    assert t["nan"][20] and not t["nan"][:20].any()
    dep = [i for i in range(50) if (NN[i] == 200 + 20 + 1).any()]
    assert dep and all(t["nan"][i] for i in dep)
    assert np.array_equal(np.isnan(t["colour"](np.ones((50, 1)))[:, 0]), t["nan"])


def _levels_host(NN, n):
    import gpvecchia_amd._lib as L
    NNf = np.asfortranarray(NN, dtype=np.int32)
    nq, m = NNf.shape
    level, order = np.full(nq, -1, dtype=np.int32), np.full(nq, -1, dtype=np.int32)
    levptr = np.full(nq + 1, -1, dtype=np.int64)
    nlev = C.c_int64(-1)
    st = L.lib().gpv_csim_levels_host(L.iptr(NNf), nq, m, n, L.iptr(level), L.iptr(order),
                                      levptr.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(nlev))
    return st, level, order, levptr, int(nlev.value)


def _assert_levels(NN, n):
    st, level, order, levptr, nlev = _levels_host(NN, n)
    assert st == GPV_OK
    lv, od, lp = T.levels(NN, n)
    assert nlev == lp.size - 1
    assert np.array_equal(level, lv) and np.array_equal(order, od) and np.array_equal(levptr[: nlev + 1], lp)
    assert (levptr[nlev + 1:] == -1).all()
    return lv, lp


def test_levels_host_on_random_lists():
    rng = np.random.default_rng(8)
    for n, nq, m in ((50, 300, 5), (0, 40, 3), (7, 1, 4), (1000, 2000, 30)):
        NN = np.zeros((nq, m), dtype=np.int32)
        for i in range(nq):
            k = int(rng.integers(0, m + 1))
            pool = n + i
            if pool:
                NN[i, :k] = rng.integers(1, pool + 1, k)
        _assert_levels(NN, n)


@functools.lru_cache(maxsize=None)
def _shape_lists(which):
    c = T.wide_case() if which == "wide" else T.deep_case()
    return c["locs"].shape[0], T.ordered_search(c["locs"], c["q"], c["m"])


def test_levels_host_on_the_wide_shape():
    n, NN = _shape_lists("wide")
    lv, lp = _assert_levels(NN, n)
    width = np.diff(lp)
    print(f"wide shape: {lp.size - 1} levels, widest {width.max()}, {int((width > 256).sum())} above 256")
    assert (width > 256).sum() >= 2 and (width <= 256).sum() >= 2                # both launch forms are needed


def test_levels_host_on_the_deep_shape():
    n, NN = _shape_lists("deep")
    lv, lp = _assert_levels(NN, n)
    width = np.diff(lp)
    print(f"deep shape: {lp.size - 1} levels, widest {width.max()}")
    assert lp.size - 1 >= 40 and width.max() <= 256                             # one run of narrow levels


def test_levels_host_refusals():
    NN = np.zeros((5, 2), dtype=np.int32)
    NN[2, 0] = 10 + 2 + 1                                                      # its own row: a forward id
    assert _levels_host(NN, 10)[0] == GPV_ERR_INDEX
    NN[2, 0] = 10 + 2                                                          # the row before: legal
    assert _levels_host(NN, 10)[0] == GPV_OK
    NN[4, 1] = -1
    assert _levels_host(NN, 10)[0] == GPV_ERR_INDEX
    NN[4, 1] = 10 + 4 + 3                                                      # beyond every row
    assert _levels_host(NN, 10)[0] == GPV_ERR_INDEX
    import gpvecchia_amd._lib as L
    assert L.lib().gpv_csim_levels_host(None, 5, 2, 10, None, None, None, None) == GPV_ERR_BAD_ARG
