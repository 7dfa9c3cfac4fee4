"""gpv_find_query_nn (csrc/gpv_nn.hip) against the search definition (tests/_krige_truth.py query_nn, which
tests/test_krige_truth_host.py pins to the host search): both routes, every bucket of list lengths, ties, duplicates, queries on
observations and outside the bounding box, an eligibility mask, non-finite inputs.

Every comparison is np.array_equal of int32 arrays.  The truth of an input is computed once at the longest list any test of it
asks for; a shorter list is its head.  Sizes: from 2048 searchable points on, inputs in one to three dimensions go through the
uniform grid (n = 3000 here, and 2040 / 2060 on either side of the threshold); everything else is brute force.  nq = 130: three
wavefronts, the last one partial.
"""
import functools
import os

import numpy as np
import pytest

import _krige_truth as KT

pytestmark = pytest.mark.gpu

MS = (1, 15, 30, 63, 85)
MMAX = max(MS)
GRID_FROM = 2048                                            # kQnnGridFrom


def _gpu(locs, q, m, eligible=None):
    import gpvecchia_amd as G
    from gpvecchia_amd import specify as S
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return S.find_query_nn_gpu(locs, q, m, eligible=eligible)


def _brute(locs, q, m, eligible=None):
    """the same call with the brute-force route forced"""
    os.environ["GPV_NN_BRUTE"] = "1"
    try:
        return _gpu(locs, q, m, eligible)
    finally:
        del os.environ["GPV_NN_BRUTE"]


@functools.lru_cache(maxsize=None)
def _uniform(n, d):
    rng = np.random.default_rng(100 * d + n)
    locs, q = rng.random((n, d)), rng.random((130, d))
    want = KT.query_nn(locs, q, MMAX)
    for a in (locs, q, want):
        a.setflags(write=False)
    return locs, q, want


@pytest.mark.parametrize("d,n", [(1, 3000), (2, 3000), (3, 3000), (4, 3000), (2, 2040), (2, 2060), (8, 500)])
def test_random_points_every_list_length(d, n):
    """dimensions 1 - 3 on the grid route (n on either side of its threshold), 4 and 8 by brute force"""
    locs, q, want = _uniform(n, d)
    for m in MS:
        got = _gpu(locs, q, m)
        assert got.shape == (130, m) and got.dtype == np.int32
        assert np.array_equal(got, want[:, :m]), (d, n, m)


@pytest.mark.parametrize("d", [1, 2, 3])
def test_both_routes_give_identical_arrays(d):
    locs, q, want = _uniform(3000, d)
    for m in (15, 85):
        assert np.array_equal(_brute(locs, q, m), _gpu(locs, q, m))
        assert np.array_equal(_brute(locs, q, m), want[:, :m])


def test_fewer_points_than_m():
    locs, q, _ = _uniform(3000, 2)
    got = _gpu(locs[:5], q, 10)
    assert np.array_equal(got, KT.query_nn(locs[:5], q, 10))
    assert (got[:, :5] > 0).all() and (got[:, 5:] == 0).all()


def _big_tie_grid():
    g = np.arange(48) / 32.0                                # 2304 points: the grid route, every distance ties
    locs = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    h = np.arange(0, 95, 7) / 64.0
    q = np.stack(np.meshgrid(h, h, indexing="ij"), axis=-1).reshape(-1, 2)
    return locs, q


CASES = {"ties": (KT.tie_grid, False), "ties_large": (_big_tie_grid, True),
         "duplicated": (KT.duplicated, False), "duplicated_large": (lambda: KT.duplicated(n=3000), True),
         "on_points": (KT.on_points, False), "on_points_large": (lambda: KT.on_points(n=3000), True),
         "outside_box": (KT.outside_box, False), "outside_box_large": (lambda: KT.outside_box(n=3000), True)}


@pytest.mark.parametrize("case", list(CASES))
def test_ties_duplicates_on_points_outside(case):
    """the inputs of the host test (brute force at their size) and the same recipes at n = 3000 (the grid route)"""
    make, on_grid = CASES[case]
    locs, q = make()
    assert (locs.shape[0] >= GRID_FROM) == on_grid
    want = KT.query_nn(locs, q, 30)
    for m in (1, 15, 30):
        assert np.array_equal(_gpu(locs, q, m), want[:, :m]), (case, m)
    assert np.array_equal(_brute(locs, q, 30), want)


@pytest.mark.parametrize("n", [500, 3300])
def test_eligible_mask_removes_a_third(n):
    locs, q, _ = _uniform(3000, 2)
    rng = np.random.default_rng(n)
    locs = np.vstack([locs, rng.random((300, 2))])[:n]
    el = np.arange(n) % 3 != 1
    assert (el.sum() >= GRID_FROM) == (n > 3000)
    got = _gpu(locs, q, 30, eligible=el)
    assert np.array_equal(got, KT.query_nn(locs, q, 30, eligible=el))
    assert not np.isin(got, np.nonzero(~el)[0] + 1).any()
    assert np.array_equal(got, _brute(locs, q, 30, eligible=el))


@pytest.mark.parametrize("n", [500, 3000])
def test_nonfinite_query_and_points(n):
    """a NaN query and an infinite one get rows of zeros; a NaN point and an infinite point enter no list"""
    locs, q, _ = _uniform(3000, 2)
    locs, q = locs[:n].copy(), q.copy()
    q[17, 1], q[64, 0] = np.nan, np.inf
    locs[3, 0], locs[11, 1] = np.nan, -np.inf
    got = _gpu(locs, q, 15)
    assert np.array_equal(got, KT.query_nn(locs, q, 15))
    assert (got[17] == 0).all() and (got[64] == 0).all() and not np.isin(got, [4, 12]).any()
    assert (np.delete(got, [17, 64], axis=0) > 0).all()


def test_refusals_leave_the_output_unwritten():
    import ctypes as C
    from gpvecchia_amd import _lib
    locs, q, _ = _uniform(3000, 2)
    lf, qf = np.asfortranarray(locs), np.asfortranarray(q)
    out = np.full((130, 15), -77, dtype=np.int32, order="F")
    f = _lib.lib().gpv_find_query_nn
    for args in ((0, _lib.dptr(lf), 3000, 2, None, _lib.dptr(qf), 130, 0, _lib.iptr(out)),
                 (0, _lib.dptr(lf), 3000, 2, None, _lib.dptr(qf), 130, _lib.lib().gpv_nn_max_m() + 1, _lib.iptr(out)),
                 (0, _lib.dptr(lf), 3000, 9, None, _lib.dptr(qf), 130, 15, _lib.iptr(out)),
                 (0, _lib.dptr(lf), 0, 2, None, _lib.dptr(qf), 130, 15, _lib.iptr(out)),
                 (0, None, 3000, 2, None, _lib.dptr(qf), 130, 15, _lib.iptr(out))):
        assert f(*args) == 2
    assert f(99, _lib.dptr(lf), 3000, 2, None, _lib.dptr(qf), 130, 15, _lib.iptr(out)) == 1
    assert (out == -77).all()
    assert f(0, _lib.dptr(lf), 3000, 2, C.cast(None, C.POINTER(C.c_uint8)), _lib.dptr(qf), 0, 15, None) == 0
