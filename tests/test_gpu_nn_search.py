"""gpv_find_ordered_nn (csrc/gpv_nn.hip) against the definition (tests/_nn_truth.py, pinned to the oracle by
tests/test_nn_truth_host.py): long rows, near ties, shards, degenerate and non-finite inputs, refusals.

Every comparison is np.array_equal of int32 arrays: one wrong index changes every conditioning set downstream, and no
tolerance would see it.  The truth of an input is computed once, for ALL rows and at the longest list any test of that input
asks for; a shorter list is its head (test_nn_truth_host.py).  Every call goes through the C entry on an array pre-filled with a
sentinel, so an entry the call should not have written shows.

Sizes: the brute-force kernel serves every row of inputs up to 8192 points and the rows below 4096 of larger ones (n <= 700
here); the grid kernel serves rows >= 4096 of inputs with more than 8192 points in one to three dimensions (n = 8300 .. 9000
here).  From m = 85 on a launch asks for more than 64 KB of LDS, m = 191 is the longest row a plan takes, and
gpv_nn_max_m() = 212 is the longest list one compute unit's 160 KB can hold.
"""
import functools

import numpy as np
import pytest

import _nn_truth as T

pytestmark = pytest.mark.gpu

SENTINEL = -77
GPV_OK, GPV_ERR_BAD_ARG = 0, 2
GRID_FROM = 4096                                            # kGridFrom: rows from here on go through the grid


def _need_gpu():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


def _search(locs, m, rows=None, device=0):
    """(status, array): the C entry on a sentinel-filled n x (m+1) array."""
    _need_gpu()
    from gpvecchia_amd import _lib
    locs = np.asfortranarray(locs, dtype=np.float64)
    n, d = locs.shape
    a, b = (0, n) if rows is None else rows
    out = np.full((n, m + 1), SENTINEL, dtype=np.int32, order="F")
    st = _lib.lib().gpv_find_ordered_nn(device, _lib.dptr(locs), n, d, m, a, b, _lib.iptr(out))
    return st, np.ascontiguousarray(out)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _uniform(n, d, mmax):
    """(points, truth at m = mmax for all rows), shared and read-only"""
    locs = np.random.default_rng(1000 * d + n).random((n, d))
    return _frozen(locs, T.nn_all(locs, mmax))


@functools.lru_cache(maxsize=None)
def _near_ties(n, levels, step, tiny, split_dims, m):
    """(points, truth, its squared-distance twin) of a near-tie recipe (tests/_nn_truth.py near_tie_points)"""
    locs = T.near_tie_points(n, levels, step, tiny, split_dims)
    return _frozen(locs, T.nn_all(locs, m), T.nn_all(locs, m, "ssq"))


# ----------------------------------------------------------------------------------------------------------------
# long rows
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("m", [0, 1, 63, 84, 85, 127, 191])
def test_long_rows_brute_force(m, d):
    """m = 84 is the last launch within 64 KB of LDS (65 280 B), m = 85 the first beyond, m = 191 the longest row of a plan;
    d = 5 and 8 take the instantiation for any dimension.  n = 600: ten workgroups, the last one partly idle, and at m = 191
    a third of the lists shorter than m + 1."""
    locs, truth = _uniform(600, d, 191)
    st, nn = _search(locs, m)
    assert st == GPV_OK
    assert np.array_equal(nn, truth[:, : m + 1])


@pytest.mark.parametrize("d", [4, 6, 7])
def test_generic_dimensions(d):
    locs, truth = _uniform(700, d, 10)
    st, nn = _search(locs, 10)
    assert st == GPV_OK and np.array_equal(nn, truth)


def test_single_point():
    st, nn = _search(np.array([[0.25, 0.5]]), 5)
    assert st == GPV_OK and np.array_equal(nn, [[1, 0, 0, 0, 0, 0]])


def test_every_list_shorter_than_the_row():
    locs, truth = _uniform(100, 2, 191)
    assert (truth[:, -1] == 0).all() and truth[99, 99] != 0
    st, nn = _search(locs, 191)
    assert st == GPV_OK and np.array_equal(nn, truth)


def test_longest_admitted_list():
    """gpv_nn_max_m() is derived from the LDS of one compute unit: the launch at that m asks for all of it and must work."""
    _need_gpu()
    from gpvecchia_amd import _lib
    mmax = _lib.lib().gpv_nn_max_m()
    assert mmax == 160 * 1024 // (12 * 64) - 1 == 212 and mmax + 1 >= _lib.lib().gpv_max_p()
    locs, truth = _uniform(300, 2, 212)
    st, nn = _search(locs, mmax)
    assert st == GPV_OK and np.array_equal(nn, truth)


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("m", [84, 85, 191])
def test_long_rows_through_the_grid(m, d):
    locs, truth = _uniform(9000, d, 191)
    st, nn = _search(locs, m)
    assert st == GPV_OK
    assert np.array_equal(nn, truth[:, : m + 1])


# ----------------------------------------------------------------------------------------------------------------
# near ties: squared distances an ulp or two apart whose rounded square roots coincide.  The definition ranks by the
# square root, so the lower index wins there; a kernel that ranked by the squared distance would take the closer one.
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", sorted(T.NEAR_TIE_BRUTE))
def test_near_ties_brute_force(m):
    locs, truth, twin = _near_ties(600, 2048, 2.0 ** -10, T.NEAR_TIE_BRUTE[m], 1, m)
    assert len(T.differing_rows(truth, twin)) >= 10        # a condition on the input: it tells the two orders apart
    st, nn = _search(locs, m)
    assert st == GPV_OK
    assert np.array_equal(nn, truth)


@pytest.mark.parametrize("case", ["one_split_dimension", "two_split_dimensions"])
def test_near_ties_through_the_grid(case):
    """one_split_dimension: x on 2^20 levels, a tiny y (the grid has one cell across it).  two_split_dimensions: x and y on a
    128 x 128 lattice two units wide (9000 points on 16 384 sites: lattice ties and duplicates besides), a tiny z of 2^-30:
    the neighbours lie about 2^-3 away, the ulp of their squared distance is 2^-58 and z^2 is 2^-60 .. 2^-54."""
    if case == "one_split_dimension":
        locs, truth, twin = _near_ties(9000, 2 ** 20, 2.0 ** -19, 2.0 ** -36, 1, 100)
    else:
        locs, truth, twin = _near_ties(9000, 128, 2.0 ** -6, 2.0 ** -30, 2, 100)
    assert len(T.differing_rows(truth[GRID_FROM:], twin[GRID_FROM:])) >= 10   # a condition on the input, over the grid's rows
    st, nn = _search(locs, 100)
    assert st == GPV_OK
    assert np.array_equal(nn, truth)


# ----------------------------------------------------------------------------------------------------------------
# shards
# ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _full_search_9000():
    locs, truth = _uniform(9000, 2, 191)
    st, nn = _search(locs, 30)
    assert st == GPV_OK
    return _frozen(nn)[0]


@pytest.mark.parametrize("rows", [(4000, 4200), (4096, 4097), (4095, 4096), (4096, 9000), (0, 4096), (8999, 9000), (5000, 5000)])
def test_shards(rows):
    """Shards that straddle, touch or avoid the row where the grid takes over, one row, the last row, no row: the rows inside
    equal the same rows of the full search (and the definition), every other entry is left as the caller had it."""
    locs, truth = _uniform(9000, 2, 191)
    full = _full_search_9000()
    assert np.array_equal(full, truth[:, :31])
    a, b = rows
    st, nn = _search(locs, 30, rows=rows)
    assert st == GPV_OK
    assert np.array_equal(nn[a:b], full[a:b])
    assert (nn[:a] == SENTINEL).all() and (nn[b:] == SENTINEL).all()


# ----------------------------------------------------------------------------------------------------------------
# degenerate inputs at a size that would take the grid
# ----------------------------------------------------------------------------------------------------------------
def test_all_points_identical():
    """Every distance is 0, so the lower indices win: row k is 1 .. 11 for k >= 10, and k itself is not in its own list."""
    n, m = 8300, 10
    locs = np.tile([0.3, -1.7], (n, 1))
    expect = np.tile(np.arange(1, m + 2, dtype=np.int32), (n, 1))
    expect[np.arange(1, m + 2)[None, :] > (np.arange(n) + 1)[:, None]] = 0
    sample = [0, 1, 9, 10, 11, 4095, 4096, n - 1]
    assert np.array_equal(expect[sample], T.nn_rows(locs, m, sample))
    st, nn = _search(locs, m)
    assert st == GPV_OK and np.array_equal(nn, expect)


@pytest.mark.parametrize("case", ["shifted_1e6", "scaled_1e-6"])
def test_shifted_and_scaled_clouds(case):
    """The definition evaluated on the same coordinates: after a shift by 1e6 the differences keep 30 bits or so and many
    distances tie; after a scaling by 1e-6 the squared distances are near 1e-16.  (Not covered, and not believed to work:
    clouds narrower than about 1e-146, where the dw * dw of the kernels' pre-filter is denormal and loses the nine parts in
    1e16 of slack it is compared with.)"""
    n, m = 8300, 10
    base = np.random.default_rng(77).random((n, 2))
    locs = base + 1e6 if case == "shifted_1e6" else base * 1e-6
    st, nn = _search(locs, m)
    assert st == GPV_OK and np.array_equal(nn, T.nn_all(locs, m))


# ----------------------------------------------------------------------------------------------------------------
# non-finite coordinates
# ----------------------------------------------------------------------------------------------------------------
def test_non_finite_coordinates():
    """One NaN point and one +Inf point at n > 8192: the grid is abandoned, the status is GPV_OK, every index is a
    predecessor, rows with m + 1 finite predecessors are those of the definition (non-finite distances sort last and stay
    out), and what include/gpvecchia.h says about the rest holds: a candidate at a NaN or infinite distance never enters a
    list, so the rows of the two points themselves are empty."""
    n, m = 8300, 10
    locs = np.random.default_rng(78).random((n, 2))
    i_nan, i_inf = 150, 4500
    locs[i_nan, 0] = np.nan
    locs[i_inf, 1] = np.inf
    st, nn = _search(locs, m)
    assert st == GPV_OK
    k1 = np.arange(n)[:, None] + 1
    assert ((nn >= 0) & (nn <= k1)).all()
    finite = np.isfinite(locs).all(axis=1)
    npred = np.cumsum(finite)                               # finite predecessors, self included
    full = finite & (npred >= m + 1)
    assert full.sum() == n - 2 - (m + 1 - 1)                # (every row from m on but the two)
    truth = T.nn_all(locs, m)
    assert np.array_equal(nn[full], truth[full])
    assert not np.isin(nn[full], [i_nan + 1, i_inf + 1]).any()
    assert np.array_equal(nn[:m + 1], truth[:m + 1])        # the short lists at the start: no non-finite point yet
    assert not nn[i_nan].any() and not nn[i_inf].any()


# ----------------------------------------------------------------------------------------------------------------
# refusals: GPV_ERR_BAD_ARG from the argument check, before the device is looked at (the device number given does not exist
# and is not what gets reported), the caller's array untouched
# ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    _need_gpu()
    from gpvecchia_amd import _lib
    L = _lib.lib()
    n, m = 100, 10
    locs = np.asfortranarray(np.random.default_rng(5).random((n, 8)))
    out = np.full((n, 256), SENTINEL, dtype=np.int32, order="F")
    lp, op = _lib.dptr(locs), _lib.iptr(out)
    nodev = 1 << 20
    mmax = L.gpv_nn_max_m()
    cases = {
        "dim = 0": (lp, n, 0, m, 0, n, op),
        "dim = 9": (lp, 80, 9, m, 0, 80, op),
        "m = -1": (lp, n, 2, -1, 0, n, op),
        "first m beyond the range": (lp, n, 2, mmax + 1, 0, n, op),
        "m = 255": (lp, n, 2, 255, 0, n, op),
        "row_begin > row_end": (lp, n, 2, m, 51, 50, op),
        "row_end > n": (lp, n, 2, m, 0, n + 1, op),
        "row_begin < 0": (lp, n, 2, m, -1, n, op),
        "n = 0": (lp, 0, 2, m, 0, 0, op),
        "NULL locs": (None, n, 2, m, 0, n, op),
        "NULL NNarray": (lp, n, 2, m, 0, n, None),
    }
    for what, args in cases.items():
        for device in (0, nodev):
            assert L.gpv_find_ordered_nn(device, *args) == GPV_ERR_BAD_ARG, (what, device)
        assert (out == SENTINEL).all(), what
    assert L.gpv_find_ordered_nn(nodev, lp, n, 2, m, 0, n, op) == 1       # GPV_ERR_NO_DEVICE: a good call, no such device
    assert (out == SENTINEL).all()
    assert L.gpv_find_ordered_nn(0, lp, n, 2, mmax, 0, n, op) == GPV_OK   # ... and the last m inside the range is served
    assert (out.ravel(order="F")[: n * (mmax + 1)] != SENTINEL).all() and (out.ravel(order="F")[n * (mmax + 1):] == SENTINEL).all()
