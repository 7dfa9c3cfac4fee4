"""tests/_nn_truth.py, the NumPy statement of the ordered nearest-neighbour definition that the GPU search is compared with,
pinned to the oracle's literal findOrderedNN (R/NN_kdtree.R:73-83), and what of gpv_find_ordered_nn can be checked without a
device: its limit and its argument check.  CPU only."""
import numpy as np
import pytest

import _nn_truth as T


def _oracle(locs, m):
    from oracle import r_side as R
    return np.nan_to_num(R.findOrderedNN(locs, m)).astype(np.int32)


@pytest.mark.parametrize("d", [1, 2, 3, 6])
def test_truth_equals_oracle_random(d):
    locs = np.random.default_rng(40 + d).random((300, d))
    for m in (0, 1, 12, 40):
        assert np.array_equal(T.nn_all(locs, m), _oracle(locs, m))


def test_truth_equals_oracle_lattice_with_duplicates():
    g = np.stack(np.meshgrid(np.arange(25.0), np.arange(17.0)), -1).reshape(-1, 2)      # regular grid: exact ties everywhere
    g = np.vstack([g, g[:9]])                                                         # exact duplicates
    assert np.array_equal(T.nn_all(g, 12), _oracle(g, 12))


def test_rows_are_prefixes_and_selected_rows_match():
    """A shorter list is the head of a longer one (the GPU tests compute one truth per input and slice it), and nn_rows of a
    selection equals the same rows of nn_all."""
    locs = np.random.default_rng(7).random((200, 2))
    full = T.nn_all(locs, 60)
    assert np.array_equal(T.nn_all(locs, 9), full[:, :10])
    rows = np.array([0, 1, 9, 10, 61, 199])
    assert np.array_equal(T.nn_rows(locs, 60, rows), full[rows])
    assert np.array_equal(full[0], np.r_[1, np.zeros(60, np.int32)]) and full[60, -1] != 0 and full[59, -1] == 0


def test_limit_of_the_gpu_search_and_its_argument_check():
    """gpv_nn_max_m() is what 160 KB of LDS hold at 12 bytes x 64 lanes per list entry and covers every row length a plan
    takes; the argument check of gpv_find_ordered_nn comes before the device is looked at, so it answers the same with or
    without a GPU and leaves the caller's array alone."""
    from gpvecchia_amd import _lib
    L = _lib.lib()
    mmax = L.gpv_nn_max_m()
    assert mmax == 160 * 1024 // (12 * 64) - 1 == 212 and mmax + 1 >= L.gpv_max_p()
    locs = np.asfortranarray(np.random.default_rng(0).random((50, 8)))
    out = np.full((50, 11), -77, dtype=np.int32, order="F")
    lp, op = _lib.dptr(locs), _lib.iptr(out)
    for args in [(lp, 50, 0, 10, 0, 50, op), (lp, 44, 9, 10, 0, 44, op), (lp, 50, 2, -1, 0, 50, op), (lp, 50, 2, mmax + 1, 0, 50, op),
                 (lp, 50, 2, 10, 26, 25, op), (lp, 50, 2, 10, 0, 51, op), (None, 50, 2, 10, 0, 50, op), (lp, 50, 2, 10, 0, 50, None)]:
        assert L.gpv_find_ordered_nn(0, *args) == 2                      # GPV_ERR_BAD_ARG
    assert (out == -77).all()


def test_ssq_key_is_a_different_order_on_near_ties():
    """Where two squared distances differ by an ulp or two and their square roots coincide, the definition takes the lower
    index and the squared-distance order does not: the near-tie recipe of the GPU tests has such rows, generic points have
    none."""
    a, b = np.float64(1.0 + 2.0 ** -51), np.nextafter(np.float64(1.0 + 2.0 ** -51), 2.0)
    assert a != b and np.sqrt(a) == np.sqrt(b)                       # what a near tie is
    for m, tiny in T.NEAR_TIE_BRUTE.items():
        locs = T.near_tie_points(600, 2048, 2.0 ** -10, tiny)
        assert len(T.differing_rows(T.nn_all(locs, m), T.nn_all(locs, m, "ssq"))) >= 10
    rnd = np.random.default_rng(1).random((100, 2))
    assert len(T.differing_rows(T.nn_all(rnd, 10), T.nn_all(rnd, 10, "ssq"))) == 0
