"""The long-double truth of the leave-block-out tests (tests/_blockcv_truth.py) against independent statements of the same
quantities, the host builder of the block index (gpv_blocks_index_host) against a Python restatement, and spatial_blocks.
CPU only.

Bars: as tests/test_loo_truth_host.py argues: the truth is long double (unit roundoff 5.4e-20) and the matrices below have
condition numbers below 1e5, so 1e-12 relative leaves four digits of room."""
import ctypes as C

import numpy as np
import pytest

import _blockcv_truth as BT
import _loo_truth as T

LD = np.longdouble
CM, CP, TAU = "matern", [1.3, 0.25, 1.5], 0.1


def _plan(n, m, seed=5):
    import gpvecchia_amd as G
    rng = np.random.default_rng(seed)
    locs = rng.random((n, 2))
    z = rng.standard_normal(n)
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="z", nn_backend="host")
    o = va["ord_z"] - 1
    return va, o, z[o]


def _labels(n, seed=2):
    """blocks of 17, 1, 2 and 40 scattered ordered rows, the rest kept"""
    perm = np.random.default_rng(seed).permutation(n)
    lab = np.full(n, -1, dtype=np.int64)
    lab[perm[:17]], lab[perm[17:18]], lab[perm[18:20]], lab[perm[20:60]] = 0, 1, 5, 9
    return lab


def test_full_conditioning_is_the_exact_gp():
    """(i) m = n - 1: the Vecchia model IS the Gaussian process, so the block conditionals are those of C + tau I"""
    n = 120
    va, o, z_ord = _plan(n, n - 1)
    lab = _labels(n)
    F = T.factor_ld(va["locsord"], va["U_prep"]["revNNarray"], CM, CP, TAU)
    got = BT.blockcv_ld(F, z_ord, lab)
    mean, var = BT.exact_blocks(va["locsord"], z_ord, CM, CP, TAU, lab)
    held = lab >= 0
    assert np.all(np.isnan(got["mean"][~held])) and np.all(np.isnan(got["var"][~held])) and got["n_heldout"] == 60
    em = float(np.abs(got["mean"][held, 0] - mean[held]).max() / np.abs(mean[held]).max())
    ev = float((np.abs(got["var"][held] - var[held]) / var[held]).max())
    print(f"m = n - 1: block mean {em:.2e} (max norm), variance {ev:.2e} (per entry)")
    assert em <= 1e-12 and ev <= 1e-12


def test_direct_conditional_of_the_vecchia_covariance():
    """(ii) m = 10, two blocks: the conditional from Sigma = Q^-1 partitioned by covariance equals the precision form"""
    n = 120
    va, o, z_ord = _plan(n, 10)
    lab = _labels(n)
    F = T.factor_ld(va["locsord"], va["U_prep"]["revNNarray"], CM, CP, TAU)
    got = BT.blockcv_ld(F, z_ord, lab)
    Sig = T.spd_inv_ld(BT.precision_ld(F, n))
    z = z_ord.astype(LD)
    for b in (0, 9):
        B = np.where(lab == b)[0]
        rest = np.setdiff1d(np.arange(n), B)
        W = Sig[np.ix_(B, rest)] @ T.spd_inv_ld(Sig[np.ix_(rest, rest)])
        mean, var = W @ z[rest], np.diag(Sig[np.ix_(B, B)] - W @ Sig[np.ix_(rest, B)])
        em = float(np.abs(got["mean"][B, 0] - mean).max() / np.abs(mean).max())
        ev = float((np.abs(got["var"][B] - var) / var).max())
        print(f"block {b} ({B.size} members): mean {em:.2e}, variance {ev:.2e}")
        assert em <= 1e-12 and ev <= 1e-12


def test_blocks_of_one_are_leave_one_out():
    """(iii)"""
    n = 120
    va, o, z_ord = _plan(n, 10)
    F = T.factor_ld(va["locsord"], va["U_prep"]["revNNarray"], CM, CP, np.linspace(0.05, 0.3, n))
    Z = np.column_stack([z_ord, np.random.default_rng(4).standard_normal(n)])
    got, loo = BT.blockcv_ld(F, Z, np.arange(n)[::-1].copy()), T.loo_ld(F, Z)
    em = float((np.abs(got["mean"] - loo["mean"]).max(axis=0) / np.abs(loo["mean"]).max(axis=0)).max())
    ev = float((np.abs(got["var"] - loo["var"]) / loo["var"]).max())
    es = float((np.abs(got["scores"][:, :6] - loo["scores"]) / loo["sabs"]).max())
    e6 = float((np.abs(got["scores"][:, 6] - loo["scores"][:, 2]) / loo["sabs"][:, 2]).max())
    e7 = float((np.abs(got["scores"][:, 7] - loo["scores"][:, 3]) / loo["sabs"][:, 3]).max())
    print(f"blocks of one: mean {em:.2e}, var {ev:.2e}, scores {es:.2e}, [6] against [2] {e6:.2e}, [7] against [3] {e7:.2e}")
    assert max(em, ev, es, e6, e7) <= 1e-12 and got["n_heldout"] == n


def _index_host(nn, rowid, n, newpos, lab):
    from gpvecchia_amd import _lib as L
    nn = np.ascontiguousarray(nn, dtype=np.int32)
    rowid = np.ascontiguousarray(rowid, dtype=np.int32)
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    newpos = None if newpos is None else np.ascontiguousarray(newpos, dtype=np.int32)
    rows, P = nn.shape
    memptr, members, setptr = np.full(n + 1, -9, np.int32), np.full(n, -9, np.int32), np.full(n + 1, -9, np.int32)
    sets, blkloc = np.full(rows * P + 1, -9, np.int32), np.full((n, 2), -9, np.int32)
    nb, nh, nr, ms = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1), C.c_int(-1)
    i32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
    st = L.lib().gpv_blocks_index_host(i32(nn), i32(rowid), rows, n, P, i32(newpos), i32(lab), C.byref(nb), C.byref(nh), C.byref(ms),
                                       C.byref(nr), i32(memptr), i32(members), i32(setptr), i32(sets), rows * P, i32(blkloc))
    return st, (int(nb.value), int(nh.value), int(ms.value), int(nr.value)), memptr, members, setptr, sets, blkloc


# six locations, P = 4, stored sets in another order than the output rows; position 1 ends two sets (coincident points), the
# first rows have missing entries, set 3 has no neighbours
NN = np.array([[-1, -1, 0, 2],
               [-1, 0, 2, 1],
               [0, 2, 1, 4],
               [-1, -1, -1, 0],
               [2, 4, 0, 5],
               [-1, 4, 0, 1]], dtype=np.int32)
ROWID = np.array([1, 2, 4, 0, 5, 3], dtype=np.int32)


def _check_index(nn, rowid, n, newpos, lab):
    st, counts, memptr, members, setptr, sets, blkloc = _index_host(nn, rowid, n, newpos, lab)
    want = BT.index_py(nn, rowid, n, newpos, lab)
    nb, nh, nr = len(want[0]) - 1, len(want[1]), len(want[3])
    assert st == 0 and counts == (nb, nh, int(np.diff(want[0]).max()), nr)
    assert np.array_equal(memptr[:nb + 1], want[0]) and np.array_equal(members[:nh], want[1])
    assert np.array_equal(setptr[:nb + 1], want[2]) and np.array_equal(sets[:nr], want[3]) and np.array_equal(blkloc, want[4])
    assert np.all(memptr[nb + 1:] == -9) and np.all(members[nh:] == -9) and np.all(sets[nr:] == -9)
    return counts, memptr, members, setptr, sets, blkloc


def test_block_index_entry_by_entry():
    """(iv)"""
    n = 6
    newpos = np.array([3, 0, 5, 1, 2, 4], dtype=np.int32)          # ordered row -> internal position
    # ordered rows 3 (position 1, the coincident pair's) and 1 (position 0) are label 5; row 4 (position 2) is label 2; label 4
    # is empty; the rest is kept
    lab = np.array([-1, 5, -1, 5, 2, -1], dtype=np.int32)
    counts, memptr, members, setptr, sets, blkloc = _check_index(NN, ROWID, n, newpos, lab)
    assert counts == (2, 3, 2, 10)
    assert list(members[:3]) == [2, 0, 1]                          # block 0 = label 2; block 1 = label 5 in ascending ordered row
    assert list(sets[setptr[0]:setptr[1]]) == [0, 1, 2, 4]         # position 2 is in the sets 0, 1, 2, 4
    assert list(sets[setptr[1]:setptr[2]]) == [0, 1, 2, 3, 4, 5]   # positions 0 or 1: every set, each once (sets 1, 2, 5 hold both)
    assert blkloc.tolist() == [[1, 0], [1, 1], [0, 0], [-1, -1], [-1, -1], [-1, -1]]
    # the identity numbering, every location a block of its own, labels descending
    _check_index(NN, ROWID, n, None, np.arange(n)[::-1])
    # the two that end in position 1 split over two blocks, and a random labelling of a real plan
    _check_index(NN, ROWID, n, None, np.array([0, 1, 1, -1, 0, 3]))
    import gpvecchia_amd as G
    m = 9
    locs = np.random.default_rng(3).random((150, 2))
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="z", nn_backend="host")
    nn = np.nan_to_num(np.asarray(va["U_prep"]["revNNarray"], dtype=np.float64), nan=0.0).astype(np.int32) - 1
    rng = np.random.default_rng(8)
    _check_index(nn, rng.permutation(150), 150, rng.permutation(150), rng.integers(-1, 12, 150))


def test_block_index_refusals():
    from gpvecchia_amd import _lib as L
    n = 6
    assert L.lib().gpv_blockcv_max_block() == 64 and L.lib().gpv_blockcv_nscores() == 8
    ok = np.zeros(n, dtype=np.int32)
    assert _index_host(NN, ROWID, n, None, ok)[0] == 0
    for bad in ([0, 0, 0, 0, 0, 6], [0, 0, 0, 0, 0, -2], [-1] * 6):            # a label >= Nlocs, < -1, no block at all
        assert _index_host(NN, ROWID, n, None, np.array(bad))[0] == 2
    assert _index_host(NN, ROWID, n, np.array([0, 1, 2, 3, 4, 4]), ok)[0] == 2   # newpos is no permutation
    assert _index_host(NN, [1, 2, 4, 0, 5, 6], n, None, ok)[0] == 2            # an output row out of range
    nn65 = np.full((65, 2), -1, dtype=np.int32)
    nn65[:, 1] = np.arange(65)
    assert _index_host(nn65, np.arange(65), 65, None, np.zeros(65))[0] == 2     # a block of 65
    st, counts = _index_host(nn65, np.arange(65), 65, None, np.r_[np.zeros(64), 1])[:2]
    assert st == 0 and counts == (2, 65, 64, 65)
    nb = C.c_int64(-1)
    ms = C.c_int(-1)
    # rows x P >= 2^31: refused before any array is read (the arrays are NULL)
    assert L.lib().gpv_blocks_index_host(None, None, 1 << 27, 1 << 27, 16, None, None, C.byref(nb), C.byref(nb), C.byref(ms),
                                         C.byref(nb), None, None, None, None, 0, None) == 8
    assert nb.value == -1


def test_spatial_blocks():
    """(v)"""
    import gpvecchia_amd as G
    rng = np.random.default_rng(6)
    for n, d, cap in ((1000, 2, 64), (777, 3, 10), (65, 1, 64), (300, 2, 1)):
        locs = rng.random((n, d))
        lab = G.spatial_blocks(locs, cap)
        sizes = np.bincount(lab)
        assert lab.shape == (n,) and np.issubdtype(lab.dtype, np.integer) and lab.min() == 0
        assert sizes.min() >= 1 and sizes.max() <= cap and sizes.sum() == n    # a partition into cells <= max_size, no id empty
        assert np.array_equal(lab, G.spatial_blocks(locs.copy(), cap))          # deterministic
        print(f"n = {n}, d = {d}, max_size = {cap}: {sizes.size} cells of {sizes.min()} .. {sizes.max()} points")
    assert np.all(G.spatial_blocks(rng.random((64, 2))) == 0) and np.all(G.spatial_blocks(rng.random((7, 2)), 7) == 0)
    # cells are spatial: the first split of the unit square is on the first coordinate
    locs = rng.random((128, 2))
    lab = G.spatial_blocks(locs)
    assert set(lab) == {0, 1} and locs[lab == 0, 0].max() <= locs[lab == 1, 0].min()
    # duplicated points do not loop forever: 200 copies of one point, and a cloud with heavy ties
    same = np.tile([[0.3, 0.7]], (200, 1))
    sizes = np.bincount(G.spatial_blocks(same, 64))
    assert sizes.sum() == 200 and sizes.max() <= 64
    ties = np.round(rng.random((500, 2)), 1)
    assert np.bincount(G.spatial_blocks(ties, 16)).max() <= 16
    with pytest.raises(ValueError):
        G.spatial_blocks(locs, 0)
