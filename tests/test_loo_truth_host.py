"""The long-double truth of the leave-one-out tests (tests/_loo_truth.py) against independent statements of the same quantities,
and the host builder of the transposed index (gpv_loo_index_host) against a Python restatement.  CPU only.

Bars: the truth is long double (unit roundoff 5.4e-20) and the matrices below have condition numbers below 1e5, so 1e-12
relative leaves four digits of room over the 2.6e-14 measured when the identities were checked."""
import ctypes as C

import numpy as np
import pytest

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


def test_full_conditioning_is_the_exact_gp():
    n = 120
    va, o, z_ord = _plan(n, n - 1)
    F = T.factor_ld(va["locsord"], va["U_prep"]["revNNarray"], CM, CP, TAU)
    got = T.loo_ld(F, z_ord)
    mean, var = T.dense_loo(va["locsord"], z_ord, CM, CP, TAU)
    em = float(np.abs(got["mean"][:, 0] - mean).max() / np.abs(mean).max())
    ev = float((np.abs(got["var"] - var) / var).max())
    print(f"m = n - 1: leave-one-out mean {em:.2e} (max norm), variance {ev:.2e} (per entry)")
    assert em <= 1e-12 and ev <= 1e-12
    # z'Qz is the sum of the squared whitened values
    e = T.apply_T(F, z_ord)[:, 0]
    r = T.apply_Tt(F, e)[:, 0]
    assert abs(float((z_ord.astype(LD) * r).sum() - (e * e).sum())) <= 1e-12 * float((e * e).sum())


def test_direct_conditional_of_the_vecchia_covariance():
    n = 120
    va, o, z_ord = _plan(n, 10)
    F = T.factor_ld(va["locsord"], va["U_prep"]["revNNarray"], CM, CP, TAU)
    got = T.loo_ld(F, z_ord)
    Tm = T.dense_T(F, n)
    assert np.all(np.triu(Tm, 1) == 0)                 # lower triangular in the ordered numbering
    Sig = T.spd_inv_ld(Tm.T @ Tm)
    z = z_ord.astype(LD)
    for i in (0, 57, n - 1):
        rest = np.array([j for j in range(n) if j != i])
        Ki = T.spd_inv_ld(Sig[np.ix_(rest, rest)])
        wgt = Sig[i, rest] @ Ki
        mean, var = wgt @ z[rest], Sig[i, i] - wgt @ Sig[rest, i]
        em, ev = float(abs(got["mean"][i, 0] - mean) / np.abs(got["mean"][:, 0]).max()), float(abs(got["var"][i] - var) / var)
        print(f"location {i}: mean {em:.2e}, variance {ev:.2e}")
        assert em <= 1e-12 and ev <= 1e-12


def test_dense_and_sparse_truth_agree():
    n = 120
    va, o, z_ord = _plan(n, 10)
    F = T.factor_ld(va["locsord"], va["U_prep"]["revNNarray"], CM, CP, np.linspace(0.05, 0.3, n))
    Tm = T.dense_T(F, n)
    B = np.random.default_rng(1).standard_normal((n, 3)).astype(LD)
    assert np.abs(T.apply_T(F, B) - Tm @ B).max() <= 1e-17 * n
    assert np.abs(T.apply_Tt(F, B) - Tm.T @ B).max() <= 1e-17 * n
    assert np.abs(T.qdiag(F, n) - np.diag(Tm.T @ Tm)).max() <= 1e-17 * n


def _index_host(nn, rowid, n):
    from gpvecchia_amd import _lib as L
    nn = np.ascontiguousarray(nn, dtype=np.int32)
    rowid = np.ascontiguousarray(rowid, dtype=np.int32)
    rows, P = nn.shape
    colptr, owner, col = np.full(n + 1, -9, np.int32), np.full(n, -9, np.int32), np.full(rows * P + 1, -9, np.int32)
    nnz = C.c_int64(-1)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
    st = L.lib().gpv_loo_index_host(i32(nn), i32(rowid), rows, n, P, i32(colptr), i32(owner), i32(col), rows * P, C.byref(nnz))
    return st, colptr, owner, col, int(nnz.value)


def test_transposed_index_entry_by_entry():
    # six locations, P = 4, stored sets in another order than the output rows; position 5 is nobody's neighbour, position 1
    # ends two sets (coincident points: the second lists its own entry in the column), set 3 has no neighbours
    nn = np.array([[-1, -1, 0, 2],
                   [-1, 0, 2, 1],
                   [0, 2, 1, 4],
                   [-1, -1, -1, 0],
                   [2, 4, 0, 5],
                   [-1, 4, 0, 1]], dtype=np.int32)
    rowid = np.array([1, 2, 4, 0, 5, 3], dtype=np.int32)
    n = 6
    st, colptr, owner, col, nnz = _index_host(nn, rowid, n)
    want_ptr, want_owner, want_col = T.index_py(nn, rowid, n)
    assert st == 0 and nnz == len(want_col) == colptr[n]
    assert np.array_equal(colptr, want_ptr) and np.array_equal(owner, want_owner) and np.array_equal(col[:nnz], want_col)
    assert np.all(col[nnz:] == -9)
    # by hand: position 0 is named by sets 0, 1, 2, 4, 5 (output rows 1, 2, 4, 5, 3) at left-aligned slots 0, 0, 0, 2, 1
    assert list(col[colptr[0]:colptr[1]]) == [1 * 4 + 0, 2 * 4 + 0, 4 * 4 + 0, 5 * 4 + 2, 3 * 4 + 1]
    assert owner[0] == 0 * 4 + 0 and owner[1] == 2 * 4 + 2 and owner[3] == -1 and owner[5] == 5 * 4 + 3
    assert list(col[colptr[1]:colptr[2]]) == [4 * 4 + 2, 3 * 4 + 2]            # the last one: set 5's OWN entry
    assert colptr[6] - colptr[5] == 0 and colptr[4] - colptr[3] == 0           # empty columns


def test_transposed_index_refusals():
    from gpvecchia_amd import _lib as L
    nnz = C.c_int64(-1)
    # rows x P >= 2^31: refused before any array is read (the arrays are NULL)
    assert L.lib().gpv_loo_index_host(None, None, 1 << 27, 1 << 27, 16, None, None, None, 0, C.byref(nnz)) == 8
    assert L.lib().gpv_loo_index_host(None, None, (1 << 27) - 1, 1 << 27, 16, None, None, None, 0, C.byref(nnz)) == 2
    assert nnz.value == -1
    nn = np.array([[-1, 0], [0, 1]], dtype=np.int32)
    assert _index_host(nn, [0, 1], 2)[0] == 0
    assert _index_host(np.array([[-1, 0], [0, 2]]), [0, 1], 2)[0] == 2         # a neighbour out of range
    assert _index_host(np.array([[0, -1], [0, 1]]), [0, 1], 2)[0] == 2         # a missing entry behind a valid one
    assert _index_host(nn, [0, 2], 2)[0] == 2                                  # an output row out of range


@pytest.mark.parametrize("n,m", [(600, 31)])
def test_in_degrees_of_a_maxmin_plan(n, m):
    """the skew the kernel must take: empty columns and columns several strides long"""
    import gpvecchia_amd as G
    locs = np.random.default_rng(3).random((n, 2))
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="z", nn_backend="host")
    nn = np.nan_to_num(np.asarray(va["U_prep"]["revNNarray"], dtype=np.float64), nan=0.0).astype(np.int32) - 1
    st, colptr, owner, col, nnz = _index_host(nn, np.arange(n), n)
    deg = np.diff(colptr)
    print("in-degree: zero at", int((deg == 0).sum()), "locations, max", int(deg.max()), ", above 64 at", int((deg > 64).sum()))
    assert st == 0 and nnz == int((nn[:, :-1] >= 0).sum()) and np.all(owner == np.arange(n) * (m + 1) + (nn >= 0).sum(axis=1) - 1)
    assert (deg == 0).sum() >= 1 and deg.max() > 64
