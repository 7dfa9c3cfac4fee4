"""The definition of the ordered nearest-neighbour arrays (R/NN_kdtree.R:73-83), stated once in NumPy for the tests of
gpv_find_ordered_nn (csrc/gpv_nn.hip).

Row k lists the min(m+1, k+1) points among 0..k closest to point k, itself included, by ascending
    d = sqrt(ssq),   ssq accumulated coordinate by coordinate as ssq + df*df in float64
(NumPy's sqrt, products and sums are correctly rounded and nothing is fused), ties to the lower index; 1-based, 0-padded.

key="ssq" ranks by the squared distance instead.  It is NOT the truth: it is what a kernel that skipped the square root would
compute.  The two orders differ exactly where two squared distances differ by an ulp or two and their rounded square roots
coincide, and the near-tie tests use it to prove that their inputs can tell the two apart.
"""
import numpy as np


def nn_rows(locs, m, rows, key="d"):
    """int32 (len(rows), m+1): the rows `rows` of the array of the definition (key="d") or of its squared-distance twin."""
    assert key in ("d", "ssq")
    locs = np.asarray(locs, dtype=np.float64)
    out = np.zeros((len(rows), m + 1), dtype=np.int32)
    for t, k in enumerate(rows):
        k = int(k)
        ssq = np.zeros(k + 1)
        with np.errstate(invalid="ignore"):                                     # (Inf - Inf: the non-finite inputs)
            for c in range(locs.shape[1]):
                df = locs[k, c] - locs[: k + 1, c]
                ssq = ssq + df * df
            d = np.sqrt(ssq) if key == "d" else ssq
        o = np.lexsort((np.arange(k + 1), d))[: min(m + 1, k + 1)]           # (NaN sorts last, behind +Inf)
        out[t, : len(o)] = o + 1
    return out


def nn_all(locs, m, key="d"):
    """Every row."""
    return nn_rows(locs, m, range(np.asarray(locs).shape[0]), key)


def near_tie_points(n, levels, step, tiny, split_dims=1, seed=3):
    """Points whose pair distances come in near ties: `split_dims` coordinates on a lattice of `levels` values `step` apart
    (exactly representable, so many pairs share the same large part of the squared distance) and one last coordinate out of
    0..8 times `tiny`, whose square moves the sum by an ulp or two: squared distances that differ, square roots that round
    to the same double."""
    rng = np.random.default_rng(seed)
    cols = [rng.integers(0, levels, n) * step for _ in range(split_dims)]
    cols.append(rng.integers(0, 9, n) * tiny)
    return np.stack(cols, axis=1)


# The brute-force near-tie cases, m -> scale of the tiny coordinate (n = 600, 2048 levels 2^-10 apart).  2^-32 gives 74 and 182
# rows in which the two orders differ at m = 30 and 84 but only 6 at m = 10, whose neighbours are closer and so have smaller
# ulps; 2^-34 gives 38 there.  The tests demand 10.
NEAR_TIE_BRUTE = {10: 2.0 ** -34, 30: 2.0 ** -32, 84: 2.0 ** -32}


def differing_rows(a, b):
    """Indices of the rows in which two arrays differ."""
    return np.nonzero((a != b).any(axis=1))[0]
