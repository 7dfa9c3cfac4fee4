"""The workgroup-per-set kernel (gpv_sets_generic.hip) against the oracle: every covariance family, the general-nu route of
its own, more than one set per workgroup, the fused sums one by one, and the edges the unrolled kernels are tested on.

Two shapes reach the kernel, the smallest that also differ in coordinate layout:
  L  m = 64 (P = 65), d = 2: packed 32-byte records (A.rec, datum in the record)
  H  m = 15, d = 9:          unpacked coordinates (A.locs, locs_ld = 9), data from A.z

What each case exists to reach:
  test_families_against_oracle          every arm of cov_runtime (COV_MATERN05 / 15 / 25 / ESQE, default = COV_MATERN_GEN), in
                                        both coordinate layouts, observed ("z") and latent ("SGV") nugget placement
  test_general_nu_regimes               cov_from_r2<COV_MATERN_GEN> -> matern_general_seg:
      folded       every s = dist/range < 4: rows that carry exp(-s) (`s < GPV_MT_FOLD_BELOW ? pv`)
      unfolded     s up to ~60: rows without exp(-s) (`pv * exp_neg(s)`); at shape H EVERY pair is there
      beyond       s beyond 512: `(unsigned)seg < mt_nseg` false -> matern_general inline, its x > 746 branch included
      coincident   r2 == 0 -> sigma^2 exactly, next to table pairs (plan creation skips zero distances when it derives
                   dist_min, so a table IS fitted here; the quadrature for every pair is the no-table test below)
  test_general_nu_table_route_equals_quadrature_route
                                        GPV_NO_MATERN_TABLE=1 in a child process: mt_nseg == 0, every pair by the quadrature;
                                        the in-table run must agree to 2e-13 and must NOT be bit-identical (no accessor shows
                                        mt_nseg: rows that differ in their last bits are the evidence that a table was fitted)
  test_more_than_one_set_per_workgroup  second and third iteration of `for (k = blockIdx.x; k < A.rows; k += gridDim.x)`: the
                                        `s_fail = 0` reset, the barriers between a set's last read of xv / s_red / loc and the
                                        next gather, acc[] over several sets; reduce_tail twice on one plan, bitwise
  test_fused_sums_one_by_one            acc[0..5] behind `A.flags & 2` and `A.flags & 4` separately; `A.Lentries == nullptr`
  test_nan_coordinate                   the `pa[t] != pa[t]` scan of the diagonal entry, through A.rec and through A.locs (last
                                        coordinate: the scan runs to A.dim, not to 3)
  test_scalar_and_vector_nuggets        `A.nuggets != nullptr ? A.nuggets[a] : A.nug_scalar`, diagonal and tau of the epilogue
  test_shards                           `kout = A.rowid[k]` with row_begin > 0; totals of two grids add up
  test_ragged_rows                      the compaction of the gather (n0 < P, holes anywhere) with the ESQE and table arms

Every case that asserts `escaped == 0` (no row beyond the flat 1e-8) depends on its INPUTS being benign: the double-precision
oracle itself must stay within 1e-8 of the extended-precision rows (oracle.r_side.rows_extended).  That was checked on the CPU
for every such case, all rows; the largest oracle error per case stands next to the case in _MARGIN below."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LL_RTOL = 1e-8
SHAPES = {"L": (64, 2), "H": (15, 9)}                 # m, d
N_ROWS = {"L": 230, "H": 260}


def _need_gpu():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


def _to_product_va(va):
    """oracle vecchia.approx (NaN = NA) -> product representation (0 / -1 = NA)."""
    prep = dict(va["U_prep"])
    prep["revNNarray"] = np.nan_to_num(prep["revNNarray"], nan=0.0).astype(np.int32)
    prep["revCond"] = np.nan_to_num(prep["revCond"], nan=-1.0).astype(np.int8)
    out = dict(va)
    out["U_prep"] = prep
    return out


def _range_rule(d):
    return 0.25 * np.sqrt(d / 2)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _setup(shape, n, seed, cond, dup=False):
    """Seeded inputs of one plan, computed once and shared read-only: locations, data, vector nuggets, vecchia.approx."""
    from oracle import r_side as R
    m, d = SHAPES[shape]
    rng = np.random.default_rng(seed)
    locs = rng.random((n, d))
    z = rng.standard_normal(n)
    tau = 0.1 + 0.1 * rng.random(n)
    if dup:                                            # every third point sits on an earlier one
        for j in range(2, n, 3):
            locs[j] = locs[rng.integers(j)]
    NN = R.findOrderedNN(locs, m)
    for j in np.where(NN[:, 0] != np.arange(1, n + 1))[0]:      # a coincident earlier point wins the tie: self back in front
        c = int(np.where(NN[j] == j + 1)[0][0])
        NN[j, 0], NN[j, c] = NN[j, c], NN[j, 0]
    va = R.vecchia_specify(locs, m, ordering="none", cond_yz=cond, NNarray=NN)
    prep = va["U_prep"]
    _freeze(locs, z, tau, va["locsord"], prep["revNNarray"], prep["revCond"])
    return locs, z, tau, va


def _esqe_cp(d):
    r = _range_rule(d)
    return [0.8, r, 0.5, 0.8 * r]


# ---- the cases compared row by row with the oracle: id -> (shape, cond, dup, covmodel, covparms) ----------------------------
def _family_cases():
    out = {}
    for shape, (m, d) in SHAPES.items():
        for nu in (0.5, 1.5, 2.5, 0.3, 1.1, 3.7):
            for cond in ("z", "SGV") if nu in (0.5, 0.3) else ("z",):
                out["%s-nu%s-%s" % (shape, nu, cond)] = (shape, cond, False, "matern", [1.3, _range_rule(d), nu])
        for cond in ("z", "SGV"):
            out["%s-esqe-%s" % (shape, cond)] = (shape, cond, False, "esqe", _esqe_cp(d))
    return out


# s = dist / range (the general-nu branch has no sqrt(2 nu) scaling, src/Matern.cpp:73-80).  Pair distances inside the
# conditioning sets of the seeded plans: L (d = 2, n = 230) 0.003 .. 1.25, H (d = 9, n = 260) 0.34 .. 1.81.  The spans of s
# below are those of ALL pairs inside the sets, measured on the CPU.
_REGIME_RANGE = {("folded", "L"): 0.4,        # s = 0.008 .. 3.1
                 ("folded", "H"): 0.8,        # s = 0.43 .. 2.3
                 ("unfolded", "L"): 0.023,    # s = 0.14 .. 55: 96 % of the pairs beyond 4, the closest ones in folded rows of the same block
                 ("unfolded", "H"): 0.036,    # s = 9.5 .. 50: every pair beyond 4
                 ("beyond", "L"): 2e-4,       # s = 16 .. 6300: 95 % of the pairs beyond 512 (89 % beyond 746), the rest in the table's last octaves
                 ("beyond", "H"): 6e-4,       # s = 570 .. 3000: every pair beyond the table, 0.3 % of them below 746
                 ("coincident", "L"): _range_rule(2),      # 8853 coincident pairs; s = 0.017 .. 4.9 for the others
                 ("coincident", "H"): _range_rule(9)}      # 2196 coincident pairs; s = 0.65 .. 3.4 for the others


def _regime_cases():
    out = {}
    for (regime, shape), rg in _REGIME_RANGE.items():
        for nu in (0.4, 2.2):
            dup = regime == "coincident"
            out["%s-%s-nu%s" % (regime, shape, nu)] = (shape, "z", dup, "matern", [1.0 if dup else 1.3, rg, nu])
    return out


FAMILY_CASES = _family_cases()
REGIME_CASES = _regime_cases()
SEED = {"L": 4101, "H": 4102}

# max over ALL rows of |oracle row - extended-precision row| / max|row| (x87 long double for the closed forms, 40-digit
# mpmath for general nu), computed on the CPU for the seeds above: the double oracle stays this far inside the 1e-8 that
# `escaped == 0` presumes.  (ragged-*: the cases of test_ragged_rows.)  The Matern 1.5 plans of
# test_more_than_one_set_per_workgroup (at 256 compute units: H n = 4133 2.0e-15 with and without the singular rows, L n = 2085
# 1.3e-14) and the rows test_nan_coordinate compares (L 1.3e-14, H 7.8e-16) were measured the same way.
_MARGIN = {
    "H-esqe-SGV": 4.8e-16,
    "H-esqe-z": 3.7e-16,
    "H-nu0.3-SGV": 4.0e-15,
    "H-nu0.3-z": 3.6e-15,
    "H-nu0.5-SGV": 4.2e-16,
    "H-nu0.5-z": 4.3e-16,
    "H-nu1.1-z": 1.2e-14,
    "H-nu1.5-z": 7.8e-16,
    "H-nu2.5-z": 9.6e-16,
    "H-nu3.7-z": 9.1e-15,
    "L-esqe-SGV": 3.5e-14,
    "L-esqe-z": 8.1e-15,
    "L-nu0.3-SGV": 1.3e-14,
    "L-nu0.3-z": 9.9e-15,
    "L-nu0.5-SGV": 1.8e-14,
    "L-nu0.5-z": 5.4e-15,
    "L-nu1.1-z": 6.7e-14,
    "L-nu1.5-z": 1.7e-14,
    "L-nu2.5-z": 2.4e-14,
    "L-nu3.7-z": 6.0e-14,
    "beyond-H-nu0.4": 7.3e-263,
    "beyond-H-nu2.2": 3.9e-258,
    "beyond-L-nu0.4": 6.8e-23,
    "beyond-L-nu2.2": 1.3e-16,
    "coincident-H-nu0.4": 1.1e-14,
    "coincident-H-nu2.2": 8.4e-15,
    "coincident-L-nu0.4": 3.5e-14,
    "coincident-L-nu2.2": 3.1e-14,
    "folded-H-nu0.4": 8.1e-15,
    "folded-H-nu2.2": 8.5e-15,
    "folded-L-nu0.4": 2.5e-14,
    "folded-L-nu2.2": 6.2e-14,
    "unfolded-H-nu0.4": 1.3e-16,
    "unfolded-H-nu2.2": 1.3e-16,
    "unfolded-L-nu0.4": 1.2e-14,
    "unfolded-L-nu2.2": 8.0e-15,
    "ragged-H-esqe": 3.7e-16,
    "ragged-H-nu1.1": 1.5e-14,
    "ragged-L-esqe": 5.4e-15,
    "ragged-L-nu1.1": 2.2e-12,
}


def _compare_with_oracle(G, shape, cond, dup, covmodel, cp, oracle_underflows=False):
    """Case 1 of the issue: failures, rows (flat 1e-8, none adjudicated), padding pattern, Zentries, log-likelihood.

    oracle_underflows (the "beyond" regime only): the oracle's K_nu (scipy.special.kv, AMOS) returns exactly 0 from s = 698 on,
    where s^nu K_nu(s) is still a NORMAL double (40-digit mpmath: K_0.4(700) = 4.7e-306, times 700^2.2 = 8e-300; kv(0.4, 700)
    = 0.0) -- the kernel's quadrature keeps these values, down to the subnormals, as the extended-precision rows do.  So the
    zero pattern INSIDE a row may differ from the oracle's there, measured on the MI355X: 10 .. 105 entries per plan.  What is
    asserted instead: the padding (columns from n0 on) is exactly zero in both, and where the two disagree inside a row the
    non-zero value is below 1e-290 (K_nu < 1e-304 beyond 697, s^nu < 3e8 at s <= 7000, and two covariances never multiply to
    more than one of them)."""
    from oracle import r_side as R
    from _parity import check_rows
    n = N_ROWS[shape]
    locs, z, tau, va = _setup(shape, n, SEED[shape], cond, dup)
    prep = va["U_prep"]
    refU = R.createU(va, cp, tau, covmodel)
    ref = refU["U_entries"]
    out = G.U_NZentries(1, n, va["locsord"], prep["revNNarray"], prep["revCond"], tau, tau, covmodel, cp)
    res = check_rows(out["Lentries"], ref["Lentries"], va["locsord"], prep["revNNarray"], prep["revCond"], tau, covmodel, cp)
    ll_ref = R.vecchia_likelihood_U(z, refU)
    ll = G.vecchia_likelihood(z, _to_product_va(va), cp, tau, covmodel)
    print("generic-kernel case", shape, cond, covmodel, cp, "failed", out["n_failed"], ref["n_failed"], res,
          "ll", ll, ll_ref, abs(ll - ll_ref) / abs(ll_ref))
    assert out["n_failed"] == ref["n_failed"] == 0
    assert res["escaped"] == 0 and res["beyond4x"] == 0, res
    if oracle_underflows:
        n0 = (~np.isnan(prep["revNNarray"])).sum(axis=1)
        pad = np.arange(prep["revNNarray"].shape[1])[None, :] >= n0[:, None]
        differ = (out["Lentries"] == 0) != (ref["Lentries"] == 0)
        print("zero pattern differs from the oracle's at", int(differ.sum()), "entries, largest",
              max(np.abs(out["Lentries"][differ]).max(initial=0.0), np.abs(ref["Lentries"][differ]).max(initial=0.0)))
        assert np.all(out["Lentries"][pad] == 0) and not differ[pad].any()
        print("  of them zero in the oracle only:", int((differ & (ref["Lentries"] == 0)).sum()))
        assert max(np.abs(out["Lentries"][differ]).max(initial=0.0), np.abs(ref["Lentries"][differ]).max(initial=0.0)) < 1e-290
    else:
        np.testing.assert_array_equal(out["Lentries"] == 0, ref["Lentries"] == 0)
    np.testing.assert_allclose(out["Zentries"], ref["Zentries"], rtol=1e-15)
    assert abs(ll - ll_ref) <= LL_RTOL * abs(ll_ref)
    return out, ref, va


@pytest.mark.parametrize("case", sorted(FAMILY_CASES))
def test_families_against_oracle(case):
    G = _need_gpu()
    assert _MARGIN[case] < 1e-9                        # a new case comes with its oracle-against-extended-precision check
    _compare_with_oracle(G, *FAMILY_CASES[case])


def _pair_s(va, rg):
    """s = dist / range of (entry i, self) for every stored entry, left-aligned like Lentries; NaN where there is none."""
    nn = va["U_prep"]["revNNarray"]
    lo = va["locsord"]
    n, p = nn.shape
    s = np.full((n, p), np.nan)
    for k in range(n):
        idx = nn[k][~np.isnan(nn[k])].astype(int) - 1
        s[k, : len(idx)] = np.sqrt(((lo[idx] - lo[idx[-1]]) ** 2).sum(axis=1)) / rg
    return s


@pytest.mark.parametrize("case", sorted(REGIME_CASES))
def test_general_nu_regimes(case):
    G = _need_gpu()
    from oracle import r_side as R
    shape, cond, dup, covmodel, cp = REGIME_CASES[case]
    assert _MARGIN[case] < 1e-9
    regime = case.split("-")[0]
    out, ref, va = _compare_with_oracle(G, shape, cond, dup, covmodel, cp, oracle_underflows=regime == "beyond")
    n = N_ROWS[shape]
    if regime == "beyond":
        # x_i of a row is -cov(i, self) / ((sigma^2 + tau_i) sqrt(sigma^2)) to first order; the higher orders are products of
        # covariances along a path from i to self, no longer than the direct one (triangle inequality) up to a polynomial
        # factor of at most ~1e12 (65 points, s^nu at s = 7000).  A pair with s > 550 has cov < 1.3 e^-550 s^(nu - 1/2)
        # < 1e-230: its entry is finite and below 1e-200, and essentially the whole row is the unit row.
        s = _pair_s(va, cp[1])
        far = s > 550.0
        far[np.arange(n), (~np.isnan(s)).sum(axis=1) - 1] = False          # (self: s = 0 anyway)
        L = out["Lentries"]
        print("beyond:", case, "far entries", int(far.sum()), "of", int((~np.isnan(s)).sum()) - n, "beyond 746:",
              int((s > 746).sum()), "max |entry|", np.abs(L[far]).max(), "oracle's", np.abs(ref["Lentries"][far]).max())
        assert far.sum() > 0.5 * ((~np.isnan(s)).sum() - n) and (s > 746.0).sum() > 0
        assert np.isfinite(L).all()
        assert np.abs(L[far]).max() < 1e-200
    if regime == "coincident":
        # sigma^2 EXACTLY: with sigma^2 = 1 a set {q, k} of two coincident points, both latent, has the pivots 1 and
        # 1 - c^2: the block fails (zero row, counted) if and only if the kernel's c = cov(q, k) is exactly 1.0
        locs, z, tau, _ = _setup(shape, n, SEED[shape], cond, dup)
        prep = va["U_prep"]
        lo = va["locsord"]
        k = next(j for j in range(2, n, 3) if j > 20)
        q = int(np.where((lo[:k] == lo[k]).all(axis=1))[0][0])
        rn = np.nan_to_num(prep["revNNarray"], nan=0.0)
        rc = prep["revCond"].copy()
        rn[k] = 0; rn[k, -2:] = [q + 1, k + 1]
        rc[k] = np.nan; rc[k, -2:] = 1
        ref2 = R.U_NZentries(1, n, lo, rn, rc, tau, tau, covmodel, cp)
        out2 = G.U_NZentries(1, n, lo, rn, rc, tau, tau, covmodel, cp)
        assert out2["n_failed"] == ref2["n_failed"] == 1
        assert np.all(out2["Lentries"][k] == 0)
        keep = np.arange(n) != k
        np.testing.assert_array_equal(out2["Lentries"][keep], out["Lentries"][keep])     # the other sets: untouched, bitwise


# ---- the same plans without a table: a fresh process, every pair by the quadrature ------------------------------------------
_NO_TABLE_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
import numpy as np
import gpvecchia_amd as G
d = np.load({inp!r})
res = {{}}
for key in [str(k) for k in d["keys"]]:
    plan = G.Plan(d[key + "/locs"], d[key + "/nn"], d[key + "/cd"])
    plan.set_data(d[key + "/z"])
    plan.eval("matern", d[key + "/cp"], d[key + "/tau"], G.GPV_WANT_LOGLIK_Z | G.GPV_WANT_U)
    res[key + "/L"] = plan.Lentries()
    res[key + "/ll"] = np.array(G.loglik_z_from_sums(plan.sums(), plan.Nlocs))
np.savez({outp!r}, **res)
print("NO_TABLE_CHILD done")
"""


def test_general_nu_table_route_equals_quadrature_route(tmp_path):
    G = _need_gpu()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data, here = {}, {}
    keys = [c for c in sorted(REGIME_CASES) if c.split("-")[0] in ("folded", "unfolded")]
    for key in keys:
        shape, cond, dup, covmodel, cp = REGIME_CASES[key]
        n = N_ROWS[shape]
        locs, z, tau, va = _setup(shape, n, SEED[shape], cond, dup)
        pva = _to_product_va(va)
        nn, cd = pva["U_prep"]["revNNarray"], pva["U_prep"]["revCond"]
        for name, v in (("locs", va["locsord"]), ("nn", nn), ("cd", cd), ("z", z), ("tau", tau), ("cp", np.array(cp))):
            data[key + "/" + name] = v
        plan = G.Plan(va["locsord"], nn, cd)
        plan.set_data(z)
        plan.eval("matern", cp, tau, G.GPV_WANT_LOGLIK_Z | G.GPV_WANT_U)
        here[key] = (plan.Lentries(), G.loglik_z_from_sums(plan.sums(), n))
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, keys=np.array(keys), **data)
    r = subprocess.run([sys.executable, "-c", _NO_TABLE_CHILD.format(root=root, inp=inp, outp=outp)], capture_output=True,
                       text=True, env=dict(os.environ, GPV_NO_MATERN_TABLE="1"), timeout=300)
    assert r.returncode == 0 and "NO_TABLE_CHILD done" in r.stdout, r.stderr[-2000:]
    child = np.load(outp)
    for key in keys:
        L, ll = here[key]
        Lq, llq = child[key + "/L"], float(child[key + "/ll"])
        print("table vs quadrature", key, "ll", abs(ll - llq) / abs(llq), "sum|L|", abs(np.abs(L).sum() - np.abs(Lq).sum())
              / np.abs(Lq).sum(), "entries that differ", int((L != Lq).sum()))
        assert abs(ll - llq) <= 2e-13 * abs(llq), (key, ll, llq)
        assert abs(np.abs(L).sum() - np.abs(Lq).sum()) <= 2e-13 * np.abs(Lq).sum(), key
        assert not np.array_equal(L, Lq), (key, "bit-identical to the quadrature route: no table was fitted for this plan")


# ---- more than one set per workgroup ------------------------------------------------------------------------------------------
def _stored_order(locs):
    """Mirror of gpv_plan_create's set order: the sets are processed in the Morton order (21 bits per coordinate, the first
    three coordinates, coordinate 0 most significant) of the point they belong to, ties by index."""
    n, d = locs.shape
    kd = min(d, 3)
    q = np.zeros((n, kd), dtype=np.uint64)
    for t in range(kd):
        col = locs[:, t]
        ok = ~np.isnan(col)
        mn, mx = col[ok].min(), col[ok].max()
        sc = 2097151.0 / (mx - mn) if mx > mn else 0.0
        v = (col - mn) * sc
        v = np.where(ok & (v > 0), np.minimum(v, 2097151.0), 0.0)
        q[:, t] = v.astype(np.uint64)
    key = np.zeros(n, dtype=np.uint64)
    for bit in range(20, -1, -1):
        for t in range(kd):
            key = (key << np.uint64(1)) | ((q[:, t] >> np.uint64(bit)) & np.uint64(1))
    return np.argsort(key, kind="stable")             # order[k] = row served as stored set k


def _make_singular(locs, revNN, revCond, anchor):
    """Row anchor + 1 moves onto point `anchor` and conditions on it as latent: a singular 2 x 2 block (as
    test_generic_kernel_edges does for its row 150)."""
    r = anchor + 1
    locs[r] = locs[anchor]
    revNN[r] = 0; revNN[r, -2:] = [anchor + 1, r + 1]
    revCond[r] = np.nan; revCond[r, -2:] = 1
    return r


@pytest.mark.parametrize("shape,sets_per_wg,singular", [("H", 2, False), ("H", 2, True), ("L", 1, True)])
def test_more_than_one_set_per_workgroup(shape, sets_per_wg, singular):
    G = _need_gpu()
    import torch
    from oracle import r_side as R
    from _parity import check_rows
    grid = 8 * torch.cuda.get_device_properties(0).multi_processor_count      # the cap of launch_sets_generic
    n = sets_per_wg * grid + 37
    m, d = SHAPES[shape]
    rng = np.random.default_rng(4200 + sets_per_wg)
    locs = rng.random((n, d))
    z = rng.standard_normal(n)
    tau = 0.1 + 0.1 * rng.random(n)
    cp = [1.3, _range_rule(d), 1.5]
    # nearest earlier points by brute force on blocks of rows (the oracle's findOrderedNN walks row by row: seconds here)
    revNN = np.zeros((n, m + 1))
    sq = (locs ** 2).sum(axis=1)
    for a in range(0, n, 512):
        b = min(a + 512, n)
        D = sq[a:b, None] + sq[None, :b] - 2.0 * locs[a:b] @ locs[:b].T
        D[np.arange(b - a)[:, None] < np.arange(b)[None, :] - a] = np.inf    # later points
        D[np.arange(b - a), np.arange(a, b)] = -np.inf                        # self in front
        o = np.argsort(D, axis=1, kind="stable")[:, : m + 1]
        for j in range(a, b):
            c = min(m + 1, j + 1)
            revNN[j, m + 1 - c:] = o[j - a, :c][::-1] + 1                     # right-aligned, farthest first, self last
    revCond = np.where(revNN != 0, 0.0, np.nan)
    revCond[:, -1] = 1                                                        # cond.yz = "z"
    bad = []
    if singular:
        order0 = _stored_order(locs)
        taken = set()
        for start in (20, sets_per_wg * grid + 18):
            k0 = next(k for k in range(start, start + 12) if order0[k] + 1 < n and not {order0[k], order0[k] + 1} & taken)
            bad.append(_make_singular(locs, revNN, revCond, int(order0[k0])))
            taken |= {bad[-1] - 1, bad[-1]}
        order = _stored_order(locs)
        pos = np.empty(n, dtype=np.int64)
        pos[order] = np.arange(n)
        # the failing set is the FIRST of its workgroup for one row, the LAST for the other; the sets before / after it in
        # the same workgroup (stored position -+ grid) are whole rows that must be right
        assert pos[bad[0]] < min(grid, 37) and pos[bad[1]] >= sets_per_wg * grid, (pos[bad], grid)
        mates = [order[pos[bad[0]] + t * grid] for t in range(1, sets_per_wg + 1)]
        mates += [order[pos[bad[1]] - t * grid] for t in range(1, sets_per_wg + 1)]
        assert not set(mates) & set(bad)
    ref = R.U_NZentries(1, n, locs, revNN, revCond, tau, tau, "matern", cp)
    assert ref["n_failed"] == len(bad)
    plan = G.Plan(locs, revNN, revCond)
    plan.set_data(z)
    flags = G.GPV_WANT_LOGLIK_Z | G.GPV_WANT_NUMERATOR | G.GPV_WANT_U
    plan.eval("matern", cp, tau, flags)
    s1, L1 = plan.sums(), plan.Lentries()
    plan.eval("matern", cp, tau, flags)
    s2, L2 = plan.sums(), plan.Lentries()
    np.testing.assert_array_equal(s1, s2)                                    # reduce_tail hand-off: bitwise
    np.testing.assert_array_equal(L1, L2)
    assert s1[6] == ref["n_failed"] and s1[7] == n, s1
    np.testing.assert_array_equal(L1 == 0, ref["Lentries"] == 0)
    good = np.setdiff1d(np.arange(n), bad)
    res = check_rows(L1[good], ref["Lentries"][good], locs, revNN, revCond, tau, "matern", cp, rows=good)
    print("sets per workgroup", shape, n, grid, "bad rows", bad, res, "sums", s1)
    assert res["escaped"] == 0 and res["beyond4x"] == 0, res
    if singular:
        assert np.all(L1[bad] == 0)
        for r in mates:
            assert np.abs(L1[r]).max() > 0.1, r                               # (the diagonal entry is 1/sqrt of a variance ~ 1)
    # acc[] over ALL the sets of every workgroup: the totals from the oracle's rows (a failed set contributes to none)
    np.testing.assert_allclose(s1[:6], _sums_from_rows(revNN[good], revCond[good], ref["Lentries"][good], z, tau, good), rtol=1e-9)


def _map_sums(s):
    """acc[0..5] of gpv_sets_generic.hip from the six sums of oracle.r_side.separable_loglik_condz (d the diagonal entry of
    a row, a its observed part times the data, w = d^2 + 1/tau):
        acc[0] = sum log d = s[0]      acc[1] = sum a^2 = s[3]      acc[4] = sum z^2 / tau = s[4]      acc[5] = sum log tau = s[1]
        acc[2] = sum log(tau + 1/d^2) = s[1] + s[2] - 2 s[0]              (tau + 1/d^2 = tau w / d^2)
        acc[3] = sum (z + a/d)^2 / (tau + 1/d^2) = s[3] + s[4] - s[5]      ((d z + a)^2 = a^2 tau w + z^2 w - tau (d a - z/tau)^2)
    The two differences lose one digit here (log tau and z^2 / tau are ten times the result): far inside 1e-9."""
    return np.array([s[0], s[3], s[1] + s[2] - 2 * s[0], s[3] + s[4] - s[5], s[4], s[1]])


def _sums_from_rows(nn, cd, Lrows, z, tau, rows):
    """The per-row terms of oracle.r_side.separable_loglik_condz for the rows `rows` only (it takes whole plans: a plan with
    failed rows has log 0 in them), mapped to acc[0..5]."""
    s = np.zeros(6)
    for t, k in enumerate(rows):
        ok = ~np.isnan(nn[t]) & (nn[t] != 0)
        n0 = int(ok.sum())
        idx = nn[t, ok].astype(np.int64) - 1
        c = cd[t, -n0:]
        M = Lrows[t, :n0]
        d = M[n0 - 1]
        a = float(np.sum(M[: n0 - 1] * z[idx[: n0 - 1]] * (c[: n0 - 1] == 0)))
        w = d * d + 1.0 / tau[k]
        s += [np.log(d), np.log(tau[k]), np.log(w), a * a, z[k] ** 2 / tau[k], (d * a - z[k] / tau[k]) ** 2 / w]
    return _map_sums(s)


# ---- the eight fused sums, one by one --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["L", "H"])
def test_fused_sums_one_by_one(shape):
    G = _need_gpu()
    from oracle import r_side as R
    n = N_ROWS[shape]
    locs, z, tau, va = _setup(shape, n, SEED[shape], "z")
    cp = [1.3, _range_rule(SHAPES[shape][1]), 1.5]
    ref = R.createU(va, cp, tau)["U_entries"]
    assert ref["n_failed"] == 0
    _, s_ref = R.separable_loglik_condz(va, ref, z, tau)
    want = _map_sums(s_ref)
    pva = _to_product_va(va)
    plan = G.Plan(pva["locsord"], pva["U_prep"]["revNNarray"], pva["U_prep"]["revCond"])
    plan.set_data(z[va["ord_z"] - 1])
    by_flag = {G.GPV_WANT_LOGLIK_Z: (2, 3), G.GPV_WANT_NUMERATOR: (0, 1, 4, 5)}
    for flags in (G.GPV_WANT_LOGLIK_Z, G.GPV_WANT_NUMERATOR, G.GPV_WANT_LOGLIK_Z | G.GPV_WANT_NUMERATOR):
        plan.eval("matern", cp, tau[va["ord"] - 1], flags)
        s = plan.sums()
        print("fused sums", shape, flags, s, want)
        assert s[6] == 0 and s[7] == n
        for f, which in by_flag.items():
            for t in which:
                if flags & f:
                    np.testing.assert_allclose(s[t], want[t], rtol=1e-9, err_msg="sum %d, flags %d" % (t, flags))
                else:
                    assert s[t] == 0.0, (t, flags, s[t])                       # not requested: exactly zero


# ---- edges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["L", "H"])
def test_nan_coordinate(shape):
    G = _need_gpu()
    from oracle import r_side as R
    from _parity import check_rows
    n = N_ROWS[shape]
    m, d = SHAPES[shape]
    locs, z, tau, va = _setup(shape, n, SEED[shape], "z")           # neighbours from the clean coordinates
    prep = va["U_prep"]
    lnan = va["locsord"].copy()
    j = 100
    lnan[j, d - 1] = np.nan                                           # the LAST coordinate: column 8 of A.locs at shape H
    cp = [1.3, _range_rule(d), 1.5]
    ref = R.U_NZentries(1, n, lnan, np.nan_to_num(prep["revNNarray"]), prep["revCond"], tau, tau, "matern", cp)
    out = G.U_NZentries(1, n, lnan, prep["revNNarray"], prep["revCond"], tau, tau, "matern", cp)
    hit = (prep["revNNarray"] == j + 1).any(axis=1)                   # exactly the sets that contain the point
    assert 1 < hit.sum() < n
    assert out["n_failed"] == ref["n_failed"] == hit.sum()
    np.testing.assert_array_equal((out["Lentries"] == 0).all(axis=1), hit)
    np.testing.assert_array_equal(out["Lentries"] == 0, ref["Lentries"] == 0)
    good = np.where(~hit)[0]
    res = check_rows(out["Lentries"][good], ref["Lentries"][good], lnan, prep["revNNarray"], prep["revCond"], tau, "matern", cp,
                     rows=good)
    assert res["escaped"] == 0 and res["beyond4x"] == 0, res
    # and through the plan: counted in the totals
    plan = G.Plan(lnan, prep["revNNarray"], prep["revCond"])
    plan.set_data(z)
    plan.eval("matern", cp, tau, G.GPV_WANT_LOGLIK_Z | G.GPV_WANT_U)
    s = plan.sums()
    assert s[6] == hit.sum() and s[7] == n


@pytest.mark.parametrize("shape", ["L", "H"])
def test_scalar_and_vector_nuggets(shape):
    G = _need_gpu()
    n = N_ROWS[shape]
    locs, z, tau, va = _setup(shape, n, SEED[shape], "z")
    prep = va["U_prep"]
    cp = [1.3, _range_rule(SHAPES[shape][1]), 1.5]
    flags = G.GPV_WANT_LOGLIK_Z | G.GPV_WANT_NUMERATOR | G.GPV_WANT_U
    got = []
    for nug in (0.15, np.full(n, 0.15)):
        plan = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
        plan.set_data(z)
        plan.eval("matern", cp, nug, flags)
        got.append((plan.sums(), plan.Lentries()))
    assert got[0][0][6] == 0 and got[0][0][7] == n and np.abs(got[0][1]).max() > 0.1
    np.testing.assert_array_equal(got[0][0], got[1][0])
    np.testing.assert_array_equal(got[0][1], got[1][1])


@pytest.mark.parametrize("nu", [1.5, 1.1])
def test_shards(nu):
    # two shards of a shape-H plan (split as test_sharded_plans_add_up splits): the rows land at A.rowid[k] of their shard
    G = _need_gpu()
    n = N_ROWS["H"]
    locs, z, tau, va = _setup("H", n, SEED["H"], "z")
    prep = va["U_prep"]
    cp = [1.3, _range_rule(9), nu]
    flags = G.GPV_WANT_LOGLIK_Z | G.GPV_WANT_NUMERATOR | G.GPV_WANT_U
    full = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
    full.set_data(z)
    full.eval("matern", cp, tau, flags)
    s_full, L_full = full.sums(), full.Lentries()
    assert s_full[6] == 0 and s_full[7] == n and (np.abs(L_full).max(axis=1) > 0.1).all()
    tot = np.zeros(8)
    cuts = [0, 131, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        pl = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"], row_begin=a, row_end=b)
        pl.set_data(z)
        pl.eval("matern", cp, tau, flags)
        s = pl.sums()
        assert s[7] == b - a
        tot += s
        np.testing.assert_array_equal(pl.Lentries(), L_full[a:b])      # same kernel, same sets: bit-identical
    np.testing.assert_allclose(tot, s_full, rtol=1e-12)


def _ragged(shape, seed):
    """Rows with missing entries anywhere and random latent / observed flags (src/U_NZentries.cpp:44-47), as
    test_generic_kernel_edges builds them."""
    m, d = SHAPES[shape]
    p, n = m + 1, N_ROWS[shape]
    rng = np.random.default_rng(seed)
    locs = rng.random((n, d))
    revNN = np.zeros((n, p)); revCond = np.full((n, p), np.nan)
    for k in range(n):
        cand = rng.permutation(k)[: min(k, p - 1)] + 1
        keep = cand[rng.random(len(cand)) < 0.8]
        row = np.zeros(p)
        pos = np.sort(rng.choice(p - 1, size=len(keep), replace=False)) if len(keep) else np.array([], int)
        row[pos] = keep
        row[p - 1] = k + 1
        revNN[k] = row
        n0 = int((row != 0).sum())
        c = (rng.random(n0) < 0.5).astype(float); c[-1] = 1
        revCond[k, p - n0:] = c
    tau = 0.1 + rng.random(n)
    return locs, revNN, revCond, tau


RAGGED_CASES = {"ragged-%s-%s" % (shape, name): (shape, covmodel, cp)
                for shape in ("L", "H")
                for name, covmodel, cp in (("esqe", "esqe", _esqe_cp(SHAPES[shape][1])),
                                           ("nu1.1", "matern", [1.0, _range_rule(SHAPES[shape][1]), 1.1]))}


@pytest.mark.parametrize("case", sorted(RAGGED_CASES))
def test_ragged_rows(case):
    G = _need_gpu()
    from oracle import r_side as R
    from _parity import check_rows
    shape, covmodel, cp = RAGGED_CASES[case]
    assert _MARGIN[case] < 1e-9
    n = N_ROWS[shape]
    locs, revNN, revCond, tau = _ragged(shape, 4300)
    ref = R.U_NZentries(1, n, locs, revNN, revCond, tau, tau, covmodel, cp)
    out = G.U_NZentries(1, n, locs, revNN, revCond, tau, tau, covmodel, cp)
    res = check_rows(out["Lentries"], ref["Lentries"], locs, revNN, revCond, tau, covmodel, cp)
    print("ragged", case, out["n_failed"], ref["n_failed"], res)
    assert out["n_failed"] == ref["n_failed"] == 0
    assert res["escaped"] == 0 and res["beyond4x"] == 0, res
    np.testing.assert_array_equal(out["Lentries"] == 0, ref["Lentries"] == 0)
