"""gpv_plan_set_blocks / gpv_plan_block_cv (gpv_blockcv.hip) on the GPU: leave-block-out cross-validation by per-block precision
solves, and what is built on it (vecchia_block_cv, vecchia_estimate(block_cv=...)).

Truth: tests/_blockcv_truth.py, Q = T'T from the long-double rows of tests/_loo_truth.py, Q_BB cut out and inverted by the
written-out Cholesky, independent of Lentries.  Bars (the project's flat 1e-8, tests/_parity.py), in the norms of
tests/test_gpu_loo.py:
  mean      per column: max |got - truth| <= 1e-8 max(max |truth|, max |z|) over the held-out locations
  var       per entry, relative
  sums      |got - truth| <= 1e-8 sum |term|; the coverage count exactly (every test asserts that the truth's margin
            ||s| - 1.96| exceeds 1e-8 and prints it)
Why 1e-8 is safe: for the exact GP precision of these 600 points and families cond(Q_BB) <= 2.2e2 for 64-point strips,
bisection cells and random blocks and cond(Q) <= 3.8e3, so b cond eps is about 3e-11.
Inputs: the plans and columns of tests/test_gpu_whiten.py (case, SHAPES, _plan), n = 600 unless said.  Every test prints its
worst measured figures."""
import ctypes as C
import functools

import numpy as np
import pytest

import _blockcv_truth as BT
import test_gpu_loo as TL
import test_gpu_whiten as TW

pytestmark = pytest.mark.gpu

TOL = 1e-8
TAU = 0.1
LD = np.longdouble


def _need_gpu():
    return TL._need_gpu()


# ---- block shapes: labels of the ORDERED rows ------------------------------------------------------------------------------
def strips(c):
    """(a) sorted on the first coordinate, chunks of 64: 600 = 9 x 64 + 24, the full size and a partial one"""
    lab = np.empty(c["n"], dtype=np.int32)
    lab[np.argsort(c["va"]["locsord"][:, 0], kind="stable")] = np.arange(c["n"]) // 64
    return lab


def cells(c):
    """(b)"""
    import gpvecchia_amd as G
    return G.spatial_blocks(c["va"]["locsord"]).astype(np.int32)


def scattered(c, seed=31):
    """(c) 64 scattered members per block"""
    lab = np.empty(c["n"], dtype=np.int32)
    lab[np.random.default_rng(seed).permutation(c["n"])] = np.arange(c["n"]) // 64
    return lab


def mixed(c, seed=32):
    """(d) sizes 1, 2, 63, 64 (scattered), every other location kept"""
    perm = np.random.default_rng(seed).permutation(c["n"])
    lab = np.full(c["n"], -1, dtype=np.int32)
    lab[perm[:1]], lab[perm[1:3]], lab[perm[3:66]], lab[perm[66:130]] = 3, 0, 17, 5
    return lab


def one_block(c):
    """(e) the first strip alone"""
    lab = strips(c)
    return np.where(lab == 0, 0, -1).astype(np.int32)


BLOCKS = dict(strips=strips, cells=cells, scattered=scattered, mixed=mixed, one=one_block)


@functools.lru_cache(maxsize=None)
def _Q(key):
    c, t = TL.truth(**dict(key))
    Q = BT.precision_ld(t["F"], c["n"])
    Q.setflags(write=False)
    return Q


_TRUTHS = {}


def truth(kw, lab, Z=None):
    """the long-double truth of a labelling on the case's 16 columns, computed once and shared read-only"""
    key = (TL._key(kw), np.asarray(lab, dtype=np.int64).tobytes(), None if Z is None else Z.tobytes())
    if key not in _TRUTHS:
        c, _ = TL.truth(**kw)
        _TRUTHS[key] = BT.from_Q(_Q(TL._key(kw)), c["Bord"] if Z is None else Z, lab)
    return _TRUTHS[key]


def check(got, t, Z, ncols, what):
    """the bars of the module docstring on the first ncols columns; got = Plan.block_cv's result.  Returns the worst figures."""
    mean, var, scores, nf, nbad = got
    held = ~np.isnan(t["var"].astype(np.float64))
    assert nf == 0 and nbad == 0 and scores.shape == (ncols, 8)
    assert np.all(np.isnan(mean[~held])) and np.all(np.isnan(var[~held])), what
    assert np.all(np.isfinite(mean[held])) and np.all(var[held] > 0), what
    want = t["mean"][held][:, :ncols]
    scale = np.maximum(np.abs(want).max(axis=0).astype(np.float64), np.abs(Z[:, :ncols]).max(axis=0))
    em = float((np.abs(mean[held] - want.astype(np.float64)).max(axis=0) / scale).max())
    ev = float((np.abs(var[held] - t["var"][held].astype(np.float64)) / t["var"][held].astype(np.float64)).max())
    ws, sabs = t["scores"][:ncols].astype(np.float64), t["sabs"][:ncols].astype(np.float64)
    idx = [0, 1, 2, 3, 4, 6, 7]
    es = float((np.abs(scores[:, idx] - ws[:, idx]) / sabs[:, idx]).max())
    margin = float(t["margin"])
    print(f"{what}: mean {em:.2e} (column max norm), var {ev:.2e} (per entry), sums {es:.2e} of sum|term|, coverage "
          f"{scores[:, 5].astype(int).tolist()} of {t['n_heldout']}, margin {margin:.2e}")
    assert margin > TOL, (what, margin)
    assert em <= TOL and ev <= TOL and es <= TOL, (what, em, ev, es)
    assert np.array_equal(scores[:, 5], ws[:, 5]), (what, scores[:, 5], ws[:, 5])
    return em, ev, es


def run(plan, c, kw, lab, ncols, what):
    counts = plan.set_blocks(lab)
    sizes = np.bincount(lab[lab >= 0])
    assert counts[:3] == (int((sizes > 0).sum()), int(sizes.sum()), int(sizes.max())), (what, counts)
    got = plan.block_cv(c["Bord"][:, :ncols])
    check(got, truth(kw, lab), c["Bord"], ncols, what)
    return got


@pytest.mark.parametrize("ncols", [16, 3, 1])
@pytest.mark.parametrize("m", [0, 1, 15, 31, 70])
def test_block_shapes(m, ncols):
    G = _need_gpu()
    kw = dict(m=m)
    c, _ = TL.truth(**kw)
    plan = TW._plan(G, c)
    for name, make in BLOCKS.items():
        run(plan, c, kw, make(c), ncols, f"m={m} ncols={ncols} {name}")


@pytest.mark.parametrize("name", list(TW.SHAPES))
def test_plan_shapes(name):
    G = _need_gpu()
    kw = TW.SHAPES[name]
    c, _ = TL.truth(**kw)
    plan = TW._plan(G, c)
    n = c["n"]
    if name == "n3":
        labs = {"all three": np.zeros(3, dtype=np.int32), "2 + 1": np.array([1, 0, 1], dtype=np.int32)}
    else:
        labs = {"cells": cells(c), "scattered": scattered(c)}
    if name == "coincident":
        o = c["va"]["ord_z"] - 1
        pair = np.where((o == n // 2) | (o == n // 3))[0]              # the ordered rows of the two coincident points
        assert pair.size == 2 and np.array_equal(c["va"]["locsord"][pair[0]], c["va"]["locsord"][pair[1]])
        together = np.full(n, -1, dtype=np.int32)
        together[pair] = 4
        split = strips(c)
        split[pair[0]], split[pair[1]] = 10, 11                        # (600 = 9 x 64 + 24: the strips end at label 9)
        labs.update({"the pair as one block": together, "the pair split over two blocks": split})
    for what, lab in labs.items():
        for ncols in (16, 3):
            run(plan, c, kw, lab, ncols, f"{name} ncols={ncols} {what}")


def test_blocks_of_one_are_leave_one_out():
    """against the shipped Plan.loo on the same columns, not the truth"""
    G = _need_gpu()
    kw = dict(m=31)
    c, t = TL.truth(**kw)
    plan = TW._plan(G, c)
    n, Z = c["n"], c["Bord"]
    assert plan.set_blocks(np.arange(n)[::-1].astype(np.int32))[:3] == (n, n, 1)
    mean, var, sc, nf, nbad = plan.block_cv(Z)
    lm, lv, ls, _ = plan.loo(Z)
    scale = np.maximum(np.abs(lm).max(axis=0), np.abs(Z).max(axis=0))
    em = float((np.abs(mean - lm).max(axis=0) / scale).max())
    ev = float((np.abs(var - lv) / lv).max())
    sabs = t["loo"]["sabs"].astype(np.float64)
    es = float((np.abs(sc[:, :5] - ls[:, :5]) / sabs[:, :5]).max())
    e6 = float((np.abs(sc[:, 6] - ls[:, 2]) / sabs[:, 2]).max())
    e7 = float((np.abs(sc[:, 7] - ls[:, 3]) / sabs[:, 3]).max())
    print(f"blocks of one against Plan.loo: mean {em:.2e}, var {ev:.2e}, sums {es:.2e}, [6] against [2] {e6:.2e}, "
          f"[7] against [3] {e7:.2e}, margin {float(t['loo']['margin']):.2e}")
    assert nf == 0 and nbad == 0 and max(em, ev, es, e6, e7) <= TOL
    assert float(t["loo"]["margin"]) > TOL and np.array_equal(sc[:, 5], ls[:, 5])


def test_one_block_of_everything_is_the_likelihood():
    G = _need_gpu()
    c = TW.case(15, n=64)
    n, Z = 64, c["Bord"]
    prep = c["va"]["U_prep"]
    plan = G.Plan(c["va"]["locsord"], prep["revNNarray"], prep["revCond"])
    plan.set_data(np.ascontiguousarray(Z[:, 0]))
    plan.eval(c["cm"], c["cp"], c["tau_ord"], G.GPV_WANT_U | G.GPV_WANT_LOGLIK_Z)
    assert plan.set_blocks(np.zeros(n, dtype=np.int32))[:3] == (1, n, n)
    mean, var, sc, nf, nbad = plan.block_cv(Z)
    em = float((np.abs(mean).max(axis=0) / np.abs(Z).max(axis=0)).max())
    joint = -0.5 * (n * np.log(2 * np.pi) + sc[0, 7] + sc[0, 6])
    ll = G.loglik_z_from_sums(plan.sums(), n)
    print(f"one block of all {n}: prior mean {em:.2e} of max |z|, joint density {joint:.12g} against loglik {ll:.12g} "
          f"({abs(joint - ll) / abs(ll):.2e} relative)")
    assert nf == 0 and nbad == 0 and em <= TOL and np.all(var > 0)
    assert abs(joint - ll) <= TOL * abs(ll)
    assert np.all(sc[:, 7] == sc[0, 7])


def _same(a, b):
    for u, v in zip(a, b):
        assert (u.tobytes() == v.tobytes()) if isinstance(u, np.ndarray) else u == v


def test_bits():
    G = _need_gpu()
    kw = dict(m=31)
    c, t = TL.truth(**kw)
    va, prep = c["va"], c["va"]["U_prep"]
    plan = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
    plan.set_data(np.ascontiguousarray(c["Bord"][:, 0]))
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U | G.GPV_WANT_LOGLIK_Z)
    Z = c["Bord"]
    sums, Lent = plan.sums(), plan.Lentries()
    w0, l0 = plan.whiten(Z, want_E=True), plan.loo(Z)
    lab = cells(c)
    plan.set_blocks(lab)
    a = plan.block_cv(Z)
    plan.block_cv(Z[:, :5])                            # another padded width in between
    _same(a, plan.block_cv(Z))                         # the same call twice
    for col in (0, 7, 15):                             # column c of a 16-column call is a one-column call, bit for bit
        one = plan.block_cv(Z[:, col])
        assert one[0][:, 0].tobytes() == a[0][:, col].tobytes() and one[1].tobytes() == a[1].tobytes()
        assert one[2][0].tobytes() == a[2][col].tobytes()
    three = plan.block_cv(Z[:, 5:8])
    assert three[0].tobytes() == np.asfortranarray(a[0][:, 5:8]).tobytes() and three[2].tobytes() == a[2][5:8].tobytes()
    # a block's mean and variance do not depend on the other blocks: relabelled, merged, split, or gone
    keep = lab == 3
    ids = np.unique(lab)
    relabel = (ids.max() - lab).astype(np.int32)
    merged = np.where(keep, 3, np.where(lab < 3, -1, 500 + np.arange(c["n"]) % 8)).astype(np.int32)   # 8 scattered blocks, some kept
    assert np.bincount(merged[merged >= 0]).max() <= 64
    split = np.arange(c["n"], dtype=np.int32)                                                          # the others: blocks of one
    split[keep] = np.where(keep)[0][0]
    alone = np.where(keep, 0, -1).astype(np.int32)
    for what, other in (("relabelled", relabel), ("merged", merged), ("split", split), ("alone", alone)):
        assert np.array_equal(other == other[np.where(keep)[0][0]], keep), what
        plan.set_blocks(other)
        b = plan.block_cv(Z)
        assert b[0][keep].tobytes() == a[0][keep].tobytes() and b[1][keep].tobytes() == a[1][keep].tobytes(), what
    # the plan's last evaluation and what whiten and loo left are what they were
    assert np.array_equal(plan.sums(), sums) and np.array_equal(plan.Lentries(), Lent)
    w1, l1 = plan.whiten(Z, want_E=True), plan.loo(Z)
    assert w0[0].tobytes() == w1[0].tobytes() and w0[1] == w1[1] and w0[3].tobytes() == w1[3].tobytes()
    _same(l0, l1)
    print("bits: repeat, column independence, block independence (relabelled, merged, split, alone), state intact")


def test_leading_dimensions_and_null_outputs():
    G = _need_gpu()
    from gpvecchia_amd import _lib as L
    kw = dict(m=15)
    c, _ = TL.truth(**kw)
    plan = TW._plan(G, c)
    lab = mixed(c)
    plan.set_blocks(lab)
    n, nc, pad = c["n"], 3, 7
    Zbig = np.full((n + pad, nc), np.nan, order="F")
    Zbig[:n] = c["Bord"][:, :nc]
    M, var, sc = np.full((n + pad + 2, nc), -7.0, order="F"), np.full(n + 1, -7.0), np.full((nc + 1, 8), -7.0)
    nf, nbad = C.c_int64(-1), C.c_int64(-1)
    raw = L.lib().gpv_plan_block_cv
    assert raw(plan._h, L.dptr(Zbig), n + pad, nc, L.dptr(M), n + pad + 2, L.dptr(var), L.dptr(sc), C.byref(nf), C.byref(nbad)) == 0
    assert np.all(M[n:] == -7.0) and var[n] == -7.0 and np.all(sc[nc] == -7.0)
    check((M[:n], var[:n], sc[:nc], nf.value, nbad.value), truth(kw, lab), c["Bord"], nc, "padded leading dimensions")
    sc2 = np.zeros((nc, 8))
    assert raw(plan._h, L.dptr(Zbig), n + pad, nc, None, 0, None, L.dptr(sc2), C.byref(nf), C.byref(nbad)) == 0
    assert sc2.tobytes() == sc[:nc].tobytes()
    mean, v2, sc3, _, _ = plan.block_cv(c["Bord"][:, :nc], want_mean=False, want_var=False)
    assert mean is None and v2 is None and sc3.tobytes() == sc2.tobytes()


def test_refusals():
    G = _need_gpu()
    from gpvecchia_amd import _lib as L
    kw = dict(m=15)
    c, _ = TL.truth(**kw)
    va, prep, n, B = c["va"], c["va"]["U_prep"], c["n"], c["Bord"]
    guard = -7.0
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731

    def cv(plan, ncols=3, ldz=None, ldm=None):
        """straight at the C ABI: the status, and whether anything was written"""
        O, v, sc = np.full((n, 17), guard, order="F"), np.full(n, guard), np.full((17, 8), guard)
        nf, nbad = C.c_int64(-1), C.c_int64(-1)
        Bf = np.asfortranarray(np.zeros((n, 17)))
        st = L.lib().gpv_plan_block_cv(plan._h, L.dptr(Bf), n if ldz is None else ldz, ncols, L.dptr(O), n if ldm is None else ldm,
                                       L.dptr(v), L.dptr(sc), C.byref(nf), C.byref(nbad))
        untouched = bool(np.all(O == guard) and np.all(v == guard) and np.all(sc == guard) and nf.value == -1 and nbad.value == -1)
        return st, untouched

    def set_raw(plan, lab):
        lab = np.ascontiguousarray(lab, dtype=np.int32)
        out = [C.c_int64(-1), C.c_int64(-1), C.c_int(-1), C.c_int64(-1)]
        st = L.lib().gpv_plan_set_blocks(plan._h, i32(lab), C.byref(out[0]), C.byref(out[1]), C.byref(out[2]), C.byref(out[3]))
        return st, [x.value for x in out]

    plan = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
    good = strips(c)
    assert cv(plan) == (7, True)                                                   # GPV_ERR_STATE: no evaluation, no blocks
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    assert cv(plan) == (7, True)                                                   # block_cv before set_blocks
    # ---- labels (GPV_ERR_BAD_ARG = 2): nothing is reported, and the plan has no blocks afterwards either
    big = np.zeros(n, dtype=np.int32)
    big[65:] = -1
    for what, lab in (("a block of 65", big), ("a label >= Nlocs", np.where(np.arange(n) == 9, n, good)),
                      ("a label < -1", np.where(np.arange(n) == 9, -2, good)), ("all -1", np.full(n, -1))):
        assert set_raw(plan, lab) == (2, [-1, -1, -1, -1]), what
        assert cv(plan) == (7, True), what
    assert L.lib().gpv_plan_set_blocks(None, i32(good), None, None, None, None) == 2
    big[64] = -1                                                                   # 64 is fine
    st, counts = set_raw(plan, big)
    assert st == 0 and counts[:3] == [1, 64, 64] and counts[3] >= 64
    assert plan.set_blocks(good)[:3] == (10, n, 64)                                # needs no evaluation of its own
    assert cv(plan)[0] == 0
    ref = plan.block_cv(B[:, :3])
    # a refused set_blocks keeps the previous blocks working
    assert set_raw(plan, np.full(n, -1))[0] == 2 and set_raw(plan, np.zeros(n))[0] == 2
    _same(ref, plan.block_cv(B[:, :3]))
    with pytest.raises(ValueError):
        plan.set_blocks(good[:-1])
    with pytest.raises(ValueError):
        plan.set_blocks(good.astype(np.float64))
    # ---- arguments
    assert cv(plan, ncols=0) == (2, True) and cv(plan, ncols=17) == (2, True) and cv(plan, ncols=-1) == (2, True)
    assert cv(plan, ldz=n - 1) == (2, True) and cv(plan, ldm=n - 1) == (2, True)
    for fn in (lambda: plan.block_cv(np.zeros((n, 17))), lambda: plan.block_cv(B[:-1])):
        with pytest.raises(ValueError):
            fn()
    # ---- state
    plan.set_data(np.ascontiguousarray(B[:, 0]))
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_LOGLIK_Z)                          # an evaluation without GPV_WANT_U: stale U
    assert cv(plan) == (7, True)
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    _same(ref, plan.block_cv(B[:, :3]))                                            # the blocks outlive evaluations
    obs = np.ones(n, dtype=bool)
    obs[5] = False
    plan.set_observed(obs)
    assert cv(plan) == (7, True)                                                   # unobserved locations
    plan.set_observed(None)
    assert cv(plan)[0] == 0
    sgv = G.vecchia_specify(np.array(c["locs"]), 15, ordering="coord", cond_yz="SGV", nn_backend="host")
    ps = G.Plan(sgv["locsord"], sgv["U_prep"]["revNNarray"], sgv["U_prep"]["revCond"])
    ps.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    assert set_raw(ps, good) == (7, [-1, -1, -1, -1]) and cv(ps) == (7, True)      # latent neighbours
    shard = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"], row_begin=0, row_end=n // 2)
    shard.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    assert set_raw(shard, good)[0] == 7 and cv(shard) == (7, True)                 # a row shard
    # ---- the API refuses what vecchia_loo refuses, and bad labels
    with pytest.raises(ValueError, match="needs cond_yz='z'"):
        G.vecchia_block_cv(c["B"][:, 0], sgv, c["cp"], TAU)
    with pytest.raises(ValueError, match="named covariance family"):
        G.vecchia_block_cv(c["B"][:, 0], TW._fresh(va), c["cp"], TAU, covmodel=lambda *a: None)
    with pytest.raises(ValueError, match="finite"):
        G.vecchia_block_cv(np.where(np.arange(n) == 3, np.nan, c["B"][:, 0]), TW._fresh(va), c["cp"], TAU)
    with pytest.raises(ValueError, match="more than 64"):
        G.vecchia_block_cv(c["B"][:, 0], TW._fresh(va), c["cp"], TAU, blocks=np.zeros(n, dtype=int))
    with pytest.raises(ValueError, match="no location is held out"):
        G.vecchia_block_cv(c["B"][:, 0], TW._fresh(va), c["cp"], TAU, blocks=np.full(n, -1))
    with pytest.raises(ValueError, match="one integer label per location"):
        G.vecchia_block_cv(c["B"][:, 0], TW._fresh(va), c["cp"], TAU, blocks=np.zeros(n - 1, dtype=int))
    with pytest.raises(ValueError, match="mean must be"):
        G.vecchia_block_cv(c["B"][:, 0], TW._fresh(va), c["cp"], TAU, mean=np.zeros(5))


def test_api_in_the_callers_order():
    G = _need_gpu()
    kw = TW.SHAPES["d2-vector-maxmin"]
    c, t = TL.truth(**kw)
    va, n = c["va"], c["n"]
    o = va["ord_z"] - 1
    rng = np.random.default_rng(17)
    Z = np.column_stack([c["B"], rng.standard_normal((n, 4))])          # R = 20: two calls
    blocks = 1000 * G.spatial_blocks(c["locs"]) + 7                      # any integer labels: mapped through np.unique
    blocks[rng.permutation(n)[:50]] = -1
    ids = np.full(n, -1, dtype=np.int64)
    ids[blocks >= 0] = np.unique(blocks[blocks >= 0], return_inverse=True)[1]
    tl = truth(kw, ids[o], Z=np.asfortranarray(Z[o]))
    mu = 2.0 + c["locs"][:, 0]
    out = G.vecchia_block_cv(Z + mu[:, None], TW._fresh(va), c["cp"], c["tau"], blocks=blocks, mean=mu)
    held = blocks >= 0
    nh = int(held.sum())
    assert out["n_heldout"] == nh == tl["n_heldout"] and out["n_blocks"] == ids.max() + 1
    want_mean, want_var, want_s = np.empty((n, 20), dtype=LD), np.empty(n, dtype=LD), np.empty((n, 20), dtype=LD)
    want_mean[o], want_var[o], want_s[o] = tl["mean"], tl["var"], tl["s"]
    assert out["mean"].shape == (n, 20) and out["var"].shape == (n,) and out["resid_std"].shape == (n, 20)
    assert np.all(np.isnan(out["mean"][~held])) and np.all(np.isnan(out["var"][~held])) and np.all(np.isnan(out["resid_std"][~held]))
    scale = np.maximum(np.abs(want_mean[held]).max(axis=0).astype(np.float64), np.abs(Z).max(axis=0))
    em = float((np.abs(out["mean"][held] - mu[held, None] - want_mean[held].astype(np.float64)).max(axis=0) / scale).max())
    ev = float((np.abs(out["var"][held] - want_var[held].astype(np.float64)) / want_var[held].astype(np.float64)).max())
    s_err = float((np.abs(out["resid_std"][held] - want_s[held].astype(np.float64)).max(axis=0)
                   / np.abs(want_s[held]).max(axis=0).astype(np.float64)).max())
    sc = tl["scores"].astype(np.float64)
    want = dict(rmse=np.sqrt(sc[:, 0] / nh), mae=sc[:, 1] / nh, log_score=-0.5 * (np.log(2 * np.pi) + (sc[:, 3] + sc[:, 2]) / nh),
                crps=sc[:, 4] / nh, coverage95=sc[:, 5] / nh, mean_sq_std_resid=sc[:, 2] / nh,
                joint_log_score=-0.5 * (np.log(2 * np.pi) + (sc[:, 7] + sc[:, 6]) / nh))
    worst = 0.0
    for k, w in want.items():
        assert out[k].shape == (20,)
        worst = max(worst, float((np.abs(out[k] - w) / np.abs(w)).max()))
    print(f"vecchia_block_cv, 20 columns, {out['n_blocks']} blocks, {nh} held out: mean {em:.2e}, var {ev:.2e}, resid_std {s_err:.2e}, "
          f"summaries {worst:.2e}, margin {float(tl['margin']):.2e}")
    # the mean is shifted by mu and back: its rounding (8 eps max |z + mu|) is far below the bar
    assert float(tl["margin"]) > TOL and max(em, ev, s_err, worst) <= TOL
    assert np.array_equal(out["coverage95"], want["coverage95"])
    # blocks=None: the cells of spatial_blocks in the caller's order
    auto = G.vecchia_block_cv(Z[:, 3], TW._fresh(va), c["cp"], c["tau"])
    lab = G.spatial_blocks(c["locs"])
    assert auto["n_heldout"] == n and auto["n_blocks"] == lab.max() + 1 and auto["mean"].shape == (n, 1)
    ta = truth(kw, lab[o], Z=np.asfortranarray(Z[o][:, 3:4]))
    wm = np.empty(n, dtype=LD)
    wm[o] = ta["mean"][:, 0]
    assert np.abs(auto["mean"][:, 0] - wm.astype(np.float64)).max() <= TOL * max(np.abs(wm).max(), np.abs(Z[:, 3]).max())


def test_estimate_with_block_cv():
    G = _need_gpu()
    locs, X, data = TW._trend_field()
    kw = dict(X=X, m=10, cond_yz="z", output_level=0, smoothness=1.5, method="L-BFGS-B")
    off = G.vecchia_estimate(data, locs, block_cv=False, **kw)
    on = G.vecchia_estimate(data, locs, block_cv=True, **kw)
    # the keys of the parent commit's result for these arguments
    assert list(off) == ["z", "beta_hat", "theta_hat", "trend", "locs", "covmodel", "n_evals", "neg_loglik", "convergence"]
    assert list(on) == list(off) + ["block_cv"]
    for k in off:
        u, w = off[k], on[k]
        assert (u.tobytes() == w.tobytes()) if isinstance(u, np.ndarray) else u == w, k
    keys = {"rmse", "mae", "log_score", "crps", "coverage95", "mean_sq_std_resid", "joint_log_score", "n_blocks", "n_heldout"}
    assert set(on["block_cv"]) == keys and on["block_cv"]["n_heldout"] == len(data)
    va = G.vecchia_specify(locs, 10, cond_yz="z")
    th = on["theta_hat"]
    want = G.vecchia_block_cv(on["z"], va, [th[0], th[1], 1.5], th[2])
    for k in keys - {"n_blocks", "n_heldout"}:
        assert on["block_cv"][k].tobytes() == want[k].tobytes(), k
    lab = np.where(locs[:, 0] < np.sort(locs[:, 0])[40], 0, -1)               # one test region of 40 points
    reg = G.vecchia_estimate(data, locs, block_cv=lab, **kw)["block_cv"]
    assert reg["n_blocks"] == 1 and reg["n_heldout"] == 40
    print({k: (float(v[0]) if isinstance(v, np.ndarray) else v) for k, v in on["block_cv"].items()}, "one region:", float(reg["rmse"][0]))
    assert 0.85 <= on["block_cv"]["coverage95"][0] <= 1.0 and 0.5 <= on["block_cv"]["mean_sq_std_resid"][0] <= 1.5
    with pytest.raises(ValueError, match="block_cv needs"):
        G.vecchia_estimate(data, locs, X=X, m=10, output_level=0, block_cv=True)
