"""gpv_plan_whiten_t / gpv_plan_precision / gpv_plan_loo (gpv_loo.hip) on the GPU: the transpose of the whitening operator of an
evaluation, precision products, leave-one-out cross-validation, and what is built on them (vecchia_precision_multiply,
vecchia_loo, vecchia_estimate(loo=True)).

Truth: tests/_loo_truth.py, the rows of T from the hand-written long-double Cholesky of tests/_whiten_truth.py, independent of
Lentries.  Bars (the project's flat 1e-8, tests/_parity.py):
  T'E, QB, leave-one-out mean    per column in the max norm: max_i |got - truth| <= 1e-8 max_i |truth|
                                 (the mean, a difference of two doubles, plus its rounding floor 8 eps max |z|: mean_floor;
                                 measured: at most 6e-14 of max |truth| wherever m > 0)
  q = diag Q, variance           per entry, relative (sums of squares: no cancellation)
  scores                         |got - truth| <= 1e-8 sum |term|; the coverage count exactly
Inputs: the plans and columns of tests/test_gpu_whiten.py (case, SHAPES); a star plan (n = 3000, every row k > 0 conditions on
row 0 alone: one column of the transposed index has 2999 entries, the rest none); n = 20 000 in given order with m = 2.
Every test prints its measured worst figures."""
import ctypes as C
import functools

import numpy as np
import pytest

import _loo_truth as T
import test_gpu_whiten as TW

pytestmark = pytest.mark.gpu

TOL = 1e-8
TAU = 0.1
LD = np.longdouble


def _need_gpu():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


def _key(kw):
    return tuple(sorted(kw.items()))


def _case(kw):
    """the cached case of tests/test_gpu_whiten.py, spelled as that file spells it (its cache tells case(31) from case(m=31))"""
    return TW.case(kw["m"]) if list(kw) == ["m"] else TW.case(**kw)


def _truth_of(va, Bord, cm, cp, tau_ord):
    F = T.factor_ld(va["locsord"], va["U_prep"]["revNNarray"], cm, cp, tau_ord)
    n = Bord.shape[0]
    E = T.apply_T(F, Bord)
    Ein = np.asfortranarray(E.astype(np.float64))      # what whiten_t is given: the whitened columns, rounded to double
    out = dict(F=F, Ein=Ein, TtE=T.apply_Tt(F, Ein), QB=T.apply_Tt(F, E), q=T.qdiag(F, n))
    out["loo"] = T.loo_from(Bord, out["QB"], out["q"])
    for a in (Ein, out["TtE"], out["QB"], out["q"]):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _truth(key):
    """long-double T'E, QB, q and leave-one-out results of the 16 columns of a case, computed once and shared read-only"""
    c = _case(dict(key))
    return _truth_of(c["va"], c["Bord"], c["cm"], c["cp"], c["tau_ord"])


def truth(**kw):
    return _case(kw), _truth(_key(kw))


def colmax(got, want, what, floor=0.0):
    """floor: an absolute allowance per column, for a result that is a difference of doubles (the leave-one-out mean).
    Returns the worst column's error over its scale, the scale being max |truth| (+ floor / 1e-8: the bar stays 1e-8 of it)."""
    want = want[:, :got.shape[1]]
    dif, scale = np.abs(got - want.astype(np.float64)).max(axis=0), np.abs(want).max(axis=0).astype(np.float64)
    assert np.all(np.isfinite(got)) and np.all(dif <= TOL * scale + floor), (what, dif, scale, floor)
    return float((dif / np.maximum(scale, 1e-300)).max()) if np.all(np.asarray(floor) == 0.0) else float((dif / (scale + floor / TOL)).max())


def mean_floor(Z):
    """The leave-one-out mean is the difference z_i - r_i / q_i of two doubles, so no double result can be nearer to the truth
    than the rounding of its two operands: r / q carries about eight roundings of half an ulp each (the products and sums
    behind r and q, the division) and the subtraction one more, 8 eps |z_i| with room.  The bar of the mean is the issue's
    1e-8 max |truth| PLUS this floor, 1.8e-15 max |z|: seven orders below the bar wherever the truth is not tiny, and the whole
    bar at m = 0, where T is diagonal, the truth is zero up to ITS rounding (1e-20) and max |truth| measures nothing."""
    return 8 * np.finfo(np.float64).eps * np.abs(np.asarray(Z, dtype=np.float64)).max(axis=0)


def entryrel(got, want, what):
    err = float((np.abs(got - want.astype(np.float64)) / np.abs(want).astype(np.float64)).max())
    assert np.all(np.isfinite(got)) and err <= TOL, (what, err)
    return err


def check_scores(got, t, ncols, what):
    want, sabs = t["loo"]["scores"][:ncols], t["loo"]["sabs"][:ncols]
    err = float((np.abs(got[:, :5] - want[:, :5].astype(np.float64)) / sabs[:, :5].astype(np.float64)).max())
    assert err <= TOL, (what, err)
    assert np.array_equal(got[:, 5], want[:, 5].astype(np.float64)), (what, got[:, 5], want[:, 5], float(t["loo"]["margin"]))
    return err


def check_all(plan, c, t, ncols, what):
    """the three entries on the first ncols columns against the truth; returns what they returned"""
    Bt, nf = plan.whiten_t(t["Ein"][:, :ncols])
    assert nf == 0 and Bt.shape == (c["n"], ncols)
    a = colmax(Bt, t["TtE"], what + " T'E")
    R, q, nf = plan.precision(c["Bord"][:, :ncols])
    assert nf == 0
    b = colmax(R, t["QB"], what + " QB")
    d = entryrel(q, t["q"], what + " q")
    mean, var, scores, nf = plan.loo(c["Bord"][:, :ncols])
    assert nf == 0 and scores.shape == (ncols, 6)
    e = colmax(mean, t["loo"]["mean"], what + " mean", floor=mean_floor(c["Bord"][:, :ncols]))
    f = entryrel(var, t["loo"]["var"], what + " var")
    g = check_scores(scores, t, ncols, what)
    print(f"{what}: T'E {a:.2e}, QB {b:.2e}, mean {e:.2e} (column max norm); q {d:.2e}, var {f:.2e} (per entry); "
          f"scores {g:.2e} of sum|term|; coverage {scores[:, 5].astype(int).tolist()}")
    return Bt, R, q, mean, var, scores


@pytest.mark.parametrize("ncols", [16, 3, 1])
@pytest.mark.parametrize("m", [0, 1, 15, 16, 31, 40, 70])
def test_row_lengths(m, ncols):
    G = _need_gpu()
    c, t = truth(m=m)
    plan = TW._plan(G, c)
    check_all(plan, c, t, ncols, f"m={m} ncols={ncols}")
    nnz, longest, empty = plan.loo_index()
    deg = np.bincount(np.concatenate([idx[:, :-1].ravel() for _, idx, _ in t["F"]]).astype(np.int64), minlength=c["n"])
    assert (nnz, longest, empty) == (int(deg.sum()), int(deg.max()), int((deg == 0).sum()))
    if m == 31:
        assert (empty, longest, int((deg > 64).sum())) == (18, 152, 77)
    if m == 70:
        assert (empty, longest, int((deg > 64).sum())) == (11, 279, 227)


@pytest.mark.parametrize("name", list(TW.SHAPES))
def test_shapes(name):
    G = _need_gpu()
    c, t = truth(**TW.SHAPES[name])
    for ncols in (16, 3):
        check_all(TW._plan(G, c), c, t, ncols, f"{name} ncols={ncols}")


@functools.lru_cache(maxsize=None)
def star_case():
    n = 3000
    rng = np.random.default_rng(11)
    locs = rng.random((n, 2))
    nn = np.zeros((n, 2), dtype=np.int32)
    nn[:, 1] = np.arange(1, n + 1)
    nn[1:, 0] = 1
    cond = np.where(nn > 0, 0, -1).astype(np.int8)
    cond[:, 1] = 1
    B = np.asfortranarray(rng.standard_normal((n, 16)))
    va = dict(locsord=locs, U_prep=dict(revNNarray=nn, revCond=cond))
    c = dict(va=va, cm="matern", cp=[1.3, 0.25, 1.5], tau_ord=np.float64(TAU), Bord=B, n=n)
    for a in (locs, nn, cond, B):
        a.setflags(write=False)
    return c, _truth_of(va, B, c["cm"], c["cp"], c["tau_ord"])


def test_star_plan():
    """one column of 2999 entries, 2999 empty ones"""
    G = _need_gpu()
    c, t = star_case()
    plan = TW._plan(G, c)
    assert plan.loo_index() == (2999, 2999, 2999)
    for ncols in (16, 1):
        check_all(plan, c, t, ncols, f"star ncols={ncols}")


@functools.lru_cache(maxsize=None)
def wide_case():
    c = TW.case(2, n=20000, ordering="none")
    return c, _truth_of(c["va"], c["Bord"], c["cm"], c["cp"], c["tau_ord"])


def test_wide_plan():
    G = _need_gpu()
    c, t = wide_case()
    plan = TW._plan(G, c)
    nnz, longest, empty = plan.loo_index()
    print("n = 20000, m = 2: entries", nnz, "longest column", longest, "empty columns", empty)
    assert empty == 6325 and nnz == 2 * 20000 - 3
    for ncols in (16, 3):
        check_all(plan, c, t, ncols, f"wide ncols={ncols}")


def test_adjoint_symmetric_and_consistent_with_whiten():
    G = _need_gpu()
    c, t = truth(m=31)
    plan = TW._plan(G, c)
    B = c["Bord"]
    rng = np.random.default_rng(21)
    Ecols = np.asfortranarray(rng.standard_normal((c["n"], 16)))
    Gm, _, _, TB = plan.whiten(B, want_E=True)
    TtE, _ = plan.whiten_t(Ecols)
    lhs, rhs = (TB * Ecols).sum(axis=0), (B * TtE).sum(axis=0)
    adj = np.abs(lhs - rhs) / np.maximum((np.abs(TB * Ecols)).sum(axis=0), np.abs(B * TtE).sum(axis=0))
    R, _, _ = plan.precision(B)
    S = B.T @ R                                         # x'(Qy) for all pairs of columns
    Sabs = np.abs(B).T @ np.abs(R)
    sym = (np.abs(S - S.T) / np.maximum(Sabs, Sabs.T)).max()
    zr = (B * R).sum(axis=0)
    gram = np.abs(zr - np.diag(Gm)) / np.abs(B * R).sum(axis=0)
    print(f"adjointness {adj.max():.2e}, symmetry {sym:.2e}, sum z r against gram[z, z] {gram.max():.2e} (of sum |term|)")
    assert adj.max() <= TOL and sym <= TOL and gram.max() <= TOL


def _raw(name, plan, *args):
    from gpvecchia_amd import _lib as L
    return getattr(L.lib(), name)(plan._h, *args)


def test_leading_dimensions_and_null_outputs():
    """leading dimensions > Nlocs: the padding rows are neither read into the result nor written; optional outputs left out"""
    G = _need_gpu()
    from gpvecchia_amd import _lib as L
    c, t = truth(m=15)
    plan = TW._plan(G, c)
    n, nc, pad = c["n"], 3, 7
    nf = C.c_int64(-1)

    def big(A, extra):
        out = np.full((n + extra, nc), np.nan, order="F")
        out[:n] = A[:, :nc]
        return out
    Bbig, Ebig = big(c["Bord"], pad), big(t["Ein"], pad)
    Obig = np.full((n + pad + 2, nc), -7.0, order="F")
    assert _raw("gpv_plan_whiten_t", plan, L.dptr(Ebig), n + pad, nc, L.dptr(Obig), n + pad + 2, C.byref(nf)) == 0 and nf.value == 0
    assert np.all(Obig[n:] == -7.0)
    colmax(Obig[:n], t["TtE"], "whiten_t, padded")
    Obig[:] = -7.0
    q = np.full(n + 1, -7.0)
    assert _raw("gpv_plan_precision", plan, L.dptr(Bbig), n + pad, nc, L.dptr(Obig), n + pad + 2, L.dptr(q), C.byref(nf)) == 0
    assert np.all(Obig[n:] == -7.0) and q[n] == -7.0
    colmax(Obig[:n], t["QB"], "precision, padded")
    entryrel(q[:n], t["q"], "q")
    Obig[:] = -7.0
    assert _raw("gpv_plan_precision", plan, L.dptr(Bbig), n + pad, nc, L.dptr(Obig), n + pad + 2, None, C.byref(nf)) == 0
    colmax(Obig[:n], t["QB"], "precision without qdiag")
    Obig[:] = -7.0
    var, sc = np.full(n + 1, -7.0), np.full((nc + 1, 6), -7.0)
    assert _raw("gpv_plan_loo", plan, L.dptr(Bbig), n + pad, nc, L.dptr(Obig), n + pad + 2, L.dptr(var), L.dptr(sc), C.byref(nf)) == 0
    assert np.all(Obig[n:] == -7.0) and var[n] == -7.0 and np.all(sc[nc] == -7.0)
    colmax(Obig[:n], t["loo"]["mean"], "loo, padded", floor=mean_floor(c["Bord"][:, :nc]))
    entryrel(var[:n], t["loo"]["var"], "var")
    check_scores(sc[:nc], t, nc, "scores")
    sc2 = np.zeros((nc, 6))
    assert _raw("gpv_plan_loo", plan, L.dptr(Bbig), n + pad, nc, None, 0, None, L.dptr(sc2), C.byref(nf)) == 0
    assert sc2.tobytes() == sc[:nc].tobytes()
    mean, var2, sc3, _ = plan.loo(c["Bord"][:, :nc], want_mean=False, want_var=False)
    assert mean is None and var2 is None and sc3.tobytes() == sc2.tobytes()
    assert L.lib().gpv_loo_nscores() == 6


def test_refusals():
    G = _need_gpu()
    from gpvecchia_amd import _lib as L
    c, t = truth(m=15)
    va, prep, n = c["va"], c["va"]["U_prep"], c["n"]
    B = c["Bord"]
    guard = -7.0

    def refused(plan, want):
        """the three entries straight at the C ABI: the status, and nothing written"""
        O, q, sc, nf = np.full((n, 3), guard, order="F"), np.full(n, guard), np.full((3, 6), guard), C.c_int64(-1)
        Bf = np.asfortranarray(B[:, :3])
        st = (_raw("gpv_plan_whiten_t", plan, L.dptr(Bf), n, 3, L.dptr(O), n, C.byref(nf)),
              _raw("gpv_plan_precision", plan, L.dptr(Bf), n, 3, L.dptr(O), n, L.dptr(q), C.byref(nf)),
              _raw("gpv_plan_loo", plan, L.dptr(Bf), n, 3, L.dptr(O), n, L.dptr(q), L.dptr(sc), C.byref(nf)))
        assert st == (want,) * 3, st
        assert np.all(O == guard) and np.all(q == guard) and np.all(sc == guard) and nf.value == -1

    def ok(plan):
        assert plan.whiten_t(B)[1] == 0 and plan.precision(B)[2] == 0 and plan.loo(B)[3] == 0

    plan = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
    refused(plan, 7)                                                               # GPV_ERR_STATE: no evaluation yet
    plan.set_data(np.ascontiguousarray(B[:, 0]))
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_LOGLIK_Z)
    refused(plan, 7)                                                               # the evaluation did not ask for U
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    ok(plan)
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_LOGLIK_Z)                          # ... and the next one did not: stale U
    refused(plan, 7)
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    # ---- arguments (GPV_ERR_BAD_ARG = 2)
    Bf, O = np.asfortranarray(np.zeros((n, 17))), np.full((n, 17), guard, order="F")
    q, sc, nf = np.full(n, guard), np.full((17, 6), guard), C.c_int64(-1)
    good = {"gpv_plan_whiten_t": [L.dptr(Bf), n, 3, L.dptr(O), n, C.byref(nf)],
            "gpv_plan_precision": [L.dptr(Bf), n, 3, L.dptr(O), n, L.dptr(q), C.byref(nf)],
            "gpv_plan_loo": [L.dptr(Bf), n, 3, L.dptr(O), n, L.dptr(q), L.dptr(sc), C.byref(nf)]}
    bad = {"gpv_plan_whiten_t": ((0, None), (3, None), (5, None), (2, 0), (2, -1), (2, 17), (1, n - 1), (4, n - 1)),
           "gpv_plan_precision": ((0, None), (3, None), (6, None), (2, 0), (2, -1), (2, 17), (1, n - 1), (4, n - 1)),
           "gpv_plan_loo": ((0, None), (6, None), (7, None), (2, 0), (2, -1), (2, 17), (1, n - 1), (4, n - 1))}
    for name, args in good.items():
        for pos, val in bad[name]:
            a = list(args)
            a[pos] = val
            O[:] = guard
            nf.value = -1
            assert _raw(name, plan, *a) == 2, (name, pos, val)
            assert np.all(O == guard) and nf.value == -1
        assert getattr(L.lib(), name)(None, *args) == 2
        assert _raw(name, plan, *args) == 0
    for fn in (plan.whiten_t, plan.precision, plan.loo):
        with pytest.raises(ValueError):
            fn(Bf)                                                                 # 17 columns
        with pytest.raises(ValueError):
            fn(B[:-1])
    # ---- state
    comm = G.Comm(0, 0, 1, lambda mine: mine)
    plan.set_comm(comm)
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    refused(plan, 7)                                                               # a communicator is attached
    plan.set_comm(None)
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    ok(plan)
    obs = np.ones(n, dtype=bool)
    obs[5] = False
    plan.set_observed(obs)
    refused(plan, 7)                                                               # unobserved locations
    plan.set_observed(None)
    ok(plan)
    shard = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"], row_begin=0, row_end=n // 2)
    shard.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    refused(shard, 7)                                                              # a row shard
    sgv = G.vecchia_specify(np.array(c["locs"]), 15, ordering="coord", cond_yz="SGV", nn_backend="host")
    ps = G.Plan(sgv["locsord"], sgv["U_prep"]["revNNarray"], sgv["U_prep"]["revCond"])
    ps.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    refused(ps, 7)                                                                 # latent neighbours
    # ---- the API refuses what vecchia_whiten refuses
    for call in (lambda v, **kw: G.vecchia_loo(c["B"][:, 0], v, c["cp"], TAU, **kw),
                 lambda v, **kw: G.vecchia_precision_multiply(c["B"][:, :2], v, c["cp"], TAU, **kw)):
        with pytest.raises(ValueError, match="needs cond_yz='z'"):
            call(sgv)
        with pytest.raises(ValueError, match="named covariance family"):
            call(TW._fresh(va), covmodel=lambda *a: None)
    with pytest.raises(ValueError, match="finite"):
        G.vecchia_loo(np.where(np.arange(n) == 3, np.nan, c["B"][:, 0]), TW._fresh(va), c["cp"], TAU)
    with pytest.raises(ValueError, match="one row per location"):
        G.vecchia_loo(c["B"][:-1, 0], TW._fresh(va), c["cp"], TAU)
    with pytest.raises(ValueError, match="nuggets must be"):
        G.vecchia_loo(c["B"][:, 0], TW._fresh(va), c["cp"], np.full(5, TAU))
    with pytest.raises(ValueError, match="mean must be"):
        G.vecchia_loo(c["B"][:, 0], TW._fresh(va), c["cp"], TAU, mean=np.zeros(5))


def test_second_evaluation_gives_its_own_q():
    G = _need_gpu()
    c, t = truth(m=15)
    plan = TW._plan(G, c)
    q1 = plan.precision(c["Bord"][:, :2])[1]
    entryrel(q1, t["q"], "first evaluation")
    cp2, tau2 = [0.7, 0.4, 1.5], 0.25
    plan.eval(c["cm"], cp2, tau2, G.GPV_WANT_U)
    t2 = _truth_of(c["va"], c["Bord"][:, :2], c["cm"], cp2, np.float64(tau2))
    R2, q2, nf = plan.precision(c["Bord"][:, :2])
    mean2, var2, sc2, _ = plan.loo(c["Bord"][:, :2])
    print("second evaluation: q", entryrel(q2, t2["q"], "q"), "QB", colmax(R2, t2["QB"], "QB"), "var",
          entryrel(var2, t2["loo"]["var"], "var"), "largest change of q", float(np.abs(q2 / q1 - 1).max()))
    colmax(mean2, t2["loo"]["mean"], "mean", floor=mean_floor(c["Bord"][:, :2]))
    assert np.abs(q2 / q1 - 1).min() > 1e-3


def test_nan_coordinate():
    """a failed row, provoked as tests/test_gpu_whiten.py provokes one: n_failed >= 1 and every output NaN"""
    G = _need_gpu()
    c, t = truth(m=15)
    va, prep, n, bad = c["va"], c["va"]["U_prep"], c["n"], 300
    poisoned = np.array(va["locsord"])
    poisoned[bad, 1] = np.nan
    plan = G.Plan(poisoned, prep["revNNarray"], prep["revCond"])
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    nn = np.nan_to_num(np.asarray(prep["revNNarray"], dtype=np.float64), nan=0.0).astype(np.int64)
    hit = int((nn == bad + 1).any(axis=1).sum())
    Bt, nf = plan.whiten_t(c["Bord"][:, :3])
    assert hit >= 1 and nf == hit and np.all(np.isnan(Bt))
    R, q, nf = plan.precision(c["Bord"][:, :3])
    assert nf == hit and np.all(np.isnan(R)) and np.all(np.isnan(q))
    mean, var, sc, nf = plan.loo(c["Bord"])
    assert nf == hit and np.all(np.isnan(mean)) and np.all(np.isnan(var)) and np.all(np.isnan(sc))
    out = G.vecchia_loo(c["B"][:, :2], TW._fresh(va, locsord=poisoned), c["cp"], TAU)
    assert np.all(np.isnan(out["mean"])) and np.all(np.isnan(out["log_score"]))


def test_state_bitwise_and_last_evaluation_intact():
    G = _need_gpu()
    c, t = truth(m=31)
    va, prep = c["va"], c["va"]["U_prep"]
    plan = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
    plan.set_data(np.ascontiguousarray(c["Bord"][:, 0]))
    plan.build_posterior()
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_DENOM)              # a posterior factor, so that the stamp is not 0
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U | G.GPV_WANT_LOGLIK_Z)
    sums, Lent, stamp = plan.sums(), plan.Lentries(), plan.factor_stamp()
    assert stamp != 0
    w0 = plan.whiten(c["Bord"], want_E=True)
    a = (plan.whiten_t(t["Ein"]), plan.precision(c["Bord"]), plan.loo(c["Bord"]))
    plan.loo(c["Bord"][:, :5])                         # another padded width in between
    b = (plan.whiten_t(t["Ein"]), plan.precision(c["Bord"]), plan.loo(c["Bord"]))
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert (u.tobytes() == v.tobytes()) if isinstance(u, np.ndarray) else u == v
    # column c of a 16-column call is the column of a one-column call, bit for bit
    for col in (0, 7, 15):
        one = (plan.whiten_t(t["Ein"][:, col]), plan.precision(c["Bord"][:, col]), plan.loo(c["Bord"][:, col]))
        assert one[0][0][:, 0].tobytes() == a[0][0][:, col].tobytes()
        assert one[1][0][:, 0].tobytes() == a[1][0][:, col].tobytes() and one[1][1].tobytes() == a[1][1].tobytes()
        assert one[2][0][:, 0].tobytes() == a[2][0][:, col].tobytes() and one[2][1].tobytes() == a[2][1].tobytes()
        assert one[2][2][0].tobytes() == a[2][2][col].tobytes()
    three = plan.precision(c["Bord"][:, 5:8])[0]
    assert three.tobytes() == np.asfortranarray(a[1][0][:, 5:8]).tobytes()
    assert np.array_equal(plan.sums(), sums) and np.array_equal(plan.Lentries(), Lent) and plan.factor_stamp() == stamp
    w1 = plan.whiten(c["Bord"], want_E=True)
    assert w0[0].tobytes() == w1[0].tobytes() and w0[1] == w1[1] and w0[3].tobytes() == w1[3].tobytes()


def test_api_in_the_callers_order():
    G = _need_gpu()
    c, t = truth(**TW.SHAPES["d2-vector-maxmin"])
    va, n = c["va"], c["n"]
    o = va["ord_z"] - 1
    rng = np.random.default_rng(17)
    Z = np.column_stack([c["B"], rng.standard_normal((n, 4))])          # R = 20: two batches
    F = t["F"]
    tl = T.loo_ld(F, Z[o])
    out = G.vecchia_loo(Z, TW._fresh(va), c["cp"], c["tau"])
    want_mean = np.empty((n, 20), dtype=LD)
    want_mean[o] = tl["mean"]
    want_var, want_s = np.empty(n, dtype=LD), np.empty((n, 20), dtype=LD)
    want_var[o], want_s[o] = tl["var"], tl["s"]
    assert out["mean"].shape == (n, 20) and out["var"].shape == (n,) and out["resid_std"].shape == (n, 20)
    a, b = colmax(out["mean"], want_mean, "mean", floor=mean_floor(Z)), entryrel(out["var"], want_var, "var")
    s_err = float((np.abs(out["resid_std"] - want_s.astype(np.float64)).max(axis=0) / np.abs(want_s).max(axis=0).astype(np.float64)).max())
    sc = tl["scores"].astype(np.float64)
    want = dict(rmse=np.sqrt(sc[:, 0] / n), mae=sc[:, 1] / n, log_score=-0.5 * (np.log(2 * np.pi) + (sc[:, 3] + sc[:, 2]) / n),
                crps=sc[:, 4] / n, coverage95=sc[:, 5] / n, mean_sq_std_resid=sc[:, 2] / n)
    worst = 0.0
    for k, w in want.items():
        assert out[k].shape == (20,)
        worst = max(worst, float((np.abs(out[k] - w) / np.abs(w)).max()))
    print(f"vecchia_loo, 20 columns: mean {a:.2e}, var {b:.2e}, resid_std {s_err:.2e}, summaries {worst:.2e}")
    assert s_err <= TOL and worst <= TOL
    assert np.array_equal(out["coverage95"], want["coverage95"])
    one = G.vecchia_loo(Z[:, 3], TW._fresh(va), c["cp"], c["tau"])
    assert one["mean"].shape == (n, 1) and one["mean"][:, 0].tobytes() == out["mean"][:, 3].tobytes()
    # mean=: subtracted before, added back
    mu = 2.0 + c["locs"][:, 0]
    for m_ in (1.5, mu):
        sh = G.vecchia_loo(Z[:, :2] + (m_ if np.ndim(m_) == 0 else m_[:, None]), TW._fresh(va), c["cp"], c["tau"], mean=m_)
        shift = m_ if np.ndim(m_) == 0 else m_[:, None]
        assert np.abs(sh["mean"] - shift - out["mean"][:, :2]).max() <= 1e-12 * np.abs(out["mean"]).max() + 1e-12
        assert np.abs(sh["rmse"] - out["rmse"][:2]).max() <= 1e-10
    # precision products
    QB, qd = G.vecchia_precision_multiply(Z, TW._fresh(va), c["cp"], c["tau"])
    want_QB, want_q = np.empty((n, 20), dtype=LD), np.empty(n, dtype=LD)
    want_QB[o] = T.apply_Tt(F, T.apply_T(F, Z[o]))
    want_q[o] = t["q"]
    print("vecchia_precision_multiply:", colmax(QB, want_QB, "QB"), entryrel(qd, want_q, "q"))


def test_estimate_with_loo():
    G = _need_gpu()
    locs, X, data = TW._trend_field()
    kw = dict(X=X, m=10, cond_yz="z", output_level=0, smoothness=1.5, method="L-BFGS-B")
    for trend in ("ols", "gls"):
        off = G.vecchia_estimate(data, locs, trend=trend, loo=False, **kw) if trend == "ols" else G.vecchia_estimate(data, locs, trend=trend, **kw)
        on = G.vecchia_estimate(data, locs, trend=trend, loo=True, **kw)
        assert "loo" not in off and list(on) == list(off) + ["loo"]
        for k in off:
            u, w = off[k], on[k]
            if isinstance(u, np.ndarray):
                assert u.tobytes() == w.tobytes(), k
            else:
                assert u == w, k
        va = G.vecchia_specify(locs, 10, cond_yz="z")
        th = on["theta_hat"]
        want = G.vecchia_loo(on["z"], va, [th[0], th[1], 1.5], th[2])
        assert set(on["loo"]) == {"rmse", "mae", "log_score", "crps", "coverage95", "mean_sq_std_resid"}
        for k, v in on["loo"].items():
            assert v.tobytes() == want[k].tobytes(), k
        print(trend, {k: float(v[0]) for k, v in on["loo"].items()})
        assert 0.85 <= on["loo"]["coverage95"][0] <= 1.0 and 0.5 <= on["loo"]["mean_sq_std_resid"][0] <= 1.5
    with pytest.raises(ValueError, match="loo=True needs"):
        G.vecchia_estimate(data, locs, X=X, m=10, output_level=0, loo=True)
