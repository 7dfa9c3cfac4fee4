"""gpv_plan_cond_sim (gpv_csim.hip) on the GPU: conditional simulation of a cond.yz='z' plan over a map by the sequential kriging
sweep, and what is built on it (Plan.cond_sim, vecchia_cond_sim, vecchia_pred(local=True, nsim=)).

Truth: tests/_csim_truth.py (the search definition, a long-double solve per location, sequential substitution, the failure and
NaN rule; proven on the CPU by tests/test_csim_truth_host.py), run in the plan's ORDERED numbering of the observations.

The bar is the project's 1e-8 against the long-double truth, per column in the max norm over the locations that are not NaN,
relative to the column's largest magnitude; sd relative to itself, per location.  The worst condition number among the inputs
is about 1e6 (smoothness 2.5, range 0.1), so FP64 does not strain the bar.  Every accuracy test prints the maxima it observed
(DESIGN.md §4u).  The set of NaN locations must be the truth's.  Observed on an MI355X: mean <= 2.3e-13, deviation fields
<= 5.5e-13, sd <= 2.4e-13 but at smoothness 2.5 (1.9e-11) and in the m = 2 case with wide levels (2.4e-10)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _csim_truth as T
import _krige_truth as KT

pytestmark = pytest.mark.gpu

N, NQ, TAU, BAR, NSIM, SEED = 1500, 400, 0.1, 1e-8, 20, 12345
GPV_ERR_BAD_ARG, GPV_ERR_UNSUPPORTED_M, GPV_ERR_STATE, GPV_ERR_INDEX = 2, 5, 7, 8
MATERN15 = ("matern", (1.2, 0.07, 1.5))
DUP = 300                                                             # this location is a copy of location 17


def _G():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


def _ordered(va, Z):
    """(the plan, the ORDERED coordinates, the ORDERED data)"""
    from gpvecchia_amd import api
    return api._plan_for(va), va["locsord"], Z[va["ord_z"] - 1]


@functools.lru_cache(maxsize=None)
def _case(dim=2, n=N, nq=NQ):
    """observations, 16 data columns, prediction locations in sweep order, normals and the 'z' plan; shared and read-only"""
    G = _G()
    rng = np.random.default_rng(70 + dim)
    locs = rng.random((n, dim))
    Z = rng.standard_normal((n, 16))
    q = rng.random((nq, dim))
    q[:5] = locs[rng.choice(n, 5, replace=False)]                     # on observations
    q[5:10, :2] = [[-0.3, 0.5], [1.2, 1.1], [0.5, 1.004], [-2.0, -3.0], [1.0 + 1e-9, 0.2]]                   # outside the box
    if nq > DUP:
        q[DUP] = q[17]                                                # a duplicate of an earlier prediction location
    E = rng.standard_normal((nq, NSIM))
    scale = None if dim != 3 else np.array([0.06, 0.08, 0.1])
    va = G.vecchia_specify(locs, 10, cond_yz="z", scale=scale)
    plan, lo, Zo = _ordered(va, Z)
    for a in (locs, Z, q, E, lo, Zo):
        a.setflags(write=False)
    return dict(locs=locs, Z=Z, q=q, E=E, va=va, scale=scale, plan=plan, lo=lo, Zo=Zo)


@functools.lru_cache(maxsize=None)
def _truth(covmodel, cp, m, dim=2, n=N, nq=NQ):
    """the long-double truth of all 16 columns, of the deviation fields of the case's normals and of the generator's"""
    G, c = _G(), _case(dim, n, nq)
    NN = T.ordered_search(c["lo"], c["q"], m, scale=c["scale"])
    t = T.truth(c["lo"], TAU, c["Zo"], c["q"], NN, covmodel, list(cp))
    t["NN"] = NN
    t["dev"] = t["colour"](c["E"])
    t["dev_seed"] = t["colour"](G.draws_normals_host(SEED, n, nq, 0, NSIM).T)
    return t


def _col_err(got, want):
    """max over the columns of max |got - want| / max |want|, over the rows that are not NaN in the truth; the NaN sets agree"""
    got, want = np.asarray(got), np.asarray(want)
    got = got[:, None] if got.ndim == 1 else got
    want = want[:, None] if want.ndim == 1 else want
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), "the NaN locations are not the truth's"
    ok = ~np.isnan(want[:, 0])
    return float((np.abs(got[ok] - want[ok]).max(axis=0) / np.abs(want[ok]).max(axis=0)).max())


def _sd_err(got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return float((np.abs(got[ok] - want[ok]) / want[ok]).max())


def _check(tag, r, t, R, dev="dev"):
    em, es = _col_err(r["mean"], t["mean"][:, :R]), _sd_err(r["sd"], t["sd"])
    ed = _col_err(r["dev"], t[dev]) if r["dev"].shape[1] else 0.0
    print(f"cond_sim {tag}: levels {r['n_levels']}, launches {r['n_launches']}, failed {r['n_failed']}; "
          f"max error mean {em:.3g}, sd {es:.3g}, dev {ed:.3g}")
    assert r["n_failed"] == int(t["failed"].sum())
    assert em <= BAR and es <= BAR and ed <= BAR


MAIN = [(m, 16) for m in (7, 15, 16, 30, 31, 63)] + [(30, 1), (30, 3)]


@pytest.mark.parametrize("m,R", MAIN)
def test_main_case_with_given_normals(m, R):
    c = _case()
    covmodel, cp = MATERN15
    t = _truth(covmodel, cp, m)
    assert t["failed"][DUP] and t["failed"].sum() >= 1
    Z = c["Zo"][:, 0] if R == 1 else c["Zo"][:, :R]
    r = c["plan"].cond_sim(covmodel, cp, TAU, c["q"], m, Z_ord=Z, E=c["E"])
    assert r["mean"].shape == (NQ, R) and r["dev"].shape == (NQ, NSIM) and r["sd"].shape == (NQ,)
    assert r["n_failed"] >= 1 and np.isnan(r["sd"][DUP])
    lv, _, lp = T.levels(t["NN"], N)
    assert r["n_levels"] == lp.size - 1 and np.diff(lp).max() <= 256 and r["n_launches"] == 1      # all narrow: one run
    _check(f"m={m} R={R}", r, t, R)


def test_main_case_with_the_generators_normals():
    c = _case()
    covmodel, cp = MATERN15
    t = _truth(covmodel, cp, 30)
    r = c["plan"].cond_sim(covmodel, cp, TAU, c["q"], 30, Z_ord=c["Zo"][:, :3], seed=SEED, nsim=NSIM)
    _check("seeded m=30", r, t, 3, dev="dev_seed")


@pytest.mark.parametrize("covmodel,cp", [("matern", (1.2, 0.1, 0.5)), ("matern", (1.2, 0.1, 2.5)), ("matern", (1.2, 0.06, 0.8))])
def test_smoothness_families(covmodel, cp):
    c = _case()
    t = _truth(covmodel, cp, 30)
    r = c["plan"].cond_sim(covmodel, cp, TAU, c["q"], 30, Z_ord=c["Zo"][:, :3], E=c["E"][:, :3])
    t = dict(t, dev=t["dev"][:, :3])
    _check(f"{covmodel} {cp}", r, t, 3)


def test_esqe_in_five_dimensions():
    c = _case(5, 600, 150)
    cp = (0.8, 0.4, 0.4, 0.3)
    t = _truth("esqe", cp, 30, 5, 600, 150)
    r = c["plan"].cond_sim("esqe", cp, TAU, c["q"], 30, Z_ord=c["Zo"][:, :3], E=c["E"])
    _check("esqe 5-D", r, t, 3)


def test_scaledim_in_three_dimensions_with_scale():
    c = _case(3, 600, 150)
    cp = (1.2, 0.06, 0.08, 0.1, 1.5)
    t = _truth("matern_scaledim", cp, 30, 3, 600, 150)
    r = c["plan"].cond_sim("matern_scaledim", cp, TAU, c["q"], 30, Z_ord=c["Zo"][:, :3], scale=c["scale"], E=c["E"])
    _check("matern_scaledim 3-D", r, t, 3)


def test_a_vector_of_nuggets():
    c = _case()
    covmodel, cp = MATERN15
    tau = 0.05 + 0.1 * np.random.default_rng(3).random(N)               # by ORDERED location
    NN = T.ordered_search(c["lo"], c["q"], 15)
    t = T.truth(c["lo"], tau, c["Zo"][:, :2], c["q"], NN, covmodel, list(cp))
    t["dev"] = t["colour"](c["E"][:, :2])
    r = c["plan"].cond_sim(covmodel, cp, tau, c["q"], 15, Z_ord=c["Zo"][:, :2], E=c["E"][:, :2])
    _check("nugget vector", r, t, 2)


def test_a_column_with_missing_data():
    G, c = _G(), _case()
    covmodel, cp = MATERN15
    z = c["Z"][:, 0].copy()
    miss = np.arange(N) % 3 == 0
    z[miss] = np.nan
    o = c["va"]["ord_z"] - 1
    NN = T.ordered_search(c["lo"], c["q"], 15, eligible=~miss[o])
    t = T.truth(c["lo"], TAU, np.where(miss, 0.0, z)[o], c["q"], NN, covmodel, list(cp))
    out = G.vecchia_cond_sim(z, c["va"], c["q"], list(cp), TAU, covmodel=covmodel, m=15, order="given", eps=c["E"][:, :4])
    assert not miss[o][NN[(NN > 0) & (NN <= N)] - 1].any()                    # no missing datum in a list
    r = dict(mean=out["mean"][:, None], sd=out["sd_cond"], dev=out["draws"] - out["mean"][:, None], n_levels=out["n_levels"],
             n_launches=-1, n_failed=out["n_failed"])
    t["dev"] = t["colour"](c["E"][:, :4])
    # (draws - mean cancels at most one digit here: the deviations are of the size of the means)
    _check("missing data", r, t, 1)
    with pytest.raises(ValueError):
        G.vecchia_cond_sim(np.stack([z, z], axis=1), c["va"], c["q"], list(cp), TAU, covmodel=covmodel)


@functools.lru_cache(maxsize=None)
def _shape(which):
    G = _G()
    c = T.wide_case() if which == "wide" else T.deep_case()
    va = G.vecchia_specify(c["locs"], 10, cond_yz="z")
    plan, lo, zo = _ordered(va, c["Z"])
    NN = T.ordered_search(lo, c["q"], c["m"])
    return c, plan, lo, zo, NN


def test_wide_levels_take_both_launch_forms():
    c, plan, lo, zo, NN = _shape("wide")
    covmodel, cp = MATERN15
    nq = c["q"].shape[0]
    E = np.random.default_rng(2).standard_normal((nq, 2))
    t = T.truth(lo, TAU, zo, c["q"], NN, covmodel, list(cp))
    t["dev"] = t["colour"](E)
    r = plan.cond_sim(covmodel, cp, TAU, c["q"], c["m"], Z_ord=zo, E=E)
    width = np.diff(T.levels(NN, lo.shape[0])[2])
    narrow = width <= 256
    runs = int(narrow[0]) + int((narrow[1:] & ~narrow[:-1]).sum())
    print(f"wide shape: {width.size} levels, widest {width.max()}, {int((~narrow).sum())} wide, {runs} narrow run(s)")
    assert (~narrow).sum() >= 2 and runs >= 1
    assert r["n_levels"] == width.size and r["n_launches"] == int((~narrow).sum()) + runs
    _check("wide levels", r, t, 1)


def test_deep_narrow_run():
    c, plan, lo, zo, NN = _shape("deep")
    covmodel, cp = MATERN15
    nq = c["q"].shape[0]
    E = np.random.default_rng(2).standard_normal((nq, 2))
    t = T.truth(lo, TAU, zo, c["q"], NN, covmodel, list(cp))
    t["dev"] = t["colour"](E)
    r = plan.cond_sim(covmodel, cp, TAU, c["q"], c["m"], Z_ord=zo, E=E)
    width = np.diff(T.levels(NN, lo.shape[0])[2])
    assert width.size >= 40 and width.max() <= 256
    assert r["n_levels"] == width.size and r["n_launches"] == 1
    _check("deep narrow run", r, t, 1)


def test_full_conditioning_is_the_exact_gp_conditional():
    """m = n + nq - 1: the mean is K_po (K_oo + tau)^-1 z and the deviation fields of E = I, taken in two calls, are the lower
    Cholesky factor of the conditional covariance in sweep order"""
    G = _G()
    c = T.exact_case()
    va = G.vecchia_specify(c["locs"], 10, cond_yz="z")
    plan, lo, zo = _ordered(va, c["Z"])
    nq = c["q"].shape[0]
    mean, Fd = T.dense_joint(lo, c["tau"], zo, c["q"], c["covmodel"], c["cp"])
    I = np.eye(nq)
    a = plan.cond_sim(c["covmodel"], c["cp"], c["tau"], c["q"], c["m"], Z_ord=zo, E=I[:, :16])
    b = plan.cond_sim(c["covmodel"], c["cp"], c["tau"], c["q"], c["m"], Z_ord=zo, E=I[:, 16:])
    F = np.hstack([a["dev"], b["dev"]])
    em = float(np.abs(a["mean"] - mean).max() / np.abs(mean).max())
    ef = float(np.abs(F - Fd).max() / np.abs(Fd).max())
    print(f"exact conditional: mean {em:.3g}, Cholesky factor {ef:.3g} (of the largest entry); levels {a['n_levels']}")
    assert a["n_failed"] == 0 and a["n_levels"] == nq and np.all(np.triu(F, 1) == 0)
    assert np.array_equal(a["mean"], b["mean"]) and np.array_equal(a["sd"], b["sd"])
    assert em <= BAR and ef <= BAR


def test_rows_without_predicted_neighbours_are_plan_krige():
    c = _case()
    covmodel, cp = MATERN15
    t = _truth(covmodel, cp, 30)
    rows = np.flatnonzero((t["NN"] <= N).all(axis=1))
    assert rows.size >= 10
    r = c["plan"].cond_sim(covmodel, cp, TAU, c["q"], 30, Z_ord=c["Zo"][:, :3], NNq=t["NN"])
    km, kv, nf = c["plan"].krige(covmodel, cp, TAU, c["q"][rows], 30, Z_ord=c["Zo"][:, :3], NNq=t["NN"][rows])
    assert nf == 0
    em = float((np.abs(r["mean"][rows] - km).max(axis=0) / np.abs(km).max(axis=0)).max())
    ev = float((np.abs(r["sd"][rows] ** 2 - kv) / kv).max())
    print(f"{rows.size} rows of level 0 against Plan.krige: mean {em:.3g}, sd^2 {ev:.3g}")
    assert em <= 2e-8 and ev <= 2e-8


def test_edges():
    c = _case()
    covmodel, cp = MATERN15
    plan = c["plan"]
    one = plan.cond_sim(covmodel, cp, TAU, c["q"][:1], 30, Z_ord=c["Zo"][:, :2], E=c["E"][:1, :3])
    km, kv, _ = plan.krige(covmodel, cp, TAU, c["q"][:1], 30, Z_ord=c["Zo"][:, :2])
    assert one["n_levels"] == 1 and one["n_launches"] == 1 and one["n_failed"] == 0
    assert np.allclose(one["mean"], km, rtol=2e-8, atol=0) and np.allclose(one["sd"] ** 2, kv, rtol=2e-8, atol=0)
    assert np.allclose(one["dev"], one["sd"][:, None] * c["E"][:1, :3], rtol=1e-15, atol=0)
    none = plan.cond_sim(covmodel, cp, TAU, np.zeros((0, 2)), 30, Z_ord=c["Zo"][:, :2], nsim=3)
    assert none["mean"].shape == (0, 2) and none["dev"].shape == (0, 3) and none["n_levels"] == 0 and none["n_failed"] == 0
    t = _truth(covmodel, cp, 30)
    means = plan.cond_sim(covmodel, cp, TAU, c["q"], 30, Z_ord=c["Zo"][:, :3])            # nsim = 0: means only
    assert means["dev"].shape == (NQ, 0)
    _check("nsim=0", means, t, 3)
    # five eligible observations, m = 10: the first rows have fewer than m neighbours
    el = np.zeros(N, dtype=bool)
    el[[3, 500, 777, 1200, 1499]] = True
    NN = T.ordered_search(c["lo"], c["q"][:40], 10, eligible=el)
    assert np.count_nonzero(NN[0]) == 5 and np.count_nonzero(NN[3]) == 8
    tt = T.truth(c["lo"], TAU, c["Zo"][:, :2], c["q"][:40], NN, covmodel, list(cp))
    tt["dev"] = tt["colour"](c["E"][:40, :2])
    r = plan.cond_sim(covmodel, cp, TAU, c["q"][:40], 10, Z_ord=c["Zo"][:, :2], eligible_ord=el, E=c["E"][:40, :2])
    _check("5 eligible, m=10", r, tt, 2)


def test_bit_identity():
    c = _case()
    covmodel, cp = MATERN15
    plan = c["plan"]
    Z = c["Zo"]
    kw = dict(seed=SEED, nsim=NSIM)
    a = plan.cond_sim(covmodel, cp, TAU, c["q"], 30, Z_ord=Z, **kw)

    def same(x, y, cols=slice(None), draws=slice(None)):
        return (np.array_equal(x["mean"], y["mean"][:, cols], equal_nan=True) and np.array_equal(x["sd"], y["sd"], equal_nan=True)
                and np.array_equal(x["dev"], y["dev"][:, draws], equal_nan=True))
    assert same(plan.cond_sim(covmodel, cp, TAU, c["q"], 30, Z_ord=Z, **kw), a)                        # two calls
    assert same(plan.cond_sim(covmodel, cp, TAU, c["q"], 30, Z_ord=Z, chunk=7, **kw), a)               # the factor pass in chunks of 7
    assert same(plan.cond_sim(covmodel, cp, TAU, c["q"], 30, Z_ord=Z[:, 2], **kw), a, cols=slice(2, 3))  # column 2 of 16, alone
    assert same(plan.cond_sim(covmodel, cp, TAU, c["q"], 30, Z_ord=Z[:, 4:7], **kw), a, cols=slice(4, 7))
    one = plan.cond_sim(covmodel, cp, TAU, c["q"], 30, Z_ord=Z, seed=SEED, col0=17, nsim=1)            # draw 17 of 20, alone
    assert same(one, a, draws=slice(17, 18))
    t = _truth(covmodel, cp, 30)
    assert same(plan.cond_sim(covmodel, cp, TAU, c["q"], 30, Z_ord=Z, NNq=t["NN"], **kw), a)           # the caller's lists
    # the caller's normals: a column's bits depend on neither the other columns nor the padded column count
    e = plan.cond_sim(covmodel, cp, TAU, c["q"], 30, Z_ord=Z[:, 0], E=c["E"])
    e1 = plan.cond_sim(covmodel, cp, TAU, c["q"], 30, Z_ord=Z[:, 0], E=c["E"][:, 5])
    assert np.array_equal(e1["dev"][:, 0], e["dev"][:, 5], equal_nan=True)


def test_an_evaluation_stays_what_it_was():
    G, c = _G(), _case()
    covmodel, cp = MATERN15
    plan = c["plan"]
    plan.set_data(c["Zo"][:, 0])
    from gpvecchia_amd import GPV_WANT_LOGLIK_Z, GPV_WANT_U
    plan.eval(covmodel, list(cp), TAU, GPV_WANT_U | GPV_WANT_LOGLIK_Z)
    s0, L0 = plan.sums(), plan.Lentries()
    w0 = plan.whiten(c["Zo"][:, :2], want_E=True)
    r = plan.cond_sim(covmodel, cp, TAU, c["q"], 30, seed=1, nsim=2)             # the plan's own data
    s1, L1 = plan.sums(), plan.Lentries()
    w1 = plan.whiten(c["Zo"][:, :2], want_E=True)
    assert np.array_equal(s0, s1) and np.array_equal(L0, L1)
    assert np.array_equal(w0[0], w1[0]) and w0[1] == w1[1] and np.array_equal(w0[3], w1[3])
    assert np.array_equal(r["mean"][:, 0], plan.cond_sim(covmodel, cp, TAU, c["q"], 30, Z_ord=c["Zo"][:, 0])["mean"][:, 0], equal_nan=True)


def _raw(plan, m, n, NNq=None, nsim=2, ldd=None):
    """the C entry on sentinel-filled outputs: (status, everything it could have written)"""
    from gpvecchia_amd import _lib as L
    c = _case()
    nq = 50
    q = np.asfortranarray(c["q"][:nq])
    cp, nug = np.array(MATERN15[1]), np.array([TAU])
    Z = np.zeros((n, 2), order="F")
    mean, dev, sd = np.full((nq, 2), -77.0, order="F"), np.full((nq, 2), -77.0, order="F"), np.full(nq, -77.0)
    cnt = [C.c_int64(-77) for _ in range(3)]
    nn = None if NNq is None else np.asfortranarray(NNq, dtype=np.int32)
    st = L.lib().gpv_plan_cond_sim(plan._h, b"matern", L.dptr(cp), 3, L.dptr(nug), 1, L.dptr(Z), n, 2, L.dptr(q), nq, m,
                                   None if nn is None else L.iptr(nn), None, None, None, nq, 5, 0, nsim, L.dptr(mean), nq,
                                   L.dptr(dev), nq if ldd is None else ldd, L.dptr(sd), *[C.byref(x) for x in cnt])
    clean = (mean == -77.0).all() and (dev == -77.0).all() and (sd == -77.0).all() and all(x.value == -77 for x in cnt)
    return st, clean


def test_refusals_write_nothing():
    G, c = _G(), _case()
    from gpvecchia_amd import api
    va = c["va"]
    prep = va["U_prep"]
    shard = api.Plan(va["locsord"], prep["revNNarray"], prep["revCond"], row_begin=0, row_end=N // 2)
    sgv_plan = api._plan_for(G.vecchia_specify(c["locs"][:500], 10, cond_yz="SGV"))
    fwd = np.zeros((50, 30), dtype=np.int32)
    fwd[4, 0] = N + 4 + 1                                                        # its own row
    for pl, n, m, kw, want in ((c["plan"], N, 64, {}, GPV_ERR_UNSUPPORTED_M), (shard, N, 30, {}, GPV_ERR_STATE),
                               (sgv_plan, 500, 10, {}, GPV_ERR_STATE), (c["plan"], N, 30, dict(NNq=fwd), GPV_ERR_INDEX),
                               (c["plan"], N, 30, dict(nsim=-1), GPV_ERR_BAD_ARG), (c["plan"], N, 30, dict(ldd=49), GPV_ERR_BAD_ARG)):
        st, clean = _raw(pl, m, n, **kw)
        assert st == want and clean, (m, kw, st)
    fwd[4, 0] = N + 4                                                            # the row before it: served
    st, clean = _raw(c["plan"], 30, N, NNq=fwd)
    assert st == 0 and not clean


def test_vecchia_cond_sim_in_the_callers_order():
    G, c = _G(), _case()
    from gpvecchia_amd import specify as S
    covmodel, cp = MATERN15
    q = c["q"][:200]
    o = S.order_maxmin_exact(q) - 1
    NN = T.ordered_search(c["lo"], q[o], 20)
    t = T.truth(c["lo"], TAU, c["Zo"][:, 0], q[o], NN, covmodel, list(cp))
    mu = 2.5
    out = G.vecchia_cond_sim(c["Z"][:, 0] + mu, c["va"], q, list(cp), TAU, covmodel=covmodel, m=20, nsim=4, seed=SEED, mean=mu,
                             mean_pred=mu)
    assert np.array_equal(out["order"], o) and out["draws"].shape == (200, 4) and out["mean"].shape == (200,)
    dev = t["colour"](G.draws_normals_host(SEED, N, 200, 0, 4).T)
    want_mean, want_draws, want_sd = np.empty(200), np.empty((200, 4)), np.empty(200)
    want_mean[o], want_draws[o], want_sd[o] = t["mean"][:, 0] + mu, t["mean"] + mu + dev, t["sd"]
    em, ed, es = _col_err(out["mean"], want_mean), _col_err(out["draws"], want_draws), _sd_err(out["sd_cond"], want_sd)
    print(f"vecchia_cond_sim, maxmin sweep: mean {em:.3g}, draws {ed:.3g}, sd {es:.3g}; levels {out['n_levels']}")
    assert em <= BAR and ed <= BAR and es <= BAR
    # predict='z': independent noise of variance nugget_pred on top of the same draws
    oz = G.vecchia_cond_sim(c["Z"][:, 0] + mu, c["va"], q, list(cp), TAU, covmodel=covmodel, m=20, nsim=4, seed=SEED, mean=mu,
                            mean_pred=mu, predict="z", nugget_pred=0.25)
    noise = (oz["draws"] - out["draws"])[~np.isnan(want_mean)]
    assert np.array_equal(oz["mean"], out["mean"], equal_nan=True) and 0.15 < noise.var() < 0.4 and abs(noise.mean()) < 0.1
    with pytest.raises(ValueError):
        G.vecchia_cond_sim(c["Z"][:, 0], c["va"], q, list(cp), TAU, order="random")


def test_vecchia_pred_local_with_draws():
    G = _G()
    rng = np.random.default_rng(8)
    n, m = 400, 10
    locs = rng.random((n, 2))
    Sigma = KT.cov_matrix(locs, "matern", [1.0, 0.1, 1.5]) + 0.05 * np.eye(n)
    data = 3.0 + np.linalg.cholesky(Sigma) @ rng.standard_normal(n)
    est = G.vecchia_estimate(data, locs, m=m, output_level=0, maxit=40, cond_yz="z")
    q = rng.random((60, 2))
    plain = G.vecchia_pred(est, q, m=m, local=True)
    pred = G.vecchia_pred(est, q, m=m, local=True, nsim=3, seed=7)
    assert np.array_equal(pred["mean_pred"], plain["mean_pred"]) and np.array_equal(pred["var_pred"], plain["var_pred"])
    assert pred["draws"].shape == (60, 3) and pred["n_failed"] == 0 and "draws" not in plain
    th = np.asarray(est["theta_hat"])
    va = G.vecchia_specify(locs, m, cond_yz="z")
    cs = G.vecchia_cond_sim(est["z"], va, q, th[:-1], th[-1], m=m, nsim=3, seed=7)
    assert np.array_equal(pred["draws"], cs["draws"] + est["beta_hat"][0])
    # the draws scatter about the kriging mean by about the kriging standard deviation
    zs = (pred["draws"] - pred["mean_pred"][:, None]) / np.sqrt(pred["var_pred"])[:, None]
    assert np.abs(zs).max() < 6 and 0.5 < zs.std() < 1.5
    with pytest.raises(ValueError):
        G.vecchia_pred(est, q, m=m, nsim=3)
