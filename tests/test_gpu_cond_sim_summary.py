"""gpv_plan_cond_sim_summary (gpv_csim_summary.hip) on the GPU: summaries of the conditional draws of a cond.yz='z' plan over a
map, folded on the device, and what is built on it (Plan.cond_sim_summary, vecchia_cond_sim_summary).

The method of tests/test_gpu_draws_summary.py: the folds are held to NumPy ON THE SAME BITS.  Plan.cond_sim(seed=, nsim=) on the
same plan and lists gives mean and dev (held to the long-double truth by tests/test_gpu_cond_sim.py), Y = (mean + offset) + dev is
formed on the host, and tests/_csim_summary_truth.py folds it (proven against a literal loop by
tests/test_cond_sim_summary_host.py).  Counts, areas of unit weights, extremes, mean and sd must then be equal EXACTLY; sums
to |got - ref| <= 1e-12 max(1, sum |terms|) against math.fsum (1e-12: that file's bar for the order of summation and a few ulp of
exp, applied to the magnitude a summation error scales with); mc_mean and mc_var to 1e-12 in that file's norm.  One loose check
ties the chain to tests/_csim_truth.py, which never ran on the device: 1e-8.  Every accuracy test prints the maxima it observed
(DESIGN.md §4v).  Observed on an MI355X: reg_total <= 7.7e-16, reg_area <= 6.8e-16, reg_weight <= 2.7e-15, mc_mean <= 2.3e-16,
mc_var <= 1.1e-15; against the long-double truth mc_mean 4.3e-15 and reg_total 2.1e-15."""
import ctypes as C
import functools

import numpy as np
import pytest

import _csim_summary_truth as ST
import _csim_truth as T

pytestmark = pytest.mark.gpu

N, NQ, M, TAU, SEED = 1500, 400, 30, 0.1, 12345
MATERN15 = ("matern", (1.2, 0.07, 1.5))
DUP = 300                                                             # this location is a copy of location 17
THR = (-0.4, 0.1, 0.8)
TOL = 1e-12
K, STEP = ST.CHUNK_ROWS, ST.STEP_ROWS                                 # gpv_csim_summary.h: members per chunk, members per step
GPV_ERR_BAD_ARG, GPV_ERR_UNSUPPORTED_M, GPV_ERR_STATE, GPV_ERR_INDEX = 2, 5, 7, 8
OBSERVED = {}                                                         # the largest errors seen, printed by the tests


def _G():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


@functools.lru_cache(maxsize=None)
def _case():
    """the recipe of tests/test_gpu_cond_sim.py _case(): n = 1500 observations, 400 locations in the order given (5 on
    observations, 5 outside the box, location 300 a copy of location 17), the 'z' plan; one data column; shared and read-only"""
    G = _G()
    from gpvecchia_amd import api
    rng = np.random.default_rng(72)
    locs = rng.random((N, 2))
    Z = rng.standard_normal((N, 16))
    q = rng.random((NQ, 2))
    q[:5] = locs[rng.choice(N, 5, replace=False)]
    q[5:10, :2] = [[-0.3, 0.5], [1.2, 1.1], [0.5, 1.004], [-2.0, -3.0], [1.0 + 1e-9, 0.2]]
    q[DUP] = q[17]
    va = G.vecchia_specify(locs, 10, cond_yz="z")
    plan, lo, zo = api._plan_for(va), va["locsord"], Z[va["ord_z"] - 1][:, 0].copy()
    offset = 0.1 + 0.3 * np.sin(np.arange(NQ))
    for a in (locs, Z, q, lo, zo, offset):
        a.setflags(write=False)
    return dict(locs=locs, z=Z[:, 0], q=q, va=va, plan=plan, lo=lo, zo=zo, offset=offset)


@functools.lru_cache(maxsize=None)
def _draws(nsim=33, col0=0):
    """Plan.cond_sim's mean, dev and sd of the main case, and the latent draws formed on the host"""
    c = _case()
    covmodel, cp = MATERN15
    r = c["plan"].cond_sim(covmodel, cp, TAU, c["q"], M, Z_ord=c["zo"], seed=SEED, col0=col0, nsim=nsim)
    mean = r["mean"][:, 0]
    live = ~np.isnan(mean)
    assert not live[DUP] and 1 <= (~live).sum() <= NQ // 100, "the NaN set is the failed locations and their dependants: at most 1 %"
    mu = mean + c["offset"]
    Y = mu[:, None] + r["dev"]
    assert np.array_equal(np.isnan(Y), np.repeat(~live[:, None], nsim, axis=1))
    return dict(mean=mean, mu=mu, live=live, Y=Y, sd=r["sd"], n_levels=r["n_levels"], n_failed=r["n_failed"])


@functools.lru_cache(maxsize=None)
def _regions():
    """the regions of the main case as index arrays, and weights of both signs"""
    d = _draws()
    dead = np.flatnonzero(~d["live"])
    rng = np.random.default_rng(4)
    pick = lambda k: np.sort(rng.choice(NQ, k, replace=False))
    regs = [np.zeros(0, dtype=np.int64), np.array([7]), dead[:2] if dead.size >= 2 else np.array([DUP, DUP]),
            np.arange(DUP - 5, DUP + 6), np.arange(NQ), np.arange(0, 250), np.arange(200, NQ)]
    regs += [pick(k) for k in (STEP - 1, STEP, STEP + 1, K - 1, K, K + 1, 2 * K - 1, 2 * K, 2 * K + 1)]
    regs.append(rng.permutation(NQ)[:150])                               # members in no order
    assert not d["live"][regs[2]].any() and d["live"][regs[3]].sum() >= 8 and not d["live"][regs[3]].all()
    wts = [0.25 + rng.random(r.size) for r in regs]
    for w in wts:
        w[::3] *= -1.0
    return regs, wts


def _run(ndraws, col0=0, link=0, thr=THR, regions=None, offset=True, **kw):
    c = _case()
    covmodel, cp = MATERN15
    return c["plan"].cond_sim_summary(covmodel, cp, TAU, c["q"], M, ndraws, seed=SEED, col0=col0, Z_ord=c["zo"],
                                      offset=c["offset"] if offset else None, link=link, thresholds=thr, regions=regions, **kw)


def _note(name, err):
    OBSERVED[name] = max(OBSERVED.get(name, 0.0), float(err))


def _close(name, got, ref, tol=TOL):
    """tests/test_gpu_draws_summary.py's norm; the NaN sets must agree"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), name
    ok = ~np.isnan(ref)
    err = float(np.max(np.abs(got[ok] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok])))) if ok.any() else 0.0
    print(f"{name}: max |diff| / max(1, |ref|) = {err:.3e}")
    _note(name.split(":")[-1].strip(), err)
    assert err <= tol, (name, err)


def _sum_close(name, got, ref, mag, tol=TOL):
    got, ref, mag = np.asarray(got), np.asarray(ref), np.asarray(mag)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = float(np.max(np.abs(got - ref) / np.maximum(1.0, mag))) if ref.size else 0.0
    print(f"{name}: max |diff| / max(1, sum |terms|) = {err:.3e}")
    _note(name.split(":")[-1].strip(), err)
    assert err <= tol, (name, err)


def _check(tag, res, Y, mu, live, sd, link, thr, csr, unit):
    """everything a call returns against the NumPy folds of the same draws"""
    loc = ST.location_truth(Y, mu, live, link, thr)
    assert np.array_equal(res["mean"], mu, equal_nan=True) and np.array_equal(res["sd"], sd, equal_nan=True), tag
    assert np.array_equal(res["exceed"], loc["exceed"], equal_nan=True), tag           # counts: exactly
    _close(f"{tag}: mc_mean", res["mc_mean"], loc["mc_mean"])
    _close(f"{tag}: mc_var", res["mc_var"], loc["mc_var"])
    assert np.all(res["mc_var"][live] >= 0.0)
    if csr is None:
        return loc
    reg = ST.region_truth(Y, live, link, thr, *csr)
    assert np.array_equal(res["reg_count"], reg["count"]), tag
    assert np.array_equal(res["reg_max"], reg["max"], equal_nan=True) and np.array_equal(res["reg_min"], reg["min"], equal_nan=True), tag
    if unit:
        assert np.array_equal(res["reg_area"], reg["area"]), tag                      # areas of unit weights: exactly
        assert np.array_equal(res["reg_weight"], reg["count"].astype(np.float64)), tag
    _sum_close(f"{tag}: reg_total", res["reg_total"], reg["total"], reg["total_mag"])
    _sum_close(f"{tag}: reg_area", res["reg_area"], reg["area"], reg["area_mag"])
    _sum_close(f"{tag}: reg_weight", res["reg_weight"], reg["weight"], np.abs(reg["weight"]))
    return loc


# ---- 1, 2. the main case: draw counts around the batch, regions of every kind, with and without weights ------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ndraws", [2, 15, 16, 17, 33])
def test_main_case_against_numpy_on_the_same_draws(ndraws, weighted):
    d = _draws()
    regs, wts = _regions()
    csr = ST.csr(regs, wts if weighted else None)
    res = _run(ndraws, regions=csr)
    assert res["reg_total"].shape == (len(regs), ndraws) and res["reg_area"].shape == (len(THR), len(regs), ndraws)
    assert res["n_levels"] == d["n_levels"] and res["n_failed"] == d["n_failed"] >= 1
    loc = _check(f"N={ndraws} weighted={weighted}", res, d["Y"][:, :ndraws], d["mu"], d["live"], d["sd"], 0, THR, csr, not weighted)
    for t in range(len(THR)):                                              # the thresholds cut through the draws
        e = loc["exceed"][t][d["live"]]
        assert e.min() < 1.0 and e.max() > 0.0 and not np.all(e == 0.0) and not np.all(e == 1.0)
    # the rules of the contract, on what came back
    assert np.isnan(res["mc_mean"][~d["live"]]).all() and np.isnan(res["exceed"][:, ~d["live"]]).all()
    assert np.all(res["reg_total"][0] == 0.0) and np.all(res["reg_area"][:, 0] == 0.0) and np.isnan(res["reg_max"][0]).all()
    assert res["reg_count"][0] == 0 and res["reg_count"][2] == 0 and res["reg_weight"][2] == 0.0 and np.isnan(res["reg_min"][2]).all()
    assert np.all(res["reg_total"][2] == 0.0) and res["reg_count"][4] == d["live"].sum()
    assert np.array_equal(res["reg_max"][1], d["Y"][7, :ndraws]) and np.array_equal(res["reg_min"][1], d["Y"][7, :ndraws])


# ---- 3, 4. the links; no threshold and eight --------------------------------------------------------------------------------
@pytest.mark.parametrize("link", [1, 2])
def test_links(link):
    d = _draws()
    regs, wts = _regions()
    csr = ST.csr(regs, wts)
    res = _run(33, link=link, regions=csr)
    _check(f"link={link}", res, d["Y"], d["mu"], d["live"], d["sd"], link, THR, csr, False)
    lat = _run(33, link=0, regions=csr)                                    # thresholds and extremes are on the latent scale
    for k in ("exceed", "reg_max", "reg_min", "reg_area", "reg_weight", "reg_count", "mean", "sd"):
        assert np.array_equal(res[k], lat[k], equal_nan=True), k


@pytest.mark.parametrize("nthr", [0, 8])
def test_no_threshold_and_eight(nthr):
    d = _draws()
    regs, wts = _regions()
    csr = ST.csr(regs, None)
    thr = tuple(np.linspace(-1.0, 1.5, nthr))
    res = _run(17, thr=thr, regions=csr)
    assert res["exceed"].shape == (nthr, NQ) and res["reg_area"].shape == (nthr, len(regs), 17)
    _check(f"nthr={nthr}", res, d["Y"][:, :17], d["mu"], d["live"], d["sd"], 0, thr, csr, True)
    none = _run(17, thr=thr, regions=None)                                  # no region at all
    assert none["reg_total"].shape == (0, 17) and np.array_equal(none["mc_mean"], res["mc_mean"], equal_nan=True)


# ---- a large region: many chunks, the second stage --------------------------------------------------------------------------
def test_large_regions_on_the_wide_shape():
    G = _G()
    from gpvecchia_amd import api
    c = T.wide_case()
    covmodel, cp = MATERN15
    va = G.vecchia_specify(c["locs"], 10, cond_yz="z")
    plan, zo = api._plan_for(va), c["Z"][va["ord_z"] - 1]
    nq, m, nd = c["q"].shape[0], c["m"], 17
    r = plan.cond_sim(covmodel, cp, TAU, c["q"], m, Z_ord=zo, seed=SEED, nsim=nd)
    mean = r["mean"][:, 0]
    live = ~np.isnan(mean)
    assert r["n_failed"] == 0 and live.all() and r["n_levels"] >= 10
    Y = mean[:, None] + r["dev"]
    lab = np.arange(nq) % 200
    regs = [np.arange(nq)] + [np.flatnonzero(lab == k) for k in range(200)]
    assert all(x.size == 100 for x in regs[1:]) and regs[0].size > 100 * K
    w = 0.5 + np.random.default_rng(6).random(nq)
    w[::7] *= -1.0
    for weighted in (False, True):
        csr = ST.csr(regs, [w[x] for x in regs] if weighted else None)
        res = plan.cond_sim_summary(covmodel, cp, TAU, c["q"], m, nd, seed=SEED, Z_ord=zo, link=1 if weighted else 0, thresholds=THR,
                                    regions=csr)
        assert res["n_launches"] == r["n_launches"] and res["n_levels"] == r["n_levels"]
        _check(f"wide weighted={weighted}", res, Y, mean, live, r["sd"], 1 if weighted else 0, THR, csr, not weighted)


# ---- identical bytes ------------------------------------------------------------------------------------------------------------
REG_KEYS = ("reg_total", "reg_max", "reg_min", "reg_area")
ALL_KEYS = REG_KEYS + ("mean", "sd", "mc_mean", "mc_var", "exceed", "reg_weight", "reg_count")


def test_identical_bytes():
    c, d = _case(), _draws()
    covmodel, cp = MATERN15
    regs, wts = _regions()
    csr = ST.csr(regs, wts)
    a = _run(33, link=1, regions=csr)
    same = lambda x, y, keys=ALL_KEYS: all(np.array_equal(x[k], y[k], equal_nan=True) for k in keys)
    assert same(_run(33, link=1, regions=csr), a)                                         # two calls
    assert same(_run(33, link=1, regions=csr, chunk=7), a)                                # the factor pass in chunks of 7
    NN = T.ordered_search(c["lo"], c["q"], M)
    assert same(_run(33, link=1, regions=csr, NNq=NN), a)                                 # the caller's lists
    two = _run(2, col0=17, link=1, regions=csr)                                           # draws 17 and 18 of 33, alone
    for k in REG_KEYS:
        assert np.array_equal(two[k], a[k][..., 17:19], equal_nan=True), k
    nine = [regs[5], regs[0], regs[12], regs[4], regs[11], regs[1], regs[13], regs[6], regs[2]]
    w9 = [wts[5], wts[0], wts[12], wts[4], wts[11], wts[1], wts[13], wts[6], wts[2]]
    b = _run(33, link=1, regions=ST.csr(nine, w9))
    for pos, r in ((2, 12), (3, 4), (4, 11), (6, 13)):                                     # a region alone against one of nine
        alone = _run(33, link=1, regions=ST.csr([regs[r]], [wts[r]]))
        for k in REG_KEYS:
            assert np.array_equal(alone[k][..., 0, :], b[k][..., pos, :], equal_nan=True), (k, r)
            assert np.array_equal(alone[k][..., 0, :], a[k][..., r, :], equal_nan=True), (k, r)
    # gpv_plan_cond_sim in the same process: mean and sd bit for bit (no offset)
    plain = _run(33, offset=False)
    assert np.array_equal(plain["mean"], d["mean"], equal_nan=True) and np.array_equal(plain["sd"], d["sd"], equal_nan=True)
    # the draws beyond the first batch are those of gpv_plan_cond_sim at the same columns
    late = _draws(2, 17)
    assert np.array_equal(late["Y"], d["Y"][:, 17:19], equal_nan=True)


def test_an_evaluation_stays_what_it_was():
    c = _case()
    covmodel, cp = MATERN15
    plan = c["plan"]
    plan.set_data(c["zo"])
    from gpvecchia_amd import GPV_WANT_LOGLIK_Z, GPV_WANT_U
    plan.eval(covmodel, list(cp), TAU, GPV_WANT_U | GPV_WANT_LOGLIK_Z)
    two = np.stack([c["zo"], 2.0 * c["zo"]], axis=1)
    s0, L0, st0 = plan.sums(), plan.Lentries(), plan.factor_stamp()
    w0 = plan.whiten(two, want_E=True)
    regs, wts = _regions()
    r = plan.cond_sim_summary(covmodel, cp, TAU, c["q"], M, 17, seed=1, thresholds=THR, regions=ST.csr(regs, wts))    # the plan's data
    s1, L1, st1 = plan.sums(), plan.Lentries(), plan.factor_stamp()
    w1 = plan.whiten(two, want_E=True)
    assert np.array_equal(s0, s1) and np.array_equal(L0, L1) and st0 == st1
    assert np.array_equal(w0[0], w1[0]) and w0[1] == w1[1] and np.array_equal(w0[3], w1[3])
    given = plan.cond_sim_summary(covmodel, cp, TAU, c["q"], M, 17, seed=1, Z_ord=c["zo"], thresholds=THR, regions=ST.csr(regs, wts))
    assert all(np.array_equal(r[k], given[k], equal_nan=True) for k in ALL_KEYS)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _raw(plan, n, m=M, ndraws=4, col0=0, ncols=1, link=0, nthr=2, nreg=2, regptr=(0, 3, 5), regidx=(0, 1, 2, 48, 49), regw=None, NNq=None,
         null=()):
    """the C entry on canary-filled outputs: (status, nothing was written)"""
    from gpvecchia_amd import _lib as L
    c = _case()
    nq = 50
    q = np.asfortranarray(c["q"][:nq])
    cp, nug = np.array(MATERN15[1]), np.array([TAU])
    Z = np.zeros(n)
    nd, nr, nt = max(ndraws, 0), max(nreg, 0), max(nthr, 0)
    out = dict(mean=np.full(nq, -77.0), sd=np.full(nq, -77.0), mc_mean=np.full(nq, -77.0), mc_var=np.full(nq, -77.0),
               exceed=np.full(nq * max(nt, 1), -77.0), reg_total=np.full(nr * nd + 1, -77.0), reg_max=np.full(nr * nd + 1, -77.0),
               reg_min=np.full(nr * nd + 1, -77.0), reg_area=np.full(nr * nd * nt + 1, -77.0), reg_weight=np.full(nr + 1, -77.0))
    cnt = np.full(nr + 1, -77, dtype=np.int64)
    three = [C.c_int64(-77) for _ in range(3)]
    thr = np.array([0.0, 0.5, 0, 0, 0, 0, 0, 0, 0, 0])
    rp, ri = np.array(regptr, dtype=np.int64), np.array(regidx, dtype=np.int32)
    rw = None if regw is None else np.array(regw, dtype=np.float64)
    nn = None if NNq is None else np.asfortranarray(NNq, dtype=np.int32)
    ptr = lambda k: None if k in null else L.dptr(out[k])
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    st = L.lib().gpv_plan_cond_sim_summary(
        plan._h, b"matern", L.dptr(cp), 3, L.dptr(nug), 1, L.dptr(Z), ncols, L.dptr(q), nq, m, None if nn is None else L.iptr(nn), None, None,
        5, col0, ndraws, None, link, nthr, None if "thr" in null else L.dptr(thr), nreg, None if "regptr" in null else rp.ctypes.data_as(i64p),
        None if "regidx" in null else ri.ctypes.data_as(i32p), None if rw is None else L.dptr(rw), ptr("mean"), ptr("sd"), ptr("mc_mean"),
        ptr("mc_var"), ptr("exceed"), ptr("reg_total"), ptr("reg_max"), ptr("reg_min"), ptr("reg_area"), ptr("reg_weight"),
        None if "reg_count" in null else cnt.ctypes.data_as(i64p), *[C.byref(x) for x in three])
    clean = all((v == -77.0).all() for v in out.values()) and (cnt == -77).all() and all(x.value == -77 for x in three)
    return st, clean


def test_refusals_write_nothing():
    G, c = _G(), _case()
    from gpvecchia_amd import api
    va = c["va"]
    prep = va["U_prep"]
    shard = api.Plan(va["locsord"], prep["revNNarray"], prep["revCond"], row_begin=0, row_end=N // 2)
    sgv_plan = api._plan_for(G.vecchia_specify(c["locs"][:500], 10, cond_yz="SGV"))
    fwd = np.zeros((50, M), dtype=np.int32)
    fwd[4, 0] = N + 4 + 1                                                        # its own row
    BAD, IDX, STATE, UM = GPV_ERR_BAD_ARG, GPV_ERR_INDEX, GPV_ERR_STATE, GPV_ERR_UNSUPPORTED_M
    p = c["plan"]
    cases = [(p, N, dict(ndraws=1), BAD), (p, N, dict(ndraws=0), BAD), (p, N, dict(col0=-1), BAD), (p, N, dict(col0=2 ** 63 - 2), BAD),
             (p, N, dict(ncols=2), BAD), (p, N, dict(link=3), BAD), (p, N, dict(link=-1), BAD), (p, N, dict(nthr=9), BAD),
             (p, N, dict(nthr=-1), BAD), (p, N, dict(null=("thr",)), BAD), (p, N, dict(null=("exceed",)), BAD),
             (p, N, dict(null=("mean",)), BAD), (p, N, dict(null=("sd",)), BAD), (p, N, dict(null=("mc_mean",)), BAD),
             (p, N, dict(null=("mc_var",)), BAD), (p, N, dict(null=("regptr",)), BAD), (p, N, dict(null=("regidx",)), BAD),
             (p, N, dict(null=("reg_total",)), BAD), (p, N, dict(null=("reg_max",)), BAD), (p, N, dict(null=("reg_min",)), BAD),
             (p, N, dict(null=("reg_area",)), BAD), (p, N, dict(null=("reg_weight",)), BAD), (p, N, dict(null=("reg_count",)), BAD),
             (p, N, dict(nreg=-1), BAD), (p, N, dict(regptr=(1, 3, 5)), BAD), (p, N, dict(regptr=(0, 4, 3)), BAD),
             (p, N, dict(regw=(1.0, np.inf, 1.0, 1.0, 1.0)), BAD), (p, N, dict(regw=(1.0, 1.0, np.nan, 1.0, 1.0)), BAD),
             (p, N, dict(regidx=(0, 1, 2, 48, 50)), IDX), (p, N, dict(regidx=(0, -1, 2, 48, 49)), IDX), (p, N, dict(NNq=fwd), IDX),
             (p, N, dict(m=64), UM), (shard, N, {}, STATE), (sgv_plan, 500, dict(m=10), STATE)]
    for pl, n, kw, want in cases:
        st, clean = _raw(pl, n, **kw)
        assert st == want and clean, (kw, st, clean)
    st, clean = _raw(p, N)                                                       # the same arguments, served
    assert st == 0 and not clean
    fwd[4, 0] = N + 4                                                            # the row before it: served
    st, clean = _raw(p, N, NNq=fwd, regw=(1.0, -2.0, 0.5, 1.0, 1.0))
    assert st == 0 and not clean


# ---- the public function ----------------------------------------------------------------------------------------------------------
def test_vecchia_cond_sim_summary_in_the_callers_order():
    G, c = _G(), _case()
    covmodel, cp = MATERN15
    n_p, nsim, mu = 200, 18, 2.5
    q = c["q"][:n_p]
    rng = np.random.default_rng(11)
    mean_pred = mu + 0.2 * rng.standard_normal(n_p)
    lab = rng.integers(-1, 6, n_p)
    lab[lab == 4] = 9                                                            # labels need not be consecutive
    area = 0.5 + rng.random(n_p)
    kw = dict(covmodel=covmodel, m=20, seed=SEED, mean=mu, mean_pred=mean_pred)
    cs = G.vecchia_cond_sim(c["z"] + mu, c["va"], q, list(cp), TAU, nsim=nsim, **kw)
    Y = cs["draws"]
    live = ~np.isnan(cs["mean"])
    assert live.sum() >= n_p - 2
    for link, gname in ((0, None), (1, "exp")):
        out = G.vecchia_cond_sim_summary(c["z"] + mu, c["va"], q, list(cp), TAU, nsim=nsim, link=gname, thresholds=[2.2, 2.9], regions=lab,
                                         weights=area, **kw)
        assert np.array_equal(out["order"], cs["order"]) and out["n_levels"] == cs["n_levels"] and out["n_failed"] == cs["n_failed"]
        assert list(out["region_ids"]) == [0, 1, 2, 3, 5, 9]
        regs = [np.flatnonzero(lab == k) for k in out["region_ids"]]
        csr = ST.csr(regs, [area[x] for x in regs])
        res = dict(mean=out["mean"], sd=out["sd_cond"], mc_mean=out["mc_mean"], mc_var=out["mc_var"], exceed=out["exceed"],
                   reg_total=out["region_total"], reg_max=out["region_max"], reg_min=out["region_min"], reg_area=out["region_area"],
                   reg_weight=out["region_weight"], reg_count=out["region_count"])
        if link == 1:                                                            # the extremes come back linked
            assert np.array_equal(res["reg_max"], np.exp(lat["region_max"]), equal_nan=True)
            assert np.array_equal(res["reg_min"], np.exp(lat["region_min"]), equal_nan=True)
            res["reg_max"], res["reg_min"] = lat["region_max"], lat["region_min"]
        _check(f"public link={link}", res, Y, cs["mean"], live, cs["sd_cond"], link, [2.2, 2.9], csr, False)
        assert np.array_equal(out["region_mean"], out["region_total"] / out["region_weight"][:, None])
        lat = out
    # a list of regions with weights per member, and draws from a later column on
    regs = [np.array([5, 3, 150]), np.zeros(0, dtype=int), np.arange(100, 200)]
    wl = [np.array([1.0, -2.0, 0.5]), np.zeros(0), np.full(100, 0.01)]
    late = G.vecchia_cond_sim_summary(c["z"] + mu, c["va"], q, list(cp), TAU, nsim=3, col0=15, regions=regs, weights=wl, **kw)
    ref = ST.region_truth(Y[:, 15:18], live, 0, [], *ST.csr(regs, wl))
    assert np.array_equal(late["region_max"], ref["max"], equal_nan=True) and np.array_equal(late["region_count"], ref["count"])
    _sum_close("public, list of regions: reg_total", late["region_total"], ref["total"], ref["total_mag"])
    whole = G.vecchia_cond_sim_summary(c["z"] + mu, c["va"], q, list(cp), TAU, nsim=3, col0=15, **kw)       # regions=None: everything
    assert whole["region_total"].shape == (1, 3) and whole["region_count"][0] == live.sum()
    assert np.array_equal(whole["region_max"][0], np.nanmax(Y[:, 15:18], axis=0))
    with pytest.raises(ValueError):
        G.vecchia_cond_sim_summary(c["z"], c["va"], q, list(cp), TAU, link="probit")


# ---- against the truth that never ran on the device ---------------------------------------------------------------------------
def test_loose_check_against_the_cpu_only_truth():
    G, c = _G(), _case()
    covmodel, cp = MATERN15
    nd = 17
    NN = T.ordered_search(c["lo"], c["q"], M)
    t = T.truth(c["lo"], TAU, c["zo"], c["q"], NN, covmodel, list(cp))
    dev = t["colour"](G.draws_normals_host(SEED, N, NQ, 0, nd).T)
    mu = t["mean"][:, 0] + c["offset"]
    live = ~t["nan"]
    assert 1 <= (~live).sum() <= NQ // 100
    Y = mu[:, None] + np.asarray(dev, dtype=np.float64)
    regs, wts = _regions()
    csr = ST.csr(regs, wts)
    res = _run(nd, link=1, regions=csr)
    assert np.array_equal(np.isnan(res["mean"]), ~live)
    loc = ST.location_truth(Y, mu, live, 1, THR)
    reg = ST.region_truth(Y, live, 1, THR, *csr)
    e_mean = float(np.abs(res["mc_mean"][live] - loc["mc_mean"][live]).max() / np.abs(loc["mc_mean"][live]).max())
    e_tot = float((np.abs(res["reg_total"] - reg["total"]).max(axis=0) / np.abs(reg["total"]).max(axis=0)).max())
    print(f"against the long-double truth: mc_mean {e_mean:.3g}, reg_total {e_tot:.3g} (of the column's largest magnitude)")
    assert e_mean <= 1e-8 and e_tot <= 1e-8
    assert np.array_equal(res["reg_count"], reg["count"])


def test_print_observed_maxima():
    """(last in the file) the largest errors the tests above saw, for DESIGN.md §4v"""
    for k in sorted(OBSERVED):
        print(f"observed maximum, {k}: {OBSERVED[k]:.3e}")
