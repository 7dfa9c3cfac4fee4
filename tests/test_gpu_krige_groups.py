"""gpv_plan_krige_groups (gpv_krige_groups.hip) on the GPU: grouped local kriging of a cond.yz='z' plan, and what is built on it
(Plan.krige_groups, vecchia_krige_groups, vecchia_pred(local=True, groups=)).

Truth: tests/_krige_groups_truth.py (the anchor, the search definition and a long-double Cholesky per group, proven on the CPU
by tests/test_krige_groups_truth_host.py).  Observations: n = 6000 uniform points, tau = 0.1, 16 data columns; about 60 groups a
case, their members scattered in a 0.05-wide cell; in every case one member lies on an observation, one group holds two
identical members and two groups lie outside the bounding box.

The bar is the project's contract figure, 1e-8: the mean relative to l1_i ||z||_inf, the variance to itself, a covariance to
sqrt(S_ii S_jj), the group mean to sum |w_i| l1_i ||z||_inf, the group variance to (sum |w_i| sqrt(S_ii))^2.  Every accuracy
test prints the maxima it observed (DESIGN.md §4t records them).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import _krige_groups_truth as GT
import _krige_truth as KT

pytestmark = pytest.mark.gpu

N, TAU, BAR = 6000, 0.1, 1e-8
GPV_ERR_BAD_ARG, GPV_ERR_UNSUPPORTED_M, GPV_ERR_STATE, GPV_ERR_INDEX = 2, 5, 7, 8
MATERN15 = ("matern", (1.2, 0.07, 1.5))
# group sizes per list length m: every row count m + g at a bucket edge (2, 16, 17, 32, 33, 64) and sizes between
SIZES = {1: (1, 15, 16, 31, 32, 63, 5, 2), 15: (1, 2, 17, 18, 49, 9), 16: (1, 16, 17, 48), 30: (1, 2, 3, 34, 7), 63: (1,),
         10: (1, 4, 7, 25)}


def _G():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


def test_row_limit():
    _G()
    from gpvecchia_amd import _lib as L
    from gpvecchia_amd import api
    assert L.lib().gpv_krige_groups_max_rows() == api.KRIGE_GROUPS_MAX_ROWS == 64


@functools.lru_cache(maxsize=None)
def _case(dim=2):
    """observations, 16 data columns and the 'z' specification (m = 10), shared and read-only"""
    G = _G()
    rng = np.random.default_rng(70 + dim)
    locs = rng.random((N, dim))
    Z = rng.standard_normal((N, 16))
    scale = {2: None, 3: np.array([0.06, 0.08, 0.1]), 5: np.array([0.3, 0.4, 0.5, 0.6, 0.7])}[dim]
    va = G.vecchia_specify(locs, 10, cond_yz="z", scale=scale)
    for a in (locs, Z):
        a.setflags(write=False)
    return dict(locs=locs, Z=Z, va=va, scale=scale, dim=dim)


@functools.lru_cache(maxsize=None)
def _layout(m, dim=2, ngroups=60):
    """the groups of a case: (q (nq, dim) with the members of a group contiguous, gptr); sizes cycle through SIZES[m]"""
    c = _case(dim)
    rng = np.random.default_rng(100 * m + dim)
    sizes = np.array([SIZES[m][k % len(SIZES[m])] for k in range(ngroups)])
    gptr = np.concatenate([[0], np.cumsum(sizes)])
    centre = rng.random((ngroups, dim))
    centre[2, :2], centre[3, :2] = [-0.3, 0.5], [1.2, 1.1]           # outside the bounding box
    q = np.repeat(centre, sizes, axis=0) + 0.05 * (rng.random((gptr[-1], dim)) - 0.5)
    q[gptr[4]] = c["locs"][17]                                       # a member on an observation
    big = int(np.nonzero(sizes >= 2)[0][0]) if (sizes >= 2).any() else None
    if big is not None:
        q[gptr[big] + 1] = q[gptr[big]]                              # two identical members
    q.setflags(write=False)
    return q, gptr


def _weights(kind, gptr, seed=5):
    g = np.diff(gptr)
    if kind == "default":
        return None, np.repeat(1.0 / g, g)
    rng = np.random.default_rng(seed)
    if kind == "unequal":
        w = 0.1 + rng.random(gptr[-1])
    else:                                                            # a contrast: +1, -1, +1, ... (a lone member: +1)
        w = np.concatenate([(-1.0) ** np.arange(k) for k in g])
    return w, w


def _errors(mean, var, gmean, gvar, cov, truth, gptr, w, zmax):
    """the five relative errors of the bar, each the maximum over the groups; cov: the packed lower triangles or None"""
    e = dict(mean=0.0, var=0.0, cov=0.0, gmean=0.0, gvar=0.0)
    at = 0
    for k, t in enumerate(truth):
        a, b = gptr[k], gptr[k + 1]
        g = b - a
        assert not t["failed"]
        s = GT.scales(t, w[a:b], zmax)
        with np.errstate(invalid="ignore", divide="ignore"):
            em = np.abs(mean[a:b] - t["mean"]) / s["mean"]
        em = np.where(np.abs(mean[a:b] - t["mean"]) == 0, 0.0, em)           # (an empty neighbour list: 0 against a scale of 0)
        e["mean"] = max(e["mean"], float(em.max()))
        e["var"] = max(e["var"], float((np.abs(var[a:b] - np.diag(t["cov"])) / s["var"]).max()))
        dg = np.abs(gmean[k] - w[a:b] @ t["mean"])
        e["gmean"] = max(e["gmean"], float(np.where(dg == 0, 0.0, dg / s["gmean"] if s["gmean"] > 0 else np.inf).max()))
        e["gvar"] = max(e["gvar"], abs(gvar[k] - w[a:b] @ t["cov"] @ w[a:b]) / s["gvar"])
        if cov is not None:
            il = np.tril_indices(g)
            e["cov"] = max(e["cov"], float((np.abs(cov[at:at + il[0].size] - t["cov"][il]) / s["cov"][il]).max()))
            at += il[0].size
    return e


def _ordered(c, nuggets=TAU):
    from gpvecchia_amd import api
    va = c["va"]
    o = va["ord_z"] - 1
    nug = np.asarray(nuggets, dtype=np.float64)
    return api._plan_for(va), c["Z"][o], (nug if nug.ndim == 0 else nug[o])


def _run_and_check(label, covmodel, cp, m, R, dim=2, weights="default", nuggets=TAU, eligible=None):
    c = _case(dim)
    q, gptr = _layout(m, dim)
    plan, Zord, nug_ord = _ordered(c, nuggets)
    w_arg, w = _weights(weights, gptr)
    o = c["va"]["ord_z"] - 1
    Z = c["Z"][:, :R]
    out = plan.krige_groups(covmodel, list(cp), nug_ord, q, gptr, m, Z_ord=Zord[:, :R], weights=w_arg, scale=c["scale"],
                            eligible_ord=None if eligible is None else eligible[o], want_cov=True)
    NN = GT.group_nn(c["locs"], q, gptr, m, eligible=eligible, scale=c["scale"])
    truth = GT.krige_groups_ld(c["locs"], nuggets, Z, q, gptr, NN, covmodel, list(cp))
    e = _errors(*out[:5], truth, gptr, w, np.abs(Z).max())
    print(f"krige_groups {label}: {covmodel} {cp} m={m} R={R} dim={dim} weights={weights}: " +
          ", ".join(f"{k} {v:.3g}" for k, v in e.items()) + f"; min var / sigma^2 {np.min(out[1]) / cp[0]:.3g}")
    assert out[5] == 0 and out[0].shape == (gptr[-1], R) and out[2].shape == (len(gptr) - 1, R)
    assert all(v <= BAR for v in e.values()), e
    return out, truth


@pytest.mark.parametrize("m,R", [(1, 16), (15, 3), (16, 1), (30, 16), (63, 3)])
def test_bucket_edges_agree_with_the_long_double_truth(m, R):
    """m + g in {2, 16, 17, 32, 33, 64}: (m, g) = (1, 1), (1, 15), (15, 1), (1, 16), (15, 2), (30, 2), (16, 17), (30, 34), (1, 63),
    (15, 49), (16, 48), (63, 1); the calls at m = 1, 15 and 16 hold groups of all three buckets"""
    out, truth = _run_and_check("edges", *MATERN15, m, R)
    q, gptr = _layout(m)
    if m != 63:                                                      # the two identical members: equal rows and columns
        k = int(np.nonzero(np.diff(gptr) >= 2)[0][0])
        g = gptr[k + 1] - gptr[k]
        S = np.zeros((g, g))
        at = int(sum(s * (s + 1) // 2 for s in np.diff(gptr)[:k]))
        S[np.tril_indices(g)] = out[4][at:at + g * (g + 1) // 2]
        S = S + np.tril(S, -1).T
        assert np.abs(S[0] - S[1]).max() <= BAR * S[0, 0] and np.array_equal(out[0][gptr[k]], out[0][gptr[k] + 1])
        assert out[1][gptr[k]] == out[1][gptr[k] + 1] > 0


FAMILIES = [("matern", (1.2, 0.1, 0.5)), ("matern", (1.2, 0.05, 2.5)), ("matern", (1.2, 0.06, 0.8)), ("esqe", (0.8, 0.1, 0.4, 0.05))]


@pytest.mark.parametrize("covmodel,cp", FAMILIES)
def test_families_agree_with_the_truth(covmodel, cp):
    _run_and_check("family", covmodel, cp, 15, 3)


def test_general_smoothness_at_the_longest_rows():
    _run_and_check("family", "matern", (1.2, 0.06, 0.8), 30, 1)


def test_scaledim_in_three_dimensions_with_scale():
    _run_and_check("scaledim", "matern_scaledim", (1.2, 0.06, 0.08, 0.1, 1.5), 15, 3, dim=3)


def test_scaledim_in_five_dimensions():
    """dim > 3: the records hold coordinates only, the data come from the call's columns"""
    _run_and_check("scaledim", "matern_scaledim", (1.2, 0.3, 0.4, 0.5, 0.6, 0.7, 1.5), 15, 3, dim=5)


def test_a_vector_of_nuggets():
    _run_and_check("nuggets", *MATERN15, 30, 3, nuggets=0.05 + 0.1 * np.random.default_rng(3).random(N))


@pytest.mark.parametrize("weights", ["unequal", "contrast"])
def test_weights(weights):
    _run_and_check("weights", *MATERN15, 30, 3, weights=weights)
    _run_and_check("weights", *MATERN15, 1, 3, weights=weights)


def test_short_conditioning_sets():
    """an eligibility mask that leaves 5 observations with m = 10: every list is 0-padded"""
    el = np.zeros(N, dtype=bool)
    el[[11, 505, 1999, 3000, 5998]] = True
    _run_and_check("short", *MATERN15, 10, 3, eligible=el)
    # the same through missing data of the one column of vecchia_krige_groups
    G, c = _G(), _case()
    q, gptr = _layout(10)
    z = np.where(el, c["Z"][:, 0], np.nan)
    lab = np.repeat(np.arange(len(gptr) - 1), np.diff(gptr))
    out = G.vecchia_krige_groups(z, c["va"], q, lab, list(MATERN15[1]), TAU, m=10)
    plan, Zord, _ = _ordered(c)
    ref = plan.krige_groups(*MATERN15, TAU, q, gptr, 10, Z_ord=Zord[:, 0], eligible_ord=el[c["va"]["ord_z"] - 1])
    assert np.array_equal(out["mean_pred"], ref[0][:, 0]) and np.array_equal(out["group_var"], ref[3]) and out["n_failed"] == 0


def test_groups_of_one_are_vecchia_krige():
    """every g = 1 group agrees with vecchia_krige at the same location within 2e-8 (both are held to 1e-8), and fails with it"""
    G, c = _G(), _case()
    rng = np.random.default_rng(9)
    q = rng.random((60, 2))
    q[:3] = c["locs"][[5, 900, 4000]]                                # on observations
    q[3] = [1.3, -0.2]
    lab = np.arange(60)
    Z = c["Z"][:, :3]
    for m in (1, 15, 30, 63):
        NN = KT.query_nn(c["locs"], q, m)
        _, _, l1, _ = KT.krige_ld(c["locs"], TAU, Z, q, NN, *MATERN15[:1], list(MATERN15[1]))
        a = G.vecchia_krige(Z, c["va"], q, list(MATERN15[1]), TAU, m=m)
        b = G.vecchia_krige_groups(Z, c["va"], q, lab, list(MATERN15[1]), TAU, m=m, return_cov=True)
        em = (np.abs(a["mean_pred"] - b["mean_pred"]).max(axis=1) / (l1 * np.abs(Z).max())).max()
        ev = (np.abs(a["var_pred"] - b["var_pred"]) / a["var_pred"]).max()
        print(f"g = 1 against vecchia_krige, m={m}: mean {em:.3g}, var {ev:.3g}")
        assert em <= 2 * BAR and ev <= 2 * BAR and a["n_failed"] == b["n_failed"] == 0
        assert np.array_equal(b["group_mean"], b["mean_pred"]) and np.array_equal(b["group_var"], b["var_pred"])
        assert all(S.shape == (1, 1) and S[0, 0] == v for S, v in zip(b["group_cov"], b["var_pred"]))
    # a location on an observation without a nugget: that group fails alone, as the location does
    tau = np.full(N, TAU)
    tau[900] = 0.0
    a = G.vecchia_krige(Z, c["va"], q, list(MATERN15[1]), tau, m=30)
    b = G.vecchia_krige_groups(Z, c["va"], q, lab, list(MATERN15[1]), tau, m=30, return_cov=True)
    assert a["n_failed"] == b["n_failed"] == 1
    for key in ("mean_pred", "var_pred"):
        assert np.array_equal(np.isnan(a[key]), np.isnan(b[key])) and np.isnan(b[key][1]).all()
    assert np.isnan(b["group_mean"][1]).all() and np.isnan(b["group_var"][1]) and np.isnan(b["group_cov"][1]).all()
    assert np.isfinite(np.delete(b["group_var"], 1)).all()
    # inside a larger group the failure takes the whole group and nothing else
    lab2 = np.arange(60) // 4
    q2 = q.copy()
    q2[[0, 2, 3]] = q[1] + [[0.004, 0.0], [0.0, -0.005], [-0.003, 0.003]]        # (observation 900 is among the 30 of the anchor)
    d = G.vecchia_krige_groups(Z, c["va"], q2, lab2, list(MATERN15[1]), tau, m=30)
    assert d["n_failed"] == 1 and np.isnan(d["mean_pred"][:4]).all() and np.isnan(d["var_pred"][:4]).all()
    assert np.isfinite(d["mean_pred"][4:]).all() and np.isnan(d["group_var"][0]) and np.isfinite(d["group_var"][1:]).all()


def test_m_equal_n_is_the_dense_conditional():
    G = _G()
    rng = np.random.default_rng(21)
    n, g = 40, 24
    locs, xg = rng.random((n, 2)), 0.4 + 0.2 * rng.random((g, 2))
    Z = rng.standard_normal((n, 3))
    tau = 0.05 + 0.1 * rng.random(n)
    covmodel, cp = "matern", [1.3, 0.25, 1.5]
    va = G.vecchia_specify(locs, 10, cond_yz="z")
    out = G.vecchia_krige_groups(Z, va, xg, np.zeros(g, dtype=int), cp, tau, m=n, return_cov=True)
    Cm = KT.cov_matrix(np.vstack([locs, xg]).astype(np.longdouble), covmodel, cp)
    K, k = Cm[:n, :n] + np.diag(tau), Cm[:n, n:]
    t = GT.krige_groups_ld(locs, tau, Z, xg, np.array([0, g]), np.arange(1, n + 1, dtype=np.int32)[None, :], covmodel, cp)[0]
    sol = np.linalg.solve(np.asarray(K, dtype=np.float64), np.asarray(np.hstack([Z, k]), dtype=np.float64))
    dense_mean, dense_cov = np.asarray(k, dtype=np.float64).T @ sol[:, :3], np.asarray(Cm[n:, n:], dtype=np.float64) - np.asarray(k, dtype=np.float64).T @ sol[:, 3:]
    assert np.abs(t["mean"] - dense_mean).max() <= 1e-9 * np.abs(Z).max() and np.abs(t["cov"] - dense_cov).max() <= 1e-9 * cp[0]
    s = GT.scales(t, np.full(g, 1.0 / g), np.abs(Z).max())
    em = (np.abs(out["mean_pred"] - t["mean"]) / s["mean"]).max()
    ec = (np.abs(out["group_cov"][0] - t["cov"]) / s["cov"]).max()
    print(f"m = n = 40, g = 24 against the dense conditional: mean {em:.3g}, cov {ec:.3g}")
    assert out["n_failed"] == 0 and em <= BAR and ec <= BAR


def test_chunking_neighbours_and_columns_change_no_bit():
    c = _case()
    plan, Zord, _ = _ordered(c)
    covmodel, cp = MATERN15
    for m in (1, 15, 30):
        q, gptr = _layout(m)
        a = plan.krige_groups(covmodel, cp, TAU, q, gptr, m, Z_ord=Zord, want_cov=True)
        b = plan.krige_groups(covmodel, cp, TAU, q, gptr, m, Z_ord=Zord, want_cov=True, chunk=7)
        assert a[5] == 0 and b[5] == 0
        assert all(np.array_equal(x, y) for x, y in zip(a[:5], b[:5]))
        # a group alone against the same group inside the mixed call: one of every size
        sizes = np.diff(gptr)
        for k in [int(np.nonzero(sizes == s)[0][-1]) for s in np.unique(sizes)]:
            s0, s1 = gptr[k], gptr[k + 1]
            one = plan.krige_groups(covmodel, cp, TAU, q[s0:s1], [0, s1 - s0], m, Z_ord=Zord, want_cov=True)
            at = int(sum(s * (s + 1) // 2 for s in sizes[:k]))
            assert np.array_equal(one[0], a[0][s0:s1]) and np.array_equal(one[1], a[1][s0:s1])
            assert np.array_equal(one[2][0], a[2][k]) and one[3][0] == a[3][k]
            assert np.array_equal(one[4], a[4][at:at + one[4].size])
        # column 2 of 16 against a one-column call, and without the covariances
        col = plan.krige_groups(covmodel, cp, TAU, q, gptr, m, Z_ord=Zord[:, 2], chunk=11)
        assert np.array_equal(col[0][:, 0], a[0][:, 2]) and np.array_equal(col[2][:, 0], a[2][:, 2])
        assert np.array_equal(col[1], a[1]) and np.array_equal(col[3], a[3]) and col[4] is None


def test_given_neighbours_and_the_plans_own_data():
    from gpvecchia_amd import specify as S
    c = _case()
    plan, Zord, _ = _ordered(c)
    covmodel, cp = MATERN15
    q, gptr = _layout(15)
    a = plan.krige_groups(covmodel, cp, TAU, q, gptr, 15, Z_ord=Zord[:, 2], want_cov=True)
    NNg = S.find_query_nn_gpu(c["va"]["locsord"], GT.anchors(q, gptr), 15)
    b = plan.krige_groups(covmodel, cp, TAU, q, gptr, 15, Z_ord=Zord[:, 2], NNg=NNg, want_cov=True)
    plan.set_data(Zord[:, 2])
    d = plan.krige_groups(covmodel, cp, TAU, q, gptr, 15, want_cov=True)
    for x in (b, d):
        assert all(np.array_equal(u, v) for u, v in zip(x[:5], a[:5])) and x[5] == 0
    # the device's search is the definition's, at the anchors
    o = c["va"]["ord_z"] - 1
    assert (o[NNg - 1] + 1 == GT.group_nn(c["locs"], q, gptr, 15)).all()


def _raw(plan, q, gptr, m, weights=None, NNg=None, n=N, R=2):
    """the C entry on sentinel-filled outputs: (status, [mean, var, gmean, gvar, cov], n_failed)"""
    from gpvecchia_amd import _lib as L
    q = np.asfortranarray(q)
    nq, ng = q.shape[0], len(gptr) - 1
    gp = np.ascontiguousarray(gptr, dtype=np.int64)
    cp, nug = np.array(MATERN15[1]), np.array([TAU])
    Z = np.zeros((n, R), order="F")
    outs = [np.full((nq, R), -77.0, order="F"), np.full(nq, -77.0), np.full((ng, R), -77.0, order="F"), np.full(ng, -77.0),
            np.full(max(int(sum(max(g, 0) * (max(g, 0) + 1) // 2 for g in np.diff(gp))), 1), -77.0)]
    nf = C.c_int64(-77)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    nn = None if NNg is None else np.asfortranarray(NNg, dtype=np.int32)
    st = L.lib().gpv_plan_krige_groups(plan._h, b"matern", L.dptr(cp), 3, L.dptr(nug), 1, L.dptr(Z), n, R, L.dptr(q), nq,
                                       gp.ctypes.data_as(C.POINTER(C.c_int64)), ng, None if w is None else L.dptr(w), m,
                                       None if nn is None else L.iptr(nn), None, None, 0, L.dptr(outs[0]), nq, L.dptr(outs[1]),
                                       L.dptr(outs[2]), ng, L.dptr(outs[3]), L.dptr(outs[4]), C.byref(nf))
    return st, outs, nf.value


def _untouched(outs, nf):
    return all((x == -77.0).all() for x in outs) and nf == -77


def test_refusals_write_nothing():
    G, c = _G(), _case()
    from gpvecchia_amd import api
    plan, _, _ = _ordered(c)
    rng = np.random.default_rng(4)
    q = rng.random((70, 2))
    ok = [0, 3, 10, 40, 70]
    NNg = np.tile(np.arange(1, 6, dtype=np.int32), (4, 1))
    w_bad = np.ones(70)
    w_bad[44] = np.nan
    w_inf = np.ones(70)
    w_inf[0] = -np.inf
    bad_nn_hi, bad_nn_lo = NNg.copy(), NNg.copy()
    bad_nn_hi[1, 2], bad_nn_lo[2, 4] = N + 1, -1
    for kw, want in ((dict(gptr=[0, 5, 70], m=1), GPV_ERR_UNSUPPORTED_M),            # m + g = 66
                     (dict(gptr=[0, 6, 70], m=1), GPV_ERR_UNSUPPORTED_M),            # m + g = 65
                     (dict(gptr=[0, 35, 70], m=30), GPV_ERR_UNSUPPORTED_M),          # 30 + 35 = 65
                     (dict(gptr=ok, m=64), GPV_ERR_UNSUPPORTED_M),
                     (dict(gptr=[0, 3, 3, 40, 70], m=5), GPV_ERR_BAD_ARG),           # an empty group
                     (dict(gptr=[0, 10, 3, 40, 70], m=5), GPV_ERR_BAD_ARG),          # not non-decreasing
                     (dict(gptr=[1, 3, 10, 40, 70], m=5), GPV_ERR_BAD_ARG),
                     (dict(gptr=[0, 3, 10, 40, 69], m=5), GPV_ERR_BAD_ARG),
                     (dict(gptr=ok, m=5, weights=w_bad), GPV_ERR_BAD_ARG),
                     (dict(gptr=ok, m=5, weights=w_inf), GPV_ERR_BAD_ARG),
                     (dict(gptr=ok, m=5, NNg=bad_nn_hi), GPV_ERR_INDEX),
                     (dict(gptr=ok, m=5, NNg=bad_nn_lo), GPV_ERR_INDEX)):
        st, outs, nf = _raw(plan, q, **kw)
        assert st == want and _untouched(outs, nf), (kw, st)
    st, outs, nf = _raw(plan, q, [0, 7, 70], 1)                                     # m + g = 64 is served
    assert st == 0 and nf == 0 and all(np.isfinite(x).all() for x in outs)
    st, outs, nf = _raw(plan, q[:0], [0], 5)                                        # no group: nothing to do
    assert st == 0 and nf == 0
    # a 'zy' plan (latent conditioning), a plan with unobserved locations, a row shard
    va = c["va"]
    prep = va["U_prep"]
    zy = G.vecchia_specify(c["locs"][:500], 10, cond_yz="zy", locs_pred=rng.random((20, 2)))
    unobs = api.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
    obs = np.ones(N, dtype=bool)
    obs[5] = False
    unobs.set_observed(obs)
    shard = api.Plan(va["locsord"], prep["revNNarray"], prep["revCond"], row_begin=0, row_end=N // 2)
    zy_plan = api._plan_for(zy)
    for pl, n in ((zy_plan, zy_plan.Nlocs), (unobs, N), (shard, N)):
        st, outs, nf = _raw(pl, q, ok, 5, n=n)
        assert st == GPV_ERR_STATE and _untouched(outs, nf)
    with pytest.raises(ValueError):
        G.vecchia_krige_groups(np.zeros(500), zy, q, np.zeros(70, dtype=int), list(MATERN15[1]), TAU)
    with pytest.raises(G.GpvError) as e:
        plan.krige_groups(*MATERN15, TAU, q, [0, 35, 70], 30, Z_ord=c["Z"][:, 0])
    assert e.value.status == GPV_ERR_UNSUPPORTED_M


def test_predict_z_and_shuffled_labels():
    """predict='z' adds the nuggets on the host; labels in any order: everything comes back in the caller's order"""
    G, c = _G(), _case()
    q, gptr = _layout(15)
    cp = list(MATERN15[1])
    lab = np.repeat(np.arange(len(gptr) - 1), np.diff(gptr)) * 3 - 40      # any integers
    rng = np.random.default_rng(6)
    w = 0.1 + rng.random(gptr[-1])
    Z = c["Z"][:, :3]
    base = G.vecchia_krige_groups(Z, c["va"], q, lab, cp, TAU, m=15, weights=w, return_cov=True)
    perm = rng.permutation(gptr[-1])
    shuf = G.vecchia_krige_groups(Z, c["va"], q[perm], lab[perm], cp, TAU, m=15, weights=w[perm], return_cov=True)
    assert np.array_equal(shuf["group_ids"], base["group_ids"]) and np.array_equal(base["group_ids"], np.unique(lab))
    # (the members of a group enter in another order: another, equally valid, elimination order -> the bar, not bits)
    plan_truth = GT.krige_groups_ld(c["locs"], TAU, Z, q, gptr, GT.group_nn(c["locs"], q, gptr, 15), "matern", cp)
    zmax = np.abs(Z).max()
    l1 = np.concatenate([t["l1"] for t in plan_truth])
    sd = np.sqrt(base["var_pred"])
    assert (np.abs(shuf["mean_pred"] - base["mean_pred"][perm]).max(axis=1) <= 2 * BAR * l1[perm] * zmax).all()
    assert (np.abs(shuf["var_pred"] - base["var_pred"][perm]) <= 2 * BAR * base["var_pred"][perm]).all()
    for k in range(len(gptr) - 1):
        idx = np.arange(gptr[k], gptr[k + 1])
        pos = np.nonzero(np.isin(perm, idx))[0]                      # where the group's members went, in the caller's order
        mem = perm[pos] - gptr[k]
        assert (np.abs(shuf["group_cov"][k] - base["group_cov"][k][np.ix_(mem, mem)]) <= 2 * BAR * np.outer(sd[idx][mem], sd[idx][mem])).all()
        assert np.abs(shuf["group_var"][k] - base["group_var"][k]) <= 2 * BAR * (np.abs(w[idx]) @ sd[idx]) ** 2
    # predict = 'z'
    taup = 0.02 + 0.1 * rng.random(gptr[-1])
    zed = G.vecchia_krige_groups(Z, c["va"], q, lab, cp, TAU, m=15, weights=w, return_cov=True, predict="z", nugget_pred=taup)
    assert np.array_equal(zed["mean_pred"], base["mean_pred"]) and np.array_equal(zed["group_mean"], base["group_mean"])
    assert np.array_equal(zed["var_pred"], base["var_pred"] + taup)
    for k in range(len(gptr) - 1):
        a, b = gptr[k], gptr[k + 1]
        assert np.allclose(zed["group_var"][k], base["group_var"][k] + (w[a:b] ** 2) @ taup[a:b], rtol=1e-14, atol=0)
        assert np.array_equal(zed["group_cov"][k], base["group_cov"][k] + np.diag(taup[a:b]))
    one = G.vecchia_krige_groups(Z[:, 0], c["va"], q, lab, cp, TAU, m=15, weights=w, mean=0.5, mean_pred=0.5)
    assert one["mean_pred"].shape == (gptr[-1],) and one["group_mean"].shape == (len(gptr) - 1,)


def test_vecchia_pred_groups_adds_the_trend_back():
    G = _G()
    rng = np.random.default_rng(8)
    n, m = 400, 10
    locs = rng.random((n, 2))
    Sigma = KT.cov_matrix(locs, "matern", [1.0, 0.1, 1.5]) + 0.05 * np.eye(n)
    data = 3.0 + np.linalg.cholesky(Sigma) @ rng.standard_normal(n)
    est = G.vecchia_estimate(data, locs, m=m, output_level=0, maxit=40, cond_yz="z")
    centre = rng.random((12, 2))
    q = np.repeat(centre, 4, axis=0) + 0.04 * (rng.random((48, 2)) - 0.5)
    lab = np.repeat(np.arange(12), 4)
    gptr = np.arange(0, 49, 4)
    pred = G.vecchia_pred(est, q, m=m, local=True, groups=lab, return_cov=True)
    th = np.asarray(est["theta_hat"])
    truth = GT.krige_groups_ld(locs, th[-1], est["z"], q, gptr, GT.group_nn(locs, q, gptr, m), "matern", list(th[:-1]))
    b0 = est["beta_hat"][0]
    w = np.full(48, 0.25)
    e = _errors(pred["mean_pred"][:, None] - b0, pred["var_pred"], pred["group_mean"][:, None] - b0, pred["group_var"], None, truth,
                gptr, w, np.abs(est["z"]).max())
    print("vecchia_pred(local=True, groups=): " + ", ".join(f"{k} {v:.3g}" for k, v in e.items()))
    assert est["trend"] == "constant" and pred["n_failed"] == 0 and all(v <= BAR for v in e.values())
    assert len(pred["group_cov"]) == 12 and np.array_equal(pred["group_ids"], np.arange(12))
    con = G.vecchia_pred(est, q, m=m, local=True, groups=lab, weights=np.tile([1.0, -1.0, 0.0, 0.0], 12))
    want = np.array([t["mean"][0, 0] - t["mean"][1, 0] for t in truth])          # a contrast: the constant cancels
    assert np.abs(con["group_mean"] - want).max() <= 1e-8 * max(t["l1"][:2].sum() for t in truth) * np.abs(est["z"]).max() + 1e-12 * abs(b0)
    plain = G.vecchia_pred(est, q, m=m, local=True)                              # without groups: the call it was
    assert set(plain) == {"mean_pred", "var_pred"}
