"""GPU parity tests on BASELINE.json's five configurations: every config runs through the HIP path
(C ABI of libgpvecchia_hip.so) and is compared with the oracle — on all rows where the oracle finishes in seconds,
on sampled rows plus size-independent properties at the full sizes.

  C1  n=5000 = 100x50 regular grid, maxmin ordering (+ the cut=9 quirk), m=10   (grid ties everywhere)
  C2  n=1e5 2-D uniform, Matern 1.5, m=20                                       (all rows vs the oracle)
  C3  n=1e6 2-D, m=30: tests/test_gpu_parity.py::test_full_size_properties_n1e6_m30
  C4  n=1e6 3-D, exponential (Matern nu=0.5), m=60: instantiation gpv_sets_kernel<61,3,COV_MATERN05>
  C5  n=5e5 2-D, Vecchia-Laplace Poisson likelihood, m=30

Tolerances as in test_gpu_parity.py: index arrays bit-exact, U entries 1e-8 normwise per row, log-likelihood 1e-8
relative (1e-7 for the Vecchia-Laplace quantities, which sit behind a Newton iteration stopped at 1e-6)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROW_TOL = 1e-8
LL_RTOL = 1e-8


def _need_gpu():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


def _row_err(A, B):
    scale = np.maximum(np.abs(B).max(axis=1), 1e-300)
    return (np.abs(A - B).max(axis=1) / scale).max()


def _to_oracle_va(va):
    """product vecchia.approx (0 / -1 = NA) -> oracle representation (NaN = NA)."""
    prep = dict(va["U_prep"])
    nn = prep["revNNarray"]
    prep["revNNarray"] = np.where(nn == 0, np.nan, nn.astype(np.float64))
    prep["revCond"] = np.where(prep["revCond"] < 0, np.nan, prep["revCond"].astype(np.float64))
    out = {k: v for k, v in va.items() if not isinstance(k, tuple)}
    out["U_prep"] = prep
    return out


def _oracle_rows(R, locs, revNN, revCond, rows, tau, covmodel, cp):
    """U_NZentries of the oracle on a subset of conditioning sets (sub-problem with remapped indices)."""
    n, p = revNN.shape
    sub = revNN[rows]
    used = np.unique(sub[sub != 0]) - 1
    remap = np.zeros(n + 1, dtype=np.int64)
    remap[used + 1] = np.arange(1, used.size + 1)
    Nl = max(used.size, len(rows))
    nnp = np.zeros((Nl, p), dtype=np.int64); nnp[: len(rows)] = remap[sub]
    cdp = np.zeros((Nl, p)); cdp[: len(rows)] = np.where(revCond[rows] < 0, 0, revCond[rows])
    lp = np.zeros((Nl, locs.shape[1])); lp[: used.size] = locs[used]
    tv = np.full(Nl, tau) if np.ndim(tau) == 0 else None
    if tv is None:
        tv = np.ones(Nl); tv[: used.size] = np.asarray(tau)[used]
    ref = R.U_NZentries(R.max_threads(), 1, lp, nnp, cdp, tv, tv[:1], covmodel, cp)
    return ref["Lentries"][: len(rows)], ref["n_failed"]


# ----------------------------------------------------------------------------------------------------------------
# C1: 100 x 50 grid, maxmin, m = 10
# ----------------------------------------------------------------------------------------------------------------
def test_C1_grid_maxmin_m10():
    G = _need_gpu()
    from oracle import r_side as R
    gx, gy = np.meshgrid((np.arange(100) + 0.5) / 100, (np.arange(50) + 0.5) / 50, indexing="ij")
    locs = np.stack([gx.ravel(), gy.ravel()], axis=1)
    n, m = locs.shape[0], 10
    assert n == 5000
    z = np.random.default_rng(1).standard_normal(n)
    cp, tau = [1.0, 0.1, 1.5], 0.1
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="SGV", nn_backend="gpu")
    # (a) the ordering is a max-min ordering in the sense of src/MaxMin.cpp:661-738 once the cut = 9 shuffle of
    # R/vecchia_specify.R:105-106 is undone: point t is (one of) the farthest from the points before it.  Grid ties make
    # the order itself non-unique (the reference's is an artefact of its heap), so the DEFINITION is checked.
    ord_ = va["ord"]
    assert np.array_equal(np.sort(ord_), np.arange(1, n + 1))
    cut = 9
    o = np.concatenate([ord_[:1], ord_[n - (cut - 1):], ord_[1: n - (cut - 1)]]) - 1
    avg = locs.mean(axis=0)
    d0 = ((locs - avg) ** 2).sum(axis=1)
    assert d0[o[0]] <= d0.min() * (1 + 1e-12)                        # grid: 4 points tie for 'closest to the centroid'
    mind = np.sqrt(((locs - locs[o[0]]) ** 2).sum(axis=1))
    mind[o[0]] = -1.0
    for t in range(1, n):
        assert mind[o[t]] >= mind.max() * (1 - 1e-12), t               # ties up to rounding of (i + .5)/100 differences
        np.minimum(mind, np.sqrt(((locs - locs[o[t]]) ** 2).sum(axis=1)), out=mind)
        mind[o[:t + 1]] = -1.0
    # ... and it is the oracle's ordering (O(n^2) definition, lowest index wins ties) element for element
    assert np.array_equal(R.order_maxmin_exact(locs), o + 1)
    # (b) neighbour arrays on the product's locsord: bit-exact against the oracle's findOrderedNN (lower index wins
    # ties, R/NN_kdtree.R:79-80) and, independently of any tie rule, equal as distance multisets
    locsord = va["locsord"]
    assert np.array_equal(locsord, locs[ord_ - 1])
    NN = va["U_prep"]["revNNarray"][:, ::-1]
    NNo = np.nan_to_num(R.findOrderedNN(locsord, m)).astype(np.int32)
    assert np.array_equal(NN, NNo)
    for k in (0, 1, 5, 10, 11, 100, 2500, n - 1):
        d = np.sort(np.sqrt(((locsord[: k + 1] - locsord[k]) ** 2).sum(axis=1)))[: m + 1]
        idx = NN[k][NN[k] != 0] - 1
        assert np.array_equal(np.sort(np.sqrt(((locsord[idx] - locsord[k]) ** 2).sum(axis=1))), d)
    # (c) SGV cond flags: the native whichCondOnLatent against the literal R/whichCondOnLatent.R:2-26
    Co = R.whichCondOnLatent(np.where(NNo == 0, np.nan, NNo.astype(float)))
    assert np.array_equal(va["U_prep"]["revCond"][:, ::-1], np.nan_to_num(Co, nan=-1).astype(np.int8))
    # (d) U entries of all 5000 rows and the log-likelihood, cond.yz = 'SGV' and 'z'
    for cond in ("SGV", "z"):
        if cond == "z":
            va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="z", nn_backend="gpu")
        ova = _to_oracle_va(va)
        refU = R.createU(ova, cp, tau)
        U = G.createU(va, cp, tau)
        assert refU["U_entries"]["n_failed"] == 0
        assert _row_err(U["Lentries"], refU["U_entries"]["Lentries"]) < ROW_TOL
        np.testing.assert_array_equal(U["Lentries"] == 0, refU["U_entries"]["Lentries"] == 0)
        np.testing.assert_allclose(U["Zentries"], refU["U_entries"]["Zentries"], rtol=1e-15)
        ll_ref = R.vecchia_likelihood_U(z, refU)
        ll = G.vecchia_likelihood(z, va, cp, tau)
        assert abs(ll - ll_ref) <= LL_RTOL * abs(ll_ref), (cond, ll, ll_ref)
        if cond == "z":
            ll_sep, _ = R.separable_loglik_condz(ova, refU["U_entries"], z, tau)
            assert abs(ll - ll_sep) <= LL_RTOL * abs(ll_sep)
        del refU


# ----------------------------------------------------------------------------------------------------------------
# C2: n = 1e5, m = 20, every row against the oracle
# ----------------------------------------------------------------------------------------------------------------
def test_C2_full_size_all_rows_n1e5_m20():
    G = _need_gpu()
    from gpvecchia_amd import specify as S
    from oracle import r_side as R
    n, m, p = 100_000, 20, 21
    locs = np.random.default_rng(0).random((n, 2))
    z = np.random.default_rng(1).standard_normal(n)
    cp, tau = [1.0, 0.05, 1.5], 0.1
    NN = S.find_ordered_nn_gpu(locs, m)
    assert np.array_equal(NN, S.find_ordered_nn(locs, m))              # GPU brute force == host cKDTree search, bit-exact
    revNN = NN[:, ::-1].copy()
    for cond in ("z", "SGV"):
        if cond == "z":
            revCond = np.where(revNN != 0, 0, -1).astype(np.int8)
            revCond[:, -1] = 1
        else:
            revCond = S.whichCondOnLatent(NN)[:, ::-1].copy()
        ref = R.U_NZentries(R.max_threads(), n, locs, revNN, np.where(revCond < 0, 0, revCond).astype(float),
                            np.full(n, tau), np.full(n, tau), "matern", cp)
        out = G.U_NZentries(1, n, locs, revNN, revCond, np.full(n, tau), np.full(n, tau), "matern", cp)
        assert out["n_failed"] == ref["n_failed"] == 0
        # ALL 1e5 rows.  cond.yz='z': flat 1e-8.  SGV: neighbours conditioned on as latent carry no nugget, and at this
        # density (spacing 0.003 against a range of 0.05) a few blocks reach cond(S) ~ 1e7..1e8, where two correct fp64
        # factorisations differ by cond*eps: those rows are adjudicated in extended precision
        from _parity import check_rows
        res = check_rows(out["Lentries"], ref["Lentries"], locs, revNN, revCond, tau, "matern", cp, label=f"C2 all rows {cond}")
        if cond == "z":
            assert res["escaped"] == 0 and res["max_err"] < ROW_TOL, res
        else:
            # every row beyond the flat bound has been measured against the extended-precision row (tests/_parity.py);
            # there must be few of them, and very few where the kernel's error exceeds 4x the oracle's own
            assert res["escaped"] <= n // 1000 and res["beyond4x"] <= max(5, res["escaped"] // 2) and res["sum_ratio"] <= 3.0, res
            err = np.abs(out["Lentries"] - ref["Lentries"]).max(axis=1) / np.abs(ref["Lentries"]).max(axis=1)
            assert np.median(err) < 1e-11
        np.testing.assert_array_equal(out["Lentries"] == 0, ref["Lentries"] == 0)
        np.testing.assert_allclose(out["Zentries"], ref["Zentries"], rtol=1e-15)
        if cond == "z":
            va = dict(U_prep=dict(revNNarray=np.where(revNN == 0, np.nan, revNN.astype(float)),
                                  revCond=np.where(revCond < 0, np.nan, revCond.astype(float))),
                      ord_z=np.arange(1, n + 1))
            ll_ref, s_ref = R.separable_loglik_condz(va, ref, z, tau)
            plan = G.Plan(locs, revNN, revCond)
            plan.set_data(z)
            plan.eval("matern", cp, tau, G.GPV_WANT_LOGLIK_Z | G.GPV_WANT_NUMERATOR)
            s = plan.sums()
            ll = G.loglik_z_from_sums(s, n)
            assert abs(ll - ll_ref) <= LL_RTOL * abs(ll_ref)
            np.testing.assert_allclose(s[0], s_ref[0], rtol=1e-10)
            np.testing.assert_allclose(s[1], s_ref[3], rtol=1e-9)
        else:
            # default mode at full size: the device posterior pass against the sparse host factorisation of the same U
            va = dict(locsord=locs, obs=np.ones(n, bool), ord=np.arange(1, n + 1), ord_z=np.arange(1, n + 1),
                      ord_pred="general", cond_yz="SGV", ic0=False, conditioning="NN",
                      U_prep=S.U_sparsity(locs, NN, np.ones(n, bool), S.whichCondOnLatent(NN)))
            ll = G.vecchia_likelihood(z, va, cp, tau)
            assert va[("_plan", 0)].has_posterior
            ll_host = G.vecchia_likelihood_U(z, G.createU(va, cp, tau))
            assert abs(ll - ll_host) <= 1e-9 * abs(ll_host)


# ----------------------------------------------------------------------------------------------------------------
# C4: 3-D, exponential covariance, m = 60
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cond", ["z", "SGV", "y"])
def test_C4_instantiation_m60_3d_exponential(cond):
    # gpv_sets_kernel<61, 3, COV_MATERN05> against the oracle on every row (n small enough for the dense oracle)
    G = _need_gpu()
    from oracle import r_side as R
    n, m = 700, 60
    rng = np.random.default_rng(160)
    locs = rng.random((n, 3))
    z = rng.standard_normal(n)
    va = R.vecchia_specify(locs, m, ordering="none", cond_yz=cond)
    cp, tau = [1.0, 0.05, 0.5], 0.1                                    # BASELINE config 4's parameters
    refU = R.createU(va, cp, tau)
    prep = va["U_prep"]
    out = G.U_NZentries(1, n, va["locsord"], prep["revNNarray"], prep["revCond"], np.full(n, tau), np.full(n, tau),
                        "matern", cp)
    assert out["n_failed"] == refU["U_entries"]["n_failed"] == 0
    assert _row_err(out["Lentries"], refU["U_entries"]["Lentries"]) < ROW_TOL
    np.testing.assert_array_equal(out["Lentries"] == 0, refU["U_entries"]["Lentries"] == 0)
    np.testing.assert_allclose(out["Zentries"], refU["U_entries"]["Zentries"], rtol=1e-15)
    pva = dict(va)
    pp = dict(prep)
    pp["revNNarray"] = np.nan_to_num(prep["revNNarray"]).astype(np.int32)
    pp["revCond"] = np.nan_to_num(prep["revCond"], nan=-1.0).astype(np.int8)
    pva["U_prep"] = pp
    ll_ref = R.vecchia_likelihood_U(z, refU)
    ll = G.vecchia_likelihood(z, pva, cp, tau)
    assert abs(ll - ll_ref) <= LL_RTOL * abs(ll_ref)
    # a longer range (the exponential kernel stays well conditioned) and vector nuggets through the same instantiation
    cp2, tau2 = [2.5, 0.4, 0.5], 0.05 + rng.random(n)
    ref2 = R.createU(va, cp2, tau2)
    out2 = G.U_NZentries(1, n, va["locsord"], prep["revNNarray"], prep["revCond"], tau2, tau2, "matern", cp2)
    assert _row_err(out2["Lentries"], ref2["U_entries"]["Lentries"]) < ROW_TOL
    ll_ref2 = R.vecchia_likelihood_U(z, ref2)
    assert abs(G.vecchia_likelihood(z, pva, cp2, tau2) - ll_ref2) <= LL_RTOL * abs(ll_ref2)


def test_C4_full_size_properties_n1e6_m60_3d():
    """BASELINE config 4 at full size: sampled neighbour rows vs the definition, ALL conditioning sets vs the oracle,
    fused sums vs a host recomputation from the U entries in HBM, shard additivity, bitwise reproducibility."""
    G = _need_gpu()
    from gpvecchia_amd import specify as S
    from oracle import r_side as R
    n, m, p = 1_000_000, 60, 61
    rng = np.random.default_rng(0)
    locs = rng.random((n, 3))
    z = np.random.default_rng(1).standard_normal(n)
    NN = S.find_ordered_nn_gpu(locs, m)
    for k in np.concatenate([[0, 1, 59, 60, 61, 200], rng.integers(1000, n, 25)]):
        d = np.sqrt((locs[: k + 1, 0] - locs[k, 0]) ** 2 + (locs[: k + 1, 1] - locs[k, 1]) ** 2
                    + (locs[: k + 1, 2] - locs[k, 2]) ** 2)             # left-to-right accumulation, src/dist.cpp:12-14
        o = np.lexsort((np.arange(k + 1), d))[: min(p, k + 1)] + 1
        assert np.array_equal(NN[k, : len(o)], o) and not NN[k, len(o):].any()
    revNN = NN[:, ::-1].copy()
    del NN
    revCond = np.where(revNN != 0, 0, -1).astype(np.int8)
    revCond[:, -1] = 1
    cp, tau = [1.0, 0.05, 0.5], 0.1
    plan = G.Plan(locs, revNN, revCond)
    plan.set_data(z)
    plan.eval("matern", cp, tau, G.GPV_WANT_LOGLIK_Z | G.GPV_WANT_NUMERATOR | G.GPV_WANT_U)
    s = plan.sums()
    assert s[6] == 0 and s[7] == n
    Lent = plan.Lentries()
    # ALL 1e6 conditioning sets against the oracle (488 MB of U entries a side; ~6 s of oracle time on the box's cores)
    from _parity import check_rows
    ref = R.U_NZentries(R.max_threads(), n, locs, revNN, np.where(revCond < 0, 0, revCond).astype(np.float64),
                        np.full(n, tau), np.full(n, tau), "matern", cp)
    assert ref["n_failed"] == 0
    res = check_rows(Lent, ref["Lentries"], locs, revNN, revCond, tau, "matern", cp, label="C4 full size, all rows")
    assert res["rows"] == n and res["escaped"] == 0 and res["max_err"] < ROW_TOL, res
    ll_ref, s_ref = R.separable_sums_condz_vectorised(revNN, ref["Lentries"], z, tau)
    assert abs(G.loglik_z_from_sums(s, n) - ll_ref) <= LL_RTOL * abs(ll_ref)
    del ref
    # fused sums vs host recomputation (cond.yz='z': every neighbour is observed-conditioned)
    n0 = (revNN != 0).sum(axis=1)
    dk = Lent[np.arange(n), n0 - 1]
    v = 1.0 / dk ** 2
    ak = np.zeros(n)
    full = n0 == p
    nb = revNN[:, :-1]
    CH = 100_000
    for a0 in range(0, n, CH):                                         # chunks bound the temporaries (1e5 x 60 doubles)
        sl = slice(a0, min(n, a0 + CH))
        f = full[sl]
        idx = np.where(f[:, None], nb[sl] - 1, 0)
        ak[sl] = np.where(f, np.einsum("ij,ij->i", Lent[sl, : p - 1], z[idx]), 0.0)
    for k in np.where(~full)[0]:
        idx = revNN[k, p - n0[k]: p - 1] - 1
        ak[k] = Lent[k, : n0[k] - 1] @ z[idx]
    mu = -ak / dk
    np.testing.assert_allclose(s[0], np.log(dk).sum(), rtol=1e-11)
    np.testing.assert_allclose(s[1], (ak ** 2).sum(), rtol=1e-10)
    np.testing.assert_allclose(s[2], np.log(tau + v).sum(), rtol=1e-11)
    np.testing.assert_allclose(s[3], ((z - mu) ** 2 / (tau + v)).sum(), rtol=1e-10)
    del Lent
    plan.eval("matern", cp, tau, G.GPV_WANT_LOGLIK_Z)
    s2 = plan.sums()
    plan.eval("matern", cp, tau, G.GPV_WANT_LOGLIK_Z)
    assert np.array_equal(plan.sums(), s2)                              # bitwise
    np.testing.assert_allclose(s2[[2, 3]], s[[2, 3]], rtol=1e-13)
    del plan
    tot = np.zeros(8)
    for a, b in ((0, 250_001), (250_001, n)):
        sh = G.Plan(locs, revNN, revCond, row_begin=a, row_end=b)
        sh.set_data(z)
        sh.eval("matern", cp, tau, G.GPV_WANT_LOGLIK_Z)
        tot += sh.sums()
        del sh
    np.testing.assert_allclose(tot[[2, 3, 7]], s2[[2, 3, 7]], rtol=1e-12)


# ----------------------------------------------------------------------------------------------------------------
# C5: Vecchia-Laplace, Poisson, m = 30
# ----------------------------------------------------------------------------------------------------------------
def _smooth_field(locs):
    x, y = locs[:, 0], locs[:, 1]
    return 0.8 * np.sin(5.0 * x) * np.cos(4.0 * y) + 0.4 * np.cos(9.0 * (x + y)) + 0.3


def test_C5_vecchia_laplace_poisson_m30_vs_oracle():
    # R/vecchia_laplace_NR.R:88-130 at the conditioning-set size of BASELINE config 5 (one U_NZentries call with vector
    # pseudo-nuggets + U2V + vecchia_mean per Newton step): same iteration count, same posterior mean, same likelihood
    G = _need_gpu()
    from oracle import r_side as R
    rng = np.random.default_rng(530)
    n, m = 2000, 30
    locs = rng.random((n, 2))
    cp = [0.5, 0.03 * 5, 1.5]
    z = rng.poisson(np.exp(_smooth_field(locs))).astype(float)
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="SGV")
    vb = _to_oracle_va(va)
    post_ref = R.calculate_posterior_VL(z, vb, "poisson", cp)
    post = G.calculate_posterior_VL(z, va, "poisson", cp)
    assert post["cnvgd"] and post_ref["cnvgd"] and post["iter"] == post_ref["iter"]
    np.testing.assert_allclose(post["mean"], post_ref["mean"], rtol=0, atol=1e-7)
    ll_ref = R.vecchia_laplace_likelihood(z, vb, "poisson", cp)
    ll = G.vecchia_laplace_likelihood(z, va, "poisson", cp)
    assert abs(ll - ll_ref) <= 1e-7 * abs(ll_ref)


def test_C5_full_size_properties_n5e5_m30():
    """BASELINE config 5 at full size (n = 5e5, m = 30, Poisson data, maxmin + SGV): the Newton loop converges, is
    bitwise reproducible, satisfies its own fixed-point equation, and on a 6e4 subsample the device pass (set kernel +
    posterior pass + mean sweeps) equals the host sparse factorisation of the same U."""
    G = _need_gpu()
    from gpvecchia_amd import api as A
    n, m = 500_000, 30
    locs = np.random.default_rng(0).random((n, 2))
    cp = [0.5, 0.03, 1.5]
    z = np.random.default_rng(2).poisson(np.exp(_smooth_field(locs))).astype(float)
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="SGV", nn_backend="gpu")
    post = G.calculate_posterior_VL(z, va, "poisson", cp)
    assert post["cnvgd"] and 2 <= post["iter"] <= 30
    y = post["mean"]
    assert np.isfinite(y).all()
    # fixed point: one more Newton step from the converged mean moves it by less than the convergence threshold
    D = np.exp(-y)
    pseudo = D * (z - np.exp(y)) + y
    y2 = G.vecchia_prediction(pseudo, va, cp, D)["mu_obs"]
    assert np.max(np.abs(y2 - y)) < 1e-5
    post2 = G.calculate_posterior_VL(z, va, "poisson", cp)
    assert post2["iter"] == post["iter"] and np.array_equal(post2["mean"], y)      # bitwise
    ll = G.vecchia_laplace_likelihood(z, va, "poisson", cp)
    assert np.isfinite(ll)
    # the smooth field is recovered: posterior mean correlates with the truth
    assert np.corrcoef(y, _smooth_field(locs))[0, 1] > 0.8
    del va
    # device pass == host SuperLU path on a subsample (the reference's CHOLMOD route, R/vecchia_prediction.R:74-83)
    ns = 60_000
    ls, zs = locs[:ns], z[:ns]
    vs = G.vecchia_specify(ls, m, ordering="maxmin", cond_yz="SGV", nn_backend="gpu")
    ps = G.calculate_posterior_VL(zs, vs, "poisson", cp)
    assert ps["cnvgd"]
    Ds = ps["D"]
    pseudo_s = ps["t"]
    mu_dev = G.vecchia_prediction(pseudo_s, vs, cp, Ds)["mu_obs"]
    U_obj = A.createU(vs, cp, Ds)
    mu_ord = A.vecchia_mean_host(pseudo_s, U_obj)
    mu_host = np.empty(ns)
    mu_host[vs["ord"] - 1] = mu_ord
    np.testing.assert_allclose(mu_dev, mu_host, rtol=0, atol=1e-8 * max(1.0, np.abs(mu_host).max()))
    ll_dev = G.vecchia_likelihood(pseudo_s, vs, cp, Ds)
    ll_host = A.vecchia_likelihood_U(pseudo_s, U_obj)
    assert abs(ll_dev - ll_host) <= 1e-9 * abs(ll_host)


# ----------------------------------------------------------------------------------------------------------------
# C3 on the reference's DEFAULT ordering: maxmin (+ the cut-9 quirk), mode L — what bench.py reports as
# secondary.mode_L_maxmin (ordering='none' only "unless the maxmin builder exists")
# ----------------------------------------------------------------------------------------------------------------
def test_full_size_maxmin_mode_L_n1e6_m30():
    """n = 1e6, m = 30, ordering='maxmin', cond.yz='z': the ordering is a permutation with the reference's cut-9 rotation
    (R/vecchia_specify.R:103-106) and decreasing maxmin distances on a sample; neighbour rows equal the ordered-NN
    definition on sampled rows; ALL 1e6 conditioning sets equal the oracle's (flat 1e-8), and so does the log-likelihood."""
    G = _need_gpu()
    from oracle import r_side as R
    from _parity import check_rows
    n, m, p = 1_000_000, 30, 31
    rng = np.random.default_rng(0)
    locs = rng.random((n, 2))
    z = np.random.default_rng(1).standard_normal(n)
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="z", nn_backend="gpu")
    ord_ = va["ord"]
    assert np.array_equal(np.sort(ord_), np.arange(1, n + 1))
    lo = va["locsord"]
    assert np.array_equal(lo, locs[ord_ - 1])
    # maxmin property after undoing the rotation ord = c(o[1], o[-(1:9)], o[2:9]): position k (k >= 1, un-rotated) holds the
    # point farthest from the k points before it; spot-check the first positions exactly
    o = np.concatenate([ord_[:1], ord_[-8:], ord_[1:-8]])                 # the un-rotated maxmin order
    lm = locs[o - 1]
    for k in range(1, 12):
        dmin = np.sqrt(((locs[:, None, :] - lm[None, :k, :]) ** 2).sum(-1)).min(axis=1)
        assert abs(dmin[o[k] - 1] - dmin.max()) <= 1e-15
    revNN = va["U_prep"]["revNNarray"]
    NN = revNN[:, ::-1]
    for k in np.concatenate([[0, 1, 5, 30, 31, 100], rng.integers(1000, n, 30)]):
        dd = np.sqrt((lo[: k + 1, 0] - lo[k, 0]) ** 2 + (lo[: k + 1, 1] - lo[k, 1]) ** 2)
        want = np.lexsort((np.arange(k + 1), dd))[: min(p, k + 1)] + 1
        assert np.array_equal(NN[k, : len(want)], want) and not NN[k, len(want):].any()
    revCond = va["U_prep"]["revCond"]
    assert np.array_equal(revCond[:, -1], np.ones(n, revCond.dtype)) and not (revCond[:, :-1] > 0).any()
    cp, tau = [1.0, 0.02, 1.5], 0.1
    plan = G.Plan(lo, revNN, revCond)
    zord = z[va["ord_z"] - 1]
    plan.set_data(zord)
    plan.eval("matern", cp, tau, G.GPV_WANT_LOGLIK_Z | G.GPV_WANT_U)
    s = plan.sums()
    assert s[6] == 0 and s[7] == n
    Lent = plan.Lentries()
    ref = R.U_NZentries(R.max_threads(), n, lo, revNN, np.where(revCond < 0, 0, revCond).astype(np.float64),
                        np.full(n, tau), np.full(n, tau), "matern", cp)
    assert ref["n_failed"] == 0
    res = check_rows(Lent, ref["Lentries"], lo, revNN, revCond, tau, "matern", cp, label="C3 maxmin mode L, all rows")
    assert res["rows"] == n and res["escaped"] == 0 and res["max_err"] < ROW_TOL, res
    ll_ref, _ = R.separable_sums_condz_vectorised(revNN, ref["Lentries"], zord, tau)
    ll = G.loglik_z_from_sums(s, n)
    assert abs(ll - ll_ref) <= LL_RTOL * abs(ll_ref)
    assert abs(G.vecchia_likelihood(z, va, cp, tau) - ll_ref) <= LL_RTOL * abs(ll_ref)


# ----------------------------------------------------------------------------------------------------------------
# ordered nearest neighbours through the grid (round 4, csrc/gpv_nn.hip): bit-exact with the definition
# ----------------------------------------------------------------------------------------------------------------
def _nn_definition_rows(locs, m, rows):
    """The definition, row by row in NumPy: sqrt of the left-to-right sum of squared differences, ties -> lower index
    (tests/_nn_truth.py states it once for every test of the search)."""
    import _nn_truth
    return _nn_truth.nn_rows(locs, m, rows)


@pytest.mark.parametrize("case", ["uniform2d", "uniform3d", "line1d", "lattice_ties", "duplicates", "clustered", "flat_dimension",
                                  "thin_slab"])
def test_grid_nn_search_is_bit_exact(case):
    """Rows from 4096 on of problems in one to three dimensions take their candidates from a uniform grid
    (gpv_nn_grid_kernel) instead of all predecessors.  Same arrays, bit for bit, as the definition: on sampled rows against
    a NumPy restatement, on all rows against the host search (cKDTree with exact re-ranking), including a regular lattice
    (every distance tied many times over), exact duplicates, strongly clustered points and a dimension without extent."""
    G = _need_gpu()
    from gpvecchia_amd import specify as S
    rng = np.random.default_rng(99)
    m = 30
    if case == "uniform2d":
        locs = rng.random((60_000, 2))
    elif case == "uniform3d":
        locs = rng.random((40_000, 3)); m = 20
    elif case == "line1d":
        locs = rng.random((30_000, 1)); m = 10
    elif case == "lattice_ties":
        gx, gy = np.meshgrid(np.arange(160) / 160.0, np.arange(100) / 100.0, indexing="ij")
        locs = np.stack([gx.ravel(), gy.ravel()], axis=1)[rng.permutation(16_000)]; m = 12
    elif case == "duplicates":
        locs = rng.random((20_000, 2))
        dup = rng.choice(np.arange(1, 20_000), 3000, replace=False)
        locs[dup] = locs[dup - 1]
    elif case == "clustered":
        centres = rng.random((40, 2))
        locs = centres[rng.integers(0, 40, 50_000)] + 1e-3 * rng.standard_normal((50_000, 2)); m = 25
    elif case == "thin_slab":                                           # an extent 1e-9 of the others: one cell across it
        locs = rng.random((30_000, 3)) * np.array([1.0, 1.0, 1e-9]); m = 15
    else:
        locs = np.stack([rng.random(20_000), np.full(20_000, 0.25)], axis=1); m = 8
    n = locs.shape[0]
    NN = S.find_ordered_nn_gpu(locs, m)
    rows = np.concatenate([[0, 1, m, m + 1, 4095, 4096, 4097, n - 1], rng.integers(4096, n, 60)])
    assert np.array_equal(NN[rows], _nn_definition_rows(locs, m, rows))
    if case not in ("lattice_ties", "duplicates"):                       # (the host search re-ranks ties itself; keep it to the tie-free cases)
        assert np.array_equal(NN, S.find_ordered_nn(locs, m))
    # a row shard (what one rank of a multi-GPU job asks for) equals the same rows of the full search
    a, b = n // 3, n // 3 + 5000
    sh = S.find_ordered_nn_gpu(locs, m, rows=(a, b))
    assert np.array_equal(sh[a:b], NN[a:b]) and not sh[:a].any() and not sh[b:].any()


# ----------------------------------------------------------------------------------------------------------------
# bench.py --mode S at full size: the posterior pass with the dense top block against the same pass with every column in
# the level schedule (different summation order, same factor)
# ----------------------------------------------------------------------------------------------------------------
_TOP_FULL_SNIPPET = r"""
import json
import numpy as np
import torch  # noqa: F401  (one HIP runtime per process: conftest.py)
import gpvecchia_amd as G
n, m = 1_000_000, 30
rng = np.random.default_rng(0)
locs = rng.random((n, 2)); z = np.random.default_rng(1).standard_normal(n)
tau = 0.05 + 0.1 * rng.random(n)
va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="SGV", nn_backend="gpu")
ll = G.vecchia_likelihood(z, va, [1.0, 0.02, 1.5], tau)
plan = va[("_plan", 0)]
ll2 = G.vecchia_likelihood(z, va, [1.0, 0.02, 1.5], tau)
mu = G.vecchia_prediction(z, va, [1.0, 0.02, 1.5], tau)["mu_obs"]
idx = np.concatenate([np.arange(200), rng.integers(0, n, 2000)])
print("RESULT" + json.dumps(dict(ll=ll, same=bool(ll == ll2), sums=plan.sums().tolist(), levels=plan.posterior_levels(),
                                 mu=mu[idx].tolist(), mu_abs_max=float(np.abs(mu).max()))))
"""


def test_full_size_dense_top_block_n1e6_m30():
    """n = 1e6, m = 30, maxmin + SGV (the reference's defaults; bench.py --mode S): with the dense top block the schedule is
    ~21 levels shorter; log-likelihood, log det W, the quadratic form and the posterior mean agree with the all-levels pass to
    rounding, and the evaluation is bitwise reproducible."""
    _need_gpu()
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for top in ("0", "128"):
        env = dict(os.environ, GPV_POST_TOP=top, PYTHONPATH=root)
        r = subprocess.run([sys.executable, "-c", _TOP_FULL_SNIPPET], capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        res[top] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1][6:])
    a, b = res["0"], res["128"]
    assert a["same"] and b["same"]
    assert 15 <= a["levels"] - b["levels"] <= 70 and b["levels"] >= 60
    assert abs(a["ll"] - b["ll"]) <= 1e-11 * abs(a["ll"])
    np.testing.assert_allclose(b["sums"][2:4], a["sums"][2:4], rtol=1e-11)
    np.testing.assert_allclose(b["mu"], a["mu"], rtol=0, atol=1e-10 * a["mu_abs_max"])
