"""gpv_plan_whiten (gpv_whiten.hip) on the GPU: the Vecchia whitening operator of an evaluation applied to a block of columns,
their Gram matrix, and what is built on it (GLS profile likelihood, replicated data, vecchia_estimate(trend="gls")).

Truth: tests/_whiten_truth.py, the definition (standardised conditional residual under C(J, J) + diag(tau_J)) by a hand-written
long-double Cholesky, independent of Lentries.  Bars (the project's flat 1e-8, tests/_parity.py):
  E       per ordered row, max_c |E_kc - truth_kc| <= 1e-8 max_c |truth_kc|
  G       |G_ij - truth_ij| <= 1e-8 sum_k |e_ki e_kj|;   logdet within 1e-8 sum_k |log term_k|
Inputs: seeded uniform locations in the unit cube, range 0.25 sqrt(d / 2), nuggets 0.1 (constant) or uniform in [0.05, 0.3]
(vector), 16 seeded standard-normal columns of which the first ncols are used.

Consistency with the shipped likelihood: gram[z, z] and logdet against sums[3] and sums[2] of the same evaluation.  The two sides
order their sums differently, so the tolerance is 4 x the agreement of the ORACLE's double evaluation (oracle.r_side.U_NZentries,
then the same two sums in float64) with the long-double truth on the same plan, relative to sum |term|: measured on the CPU for
the two plans below, 2.15e-15 / 1.3e-16 (quadratic form) and 8.3e-16 / 6.4e-16 (logdet); the largest is recorded as
_ORACLE_VS_LD = 2.2e-15.  The test prints the oracle's figures again and holds the oracle to the same 4 x bar."""
import ctypes as C
import functools

import numpy as np
import pytest

import _whiten_truth as W

pytestmark = pytest.mark.gpu

TOL = 1e-8
TAU = 0.1
_ORACLE_VS_LD = 2.2e-15


def _need_gpu():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


def _family(name, d):
    r = 0.25 * np.sqrt(d / 2)
    return {"nu0.5": ("matern", [1.3, r, 0.5]), "nu1.5": ("matern", [1.3, r, 1.5]), "nu2.5": ("matern", [1.3, r, 2.5]),
            "esqe": ("esqe", [0.8, r, 0.5, 0.8 * r])}[name]


@functools.lru_cache(maxsize=None)
def case(m, d=2, n=600, ordering="maxmin", fam="nu1.5", vecnug=False, dup=False, seed=3):
    """Seeded inputs of one plan and their long-double truth, computed once and shared read-only."""
    import gpvecchia_amd as G
    rng = np.random.default_rng(seed)
    locs = rng.random((n, d))
    if dup:
        locs[n // 2] = locs[n // 3]                    # two coincident points
    B = rng.standard_normal((n, 16))
    tau = rng.uniform(0.05, 0.3, n) if vecnug else np.float64(TAU)
    va = G.vecchia_specify(locs, min(m, n - 1), ordering=ordering, cond_yz="z", nn_backend="host")
    cm, cp = _family(fam, d)
    o = va["ord_z"] - 1
    Bord = np.asfortranarray(B[o])
    tau_ord = tau[o] if vecnug else tau
    E, logterm = W.whiten_ld(va["locsord"], va["U_prep"]["revNNarray"], Bord, cm, cp, tau_ord)
    for a in (locs, B, Bord, E, logterm, va["locsord"]):
        a.setflags(write=False)
    return dict(locs=locs, B=B, Bord=Bord, tau=tau, tau_ord=tau_ord, va=va, cm=cm, cp=cp, E=E, logterm=logterm, n=n)


def _fresh(va, **over):
    """a copy of a shared vecchia.approx without the device plan the API may have cached in it"""
    return dict({k: v for k, v in va.items() if isinstance(k, str)}, **over)


def _plan(G, c):
    prep = c["va"]["U_prep"]
    plan = G.Plan(c["va"]["locsord"], prep["revNNarray"], prep["revCond"])
    plan.eval(c["cm"], c["cp"], c["tau_ord"], G.GPV_WANT_U)
    return plan


def check(c, ncols, G_, logdet, E_, what):
    """asserts the three bars; returns the measured figures"""
    Et = c["E"][:, :ncols]
    row = np.abs(E_ - Et.astype(np.float64)).max(axis=1) / np.maximum(np.abs(Et).max(axis=1).astype(np.float64), 1e-300)
    Gt = (Et.T @ Et)
    Gs = (np.abs(Et).T @ np.abs(Et)).astype(np.float64)
    gerr = (np.abs(G_ - Gt.astype(np.float64)) / Gs).max()
    lerr = abs(logdet - float(c["logterm"].sum())) / float(np.abs(c["logterm"]).sum())
    print(f"{what}: worst E row {row.max():.3e} (row {int(row.argmax())}), G {gerr:.3e} of sum|term|, logdet {lerr:.3e} of sum|term|")
    assert np.array_equal(G_, G_.T)
    assert row.max() <= TOL and gerr <= TOL and lerr <= TOL, (what, float(row.max()), float(gerr), float(lerr))
    return float(row.max()), float(gerr), float(lerr)


@pytest.mark.parametrize("m", [0, 1, 15, 16, 31, 40, 70])
def test_row_lengths(m):
    G = _need_gpu()
    c = case(m)
    Gm, logdet, nf, E = _plan(G, c).whiten(c["Bord"], want_E=True)
    assert nf == 0
    check(c, 16, Gm, logdet, E, f"m={m} ncols=16")


@pytest.mark.parametrize("ncols", [1, 3])
@pytest.mark.parametrize("m", [31, 70])
def test_column_counts(m, ncols):
    G = _need_gpu()
    c = case(m)
    Gm, logdet, nf, E = _plan(G, c).whiten(c["Bord"][:, :ncols], want_E=True)
    assert nf == 0 and E.shape == (c["n"], ncols)
    check(c, ncols, Gm, logdet, E, f"m={m} ncols={ncols}")


SHAPES = {
    "d5-esqe-vector-coord": dict(m=16, d=5, ordering="coord", fam="esqe", vecnug=True),
    "d2-vector-maxmin": dict(m=31, vecnug=True),
    "d2-coord-nu0.5": dict(m=15, ordering="coord", fam="nu0.5"),
    "d3-nu2.5": dict(m=40, d=3, fam="nu2.5"),
    "coincident": dict(m=15, ordering="coord", dup=True),
    "n3": dict(m=2, n=3, ordering="none"),
    "n601": dict(m=31, n=601),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name):
    G = _need_gpu()
    c = case(**SHAPES[name])
    for ncols in (16, 3):
        Gm, logdet, nf, E = _plan(G, c).whiten(c["Bord"][:, :ncols], want_E=True)
        assert nf == 0
        check(c, ncols, Gm, logdet, E, f"{name} ncols={ncols}")


def _raw(G, plan, B, ldb, ncols, E, lde, gram, logdet, nf):
    from gpvecchia_amd import _lib as L
    return L.lib().gpv_plan_whiten(plan._h, B, ldb, ncols, E, lde, gram, logdet, nf)


def test_leading_dimensions():
    """ldb, lde > Nlocs: the padding rows are neither read into the result nor written"""
    G = _need_gpu()
    from gpvecchia_amd import _lib as L
    c = case(15)
    n, nc, pad = c["n"], 3, 7
    Bbig = np.full((n + pad, nc), np.nan, order="F")
    Bbig[:n] = c["Bord"][:, :nc]
    Ebig = np.full((n + pad + 2, nc), -7.0, order="F")
    Gm, ld, nf = np.zeros((nc, nc)), C.c_double(0), C.c_int64(-1)
    st = _raw(G, _plan(G, c), L.dptr(Bbig), n + pad, nc, L.dptr(Ebig), n + pad + 2, L.dptr(Gm), C.byref(ld), C.byref(nf))
    assert st == 0 and nf.value == 0
    assert np.all(Ebig[n:] == -7.0)
    check(c, nc, Gm, ld.value, Ebig[:n], "ldb = n + 7, lde = n + 9")


def test_consistent_with_shipped_likelihood():
    G = _need_gpu()
    from oracle import r_side as R
    worst = 0.0
    for kw in (dict(m=31), dict(m=16, d=5, ordering="coord", fam="esqe", vecnug=True)):
        c = case(**kw)
        va, n = c["va"], c["n"]
        z_ord = np.ascontiguousarray(c["Bord"][:, 0])
        prep = va["U_prep"]
        plan = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
        plan.set_data(z_ord)
        plan.eval(c["cm"], c["cp"], c["tau_ord"], G.GPV_WANT_U | G.GPV_WANT_LOGLIK_Z)
        sums = plan.sums()
        Gm, logdet, nf = plan.whiten(z_ord)
        # the oracle's double evaluation of the same two sums against the long-double truth
        tv = np.broadcast_to(c["tau_ord"], (n,))
        nn = np.nan_to_num(np.asarray(prep["revNNarray"], dtype=np.float64), nan=0.0).astype(np.int64)
        ref = R.U_NZentries(R.max_threads(), n, va["locsord"], prep["revNNarray"], np.where(prep["revCond"] < 0, 0, prep["revCond"]),
                            np.array(tv), np.array(tv), c["cm"], c["cp"])["Lentries"]
        quad_o = logdet_o = 0.0
        for k in range(n):
            idx = nn[k][nn[k] > 0] - 1
            row = ref[k, :len(idx)]
            s = tv[k] + 1.0 / row[-1] ** 2
            quad_o += (z_ord[k] + row[:-1] @ z_ord[idx[:-1]] / row[-1]) ** 2 / s
            logdet_o += np.log(s)
        e0 = c["E"][:, 0]
        qs, ls = float((e0 * e0).sum()), float(np.abs(c["logterm"]).sum())
        fig = max(abs(quad_o - float((e0 * e0).sum())) / qs, abs(logdet_o - float(c["logterm"].sum())) / ls)
        dq, dl = abs(Gm[0, 0] - sums[3]) / qs, abs(logdet - sums[2]) / ls
        print(f"{kw}: oracle vs long double {fig:.2e}; whiten vs sums: quadratic form {dq:.2e}, logdet {dl:.2e} (of sum |term|)")
        worst = max(worst, fig)
        assert nf == 0 and sums[6] == 0
        assert dq <= 4 * _ORACLE_VS_LD and dl <= 4 * _ORACLE_VS_LD
    assert worst <= 4 * _ORACLE_VS_LD


def test_state_bitwise_and_last_evaluation_intact():
    G = _need_gpu()
    c = case(31)
    va, prep = c["va"], c["va"]["U_prep"]
    plan = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
    plan.set_data(np.ascontiguousarray(c["Bord"][:, 0]))
    plan.build_posterior()
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_DENOM)              # a posterior factor, so that the stamp is not 0
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U | G.GPV_WANT_LOGLIK_Z)
    sums, Lent, stamp = plan.sums(), plan.Lentries(), plan.factor_stamp()
    assert stamp != 0
    a = plan.whiten(c["Bord"], want_E=True)
    b = plan.whiten(c["Bord"][:, :5])                  # another padded width in between
    a2 = plan.whiten(c["Bord"], want_E=True)
    assert a[0].tobytes() == a2[0].tobytes() and a[1] == a2[1] and a[3].tobytes() == a2[3].tobytes()
    assert b[0].tobytes() == plan.whiten(c["Bord"][:, :5])[0].tobytes()
    assert np.array_equal(plan.sums(), sums) and np.array_equal(plan.Lentries(), Lent) and plan.factor_stamp() == stamp


def test_refusals():
    G = _need_gpu()
    from gpvecchia_amd import _lib as L
    c = case(15)
    va, prep, n = c["va"], c["va"]["U_prep"], c["n"]
    B = c["Bord"]

    def status(fn):
        with pytest.raises(G.GpvError) as e:
            fn()
        return e.value.status

    plan = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
    assert status(lambda: plan.whiten(B)) == 7                                     # GPV_ERR_STATE: no evaluation yet
    plan.set_data(np.ascontiguousarray(B[:, 0]))
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_LOGLIK_Z)
    assert status(lambda: plan.whiten(B)) == 7                                     # the evaluation did not ask for U
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    assert plan.whiten(B)[2] == 0
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_LOGLIK_Z)                          # ... and the next one did not: stale U
    assert status(lambda: plan.whiten(B)) == 7
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    # ---- arguments (GPV_ERR_BAD_ARG = 2), straight at the C entry
    Bf = np.asfortranarray(np.zeros((n, 17)))
    Gm, E = np.zeros((17, 17)), np.zeros((n, 17), order="F")
    ld, nf = C.c_double(0), C.c_int64(0)
    ok = (L.dptr(Bf), n, 3, L.dptr(E), n, L.dptr(Gm), C.byref(ld), C.byref(nf))
    assert _raw(G, plan, *ok) == 0
    for pos, val in ((0, None), (5, None), (6, None), (7, None), (2, 0), (2, -1), (2, 17), (1, n - 1), (4, n - 1)):
        args = list(ok)
        args[pos] = val
        assert _raw(G, plan, *args) == 2, (pos, val)
    assert L.lib().gpv_plan_whiten(None, *ok) == 2
    args = list(ok)
    args[3], args[4] = None, 0                                                     # no E: lde is not looked at
    assert _raw(G, plan, *args) == 0
    assert L.lib().gpv_whiten_max_cols() == 16
    with pytest.raises(ValueError):
        plan.whiten(Bf)                                                            # 17 columns
    with pytest.raises(ValueError):
        plan.whiten(B[:-1])
    # ---- state
    comm = G.Comm(0, 0, 1, lambda mine: mine)
    plan.set_comm(comm)
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    assert status(lambda: plan.whiten(B)) == 7                                     # a communicator is attached
    plan.set_comm(None)
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    assert plan.whiten(B)[2] == 0
    obs = np.ones(n, dtype=bool)
    obs[5] = False
    plan.set_observed(obs)
    assert status(lambda: plan.whiten(B)) == 7                                     # unobserved locations
    plan.set_observed(None)
    assert plan.whiten(B)[2] == 0
    shard = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"], row_begin=0, row_end=n // 2)
    shard.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    assert status(lambda: shard.whiten(B)) == 7                                    # a row shard
    sgv = G.vecchia_specify(np.array(c["locs"]), 15, ordering="coord", cond_yz="SGV", nn_backend="host")
    ps = G.Plan(sgv["locsord"], sgv["U_prep"]["revNNarray"], sgv["U_prep"]["revCond"])
    ps.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    assert status(lambda: ps.whiten(B)) == 7                                       # latent neighbours
    with pytest.raises(ValueError):
        G.vecchia_whiten(c["B"], sgv, c["cp"], TAU)


def test_vl_step_invalidates_the_factor():
    """a Vecchia-Laplace step rewrites the nuggets the resident U was computed with (and, fused, leaves U alone)"""
    G = _need_gpu()
    from gpvecchia_amd import _lib as L
    c = case(15)
    va, prep, n = c["va"], c["va"]["U_prep"], c["n"]
    plan = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
    plan.build_posterior()
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    assert plan.whiten(c["Bord"])[2] == 0
    zc = np.ascontiguousarray(np.random.default_rng(1).poisson(2.0, n).astype(np.float64))
    L.check(L.lib().gpv_plan_vl_begin(plan._h, 2, None, L.dptr(zc), None, None), "gpv_plan_vl_begin")
    cp = np.ascontiguousarray(c["cp"], dtype=np.float64)
    dmax, fl = C.c_double(0), C.c_int(0)
    L.check(L.lib().gpv_plan_vl_step(plan._h, c["cm"].encode(), L.dptr(cp), 3, C.byref(dmax), C.byref(fl)), "gpv_plan_vl_step")
    stale = True
    try:
        Gm, logdet, nf, E = plan.whiten(c["Bord"], want_E=True)
        stale = False                                  # (an unfused pass materialises U with the pseudo-nuggets: then consistent)
    except G.GpvError as e:
        assert e.status == 7
    if not stale:
        D = np.zeros(n)
        L.check(L.lib().gpv_plan_vl_get(plan._h, None, None, L.dptr(D)), "gpv_plan_vl_get")
        Et, lt = W.whiten_ld(va["locsord"], prep["revNNarray"], c["Bord"], c["cm"], c["cp"], D)
        assert np.abs(E - Et.astype(np.float64)).max() <= 1e-8 * np.abs(Et).max()


def test_nan_coordinate():
    G = _need_gpu()
    c = case(15)
    va, prep, n, bad = c["va"], c["va"]["U_prep"], c["n"], 300
    poisoned = np.array(va["locsord"])
    poisoned[bad, 1] = np.nan
    plan = G.Plan(poisoned, prep["revNNarray"], prep["revCond"])
    plan.set_data(np.ascontiguousarray(c["Bord"][:, 0]))
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U | G.GPV_WANT_LOGLIK_Z)
    Gm, logdet, nf, E = plan.whiten(c["Bord"], want_E=True)
    nn = np.nan_to_num(np.asarray(prep["revNNarray"], dtype=np.float64), nan=0.0).astype(np.int64)
    hit = (nn == bad + 1).any(axis=1)
    assert hit.sum() >= 1 and nf == hit.sum() == plan.sums()[6]
    assert np.isnan(logdet) and np.all(np.isnan(Gm))
    assert np.all(np.isnan(E[hit])) and not np.any(np.isnan(E[~hit]))
    Et = c["E"].astype(np.float64)
    assert (np.abs(E[~hit] - Et[~hit]).max(axis=1) <= TOL * np.abs(Et[~hit]).max(axis=1)).all()
    assert np.all(G.vecchia_likelihood_replicates(c["B"][:, :2], _fresh(va, locsord=poisoned), c["cp"], TAU) == -np.inf)


def test_profile_likelihood_equals_dense_gls():
    G = _need_gpu()
    rng = np.random.default_rng(8)
    n = 192                                            # m = n - 1 at the longest row the library takes (m + 1 <= 192)
    locs = rng.random((n, 2))
    X = np.column_stack([np.ones(n), locs[:, 0], locs[:, 1] ** 2])
    z = X @ [2.0, -1.5, 0.7] + rng.standard_normal(n)
    cm, cp = _family("nu1.5", 2)
    va = G.vecchia_specify(locs, n - 1, cond_yz="z", nn_backend="host")
    got = G.vecchia_profile_likelihood(z, X, va, cp, TAU)
    want = W.dense_gls(locs, X, z, cm, cp, TAU)
    for k in ("beta_hat", "beta_cov", "quadform", "logdet", "loglik"):
        err = np.abs(np.asarray(got[k]) - np.asarray(want[k])).max() / np.abs(np.asarray(want[k])).max()
        print(f"{k}: {err:.3e}")
        assert err <= TOL, (k, got[k], want[k])
    E, logdet = G.vecchia_whiten(np.column_stack([X, z]), va, cp, TAU)
    assert abs(logdet - want["logdet"]) <= TOL * abs(want["logdet"])
    assert np.allclose(W.profile_from(E.T @ E, logdet, n)["beta_hat"], want["beta_hat"], rtol=1e-8, atol=0)


def test_replicates_equal_single_likelihoods():
    G = _need_gpu()
    c = case(31)
    rng = np.random.default_rng(4)
    Z = rng.standard_normal((c["n"], 20))
    for tau in (TAU, c["tau"] if c["tau"].ndim else rng.uniform(0.05, 0.3, c["n"])):
        va = _fresh(c["va"])
        ll = G.vecchia_likelihood_replicates(Z, va, c["cp"], tau)
        one = np.array([G.vecchia_likelihood(Z[:, r], va, c["cp"], tau) for r in range(20)])
        print("replicates vs single calls:", np.abs(ll - one).max() / np.abs(one).max())
        assert ll.shape == (20,) and np.all(np.abs(ll - one) <= TOL * np.abs(one))


@functools.lru_cache(maxsize=None)
def _trend_field():
    """n = 1500 draws of a Matern-1.5 field (variance 2, range 0.2) plus noise 0.3 plus the trend 2 - 1.5 x1"""
    rng = np.random.default_rng(2025)
    n = 1500
    locs = rng.random((n, 2))
    r = np.sqrt(((locs[:, None, :] - locs[None, :, :]) ** 2).sum(-1))
    cc = np.sqrt(3.0) / 0.2
    S = 2.0 * (1 + cc * r) * np.exp(-cc * r) + 0.3 * np.eye(n)
    X = np.column_stack([np.ones(n), locs[:, 0]])
    data = X @ [2.0, -1.5] + np.linalg.cholesky(S) @ rng.standard_normal(n)
    return locs, X, data


@pytest.mark.parametrize("method", ["Nelder-Mead", "L-BFGS-B", "fisher"])
def test_estimation_gls(method):
    G = _need_gpu()
    locs, X, data = _trend_field()
    kw = dict(X=X, m=10, cond_yz="z", output_level=0, smoothness=1.5, method=method)
    gls = G.vecchia_estimate(data, locs, trend="gls", **kw)
    ols = G.vecchia_estimate(data, locs, **kw)
    va = G.vecchia_specify(locs, 10, cond_yz="z")
    th = ols["theta_hat"]
    ols_profile = -G.vecchia_profile_likelihood(data, X, va, [th[0], th[1], 1.5], th[2])["loglik"]
    print(method, "gls", gls["neg_loglik"], gls["beta_hat"], gls["beta_se"], gls["theta_hat"], gls["n_evals"],
          "| ols fit: profile value", ols_profile, ols["beta_hat"], ols["theta_hat"])
    assert gls["neg_loglik"] <= ols_profile
    assert np.all(np.abs(gls["beta_hat"] - [2.0, -1.5]) <= 4 * gls["beta_se"])
    assert gls["beta_cov"].shape == (2, 2) and np.allclose(gls["z"], data - X @ gls["beta_hat"], rtol=0, atol=1e-12)
    if method == "fisher":
        assert np.all(np.isfinite(gls["theta_se"])) and len(gls["theta_se"]) == 3


def test_envelope_gradient():
    """the gradient handed to L-BFGS-B against central differences of the profile likelihood"""
    G = _need_gpu()
    from gpvecchia_amd.wrappers import profile_negloglik_grad
    locs, X, data = _trend_field()
    va = G.vecchia_specify(locs, 10, cond_yz="z")
    lg = np.log([1.5, 0.15, 0.4])
    f0, g, _ = profile_negloglik_grad(lg, data, X, va, "matern", 1.5)
    h = 1e-4
    fd = np.zeros(3)
    for i in range(3):
        e = np.zeros(3)
        e[i] = h
        fd[i] = (profile_negloglik_grad(lg + e, data, X, va, "matern", 1.5)[0]
                 - profile_negloglik_grad(lg - e, data, X, va, "matern", 1.5)[0]) / (2 * h)
    print("gradient", g, "central differences", fd, "relative", np.abs(g - fd).max() / np.abs(fd).max())
    assert np.abs(g - fd).max() <= 1e-5 * np.abs(fd).max()
