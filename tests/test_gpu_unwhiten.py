"""gpv_plan_unwhiten / gpv_plan_simulate (gpv_unwhiten.hip) on the GPU: the colouring operator of an evaluation, the exact inverse
of gpv_plan_whiten, its level schedule, and what is built on it (vecchia_unwhiten, vecchia_simulate).

Truth: tests/_unwhiten_truth.py, the definition (conditional weights and variance under C(J, J) + diag(tau_J), then the recursion
in the ordered row sequence) by the hand-written long-double Cholesky of tests/_whiten_truth.py, independent of Lentries.
Bar (the project's flat 1e-8, tests/_parity.py), per column in the max norm:
    max_k |B_kc - T_kc| <= 1e-8 max_k |T_kc|.
The same recursion in float64 numpy agrees with the long-double truth to 4e-15 .. 1e-14 on the n = 600 plans below, so the bar is
far from what a correct kernel produces; every test prints its measured worst figure.
Inputs: the plans of tests/test_gpu_whiten.py (seeded uniform locations, range 0.25 sqrt(d / 2), nuggets 0.1 or uniform in
[0.05, 0.3]) with their 16 seeded standard-normal columns as E; for wide levels n = 20 000 uniform points in given order with
m = 2 and m = 1, whose schedules hold levels far wider than gpv_unwhiten_narrow() = 256 rows beside narrow ones.

Run as a script (`python tests/test_gpu_unwhiten.py OUT.npz`) this file colours the columns of _state_case and simulates 20 draws
and saves both: test_without_graph_is_bitwise_the_same starts it in a fresh child process under GPV_NO_GRAPH=1, a switch the
library reads once."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _unwhiten_truth as U
import _whiten_truth as W
import test_gpu_whiten as TW

pytestmark = pytest.mark.gpu

TOL = 1e-8
TAU = 0.1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


@functools.lru_cache(maxsize=None)
def _truth(key):
    """long-double colouring of the 16 columns of a tests/test_gpu_whiten.py case, computed once and shared read-only"""
    c = _case(dict(key))
    T = U.unwhiten_ld(c["va"]["locsord"], c["va"]["U_prep"]["revNNarray"], c["Bord"], c["cm"], c["cp"], c["tau_ord"])
    T.setflags(write=False)
    return T


def truth(**kw):
    return _case(kw), _truth(_key(kw))


@functools.lru_cache(maxsize=None)
def wide_case(m):
    """n = 20 000 in given order: 36 levels, 9 of them wider than 1024 rows, widest 1742 (m = 2); 21 levels, widest 2788 (m = 1)"""
    import gpvecchia_amd as G
    n = 20000
    locs = np.random.default_rng(3).random((n, 2))
    E = np.asfortranarray(np.random.default_rng(5).standard_normal((n, 16)))
    va = G.vecchia_specify(locs, m, ordering="none", cond_yz="z", nn_backend="host")
    cm, cp = "matern", [1.3, 0.25, 1.5]
    T = U.unwhiten_ld(va["locsord"], va["U_prep"]["revNNarray"], E, cm, cp, TAU)
    for a in (locs, E, T):
        a.setflags(write=False)
    return dict(va=va, cm=cm, cp=cp, tau_ord=np.float64(TAU), Bord=E, n=n), T


def check(T, B, what):
    """asserts the bar per column; returns the worst figure"""
    T = T[:, :B.shape[1]]
    err = np.abs(B - T.astype(np.float64)).max(axis=0) / np.abs(T).max(axis=0).astype(np.float64)
    print(f"{what}: worst column {err.max():.3e}")
    assert np.all(np.isfinite(B)) and err.max() <= TOL, (what, err)
    return float(err.max())


def check_schedule(G, plan, revNN, what):
    from gpvecchia_amd import _lib as L
    narrow = L.lib().gpv_unwhiten_narrow()
    lev = U.levels(revNN)
    want = U.launches(lev, narrow)
    got = plan.unwhiten_levels()
    print(f"{what}: levels {got[0]}, launches {got[1]}, widest level {np.bincount(lev).max()} rows (narrow <= {narrow})")
    assert got == want, (what, got, want)
    return lev


@pytest.mark.parametrize("m", [0, 1, 15, 16, 31, 40, 70])
def test_row_lengths(m):
    G = _need_gpu()
    c, T = truth(m=m)
    plan = TW._plan(G, c)
    B, nf = plan.unwhiten(c["Bord"])
    assert nf == 0
    check(T, B, f"m={m} ncols=16")
    check_schedule(G, plan, c["va"]["U_prep"]["revNNarray"], f"m={m}")


@pytest.mark.parametrize("m", [2, 1])
def test_wide_levels(m):
    """both kinds of launch and the hand-over between them"""
    G = _need_gpu()
    from gpvecchia_amd import _lib as L
    c, T = wide_case(m)
    plan = TW._plan(G, c)
    lev = check_schedule(G, plan, c["va"]["U_prep"]["revNNarray"], f"wide m={m}")
    width = np.bincount(lev)
    narrow = L.lib().gpv_unwhiten_narrow()
    assert (width > narrow).sum() >= 3 and (width <= narrow).sum() >= 3
    for ncols in (16, 3):
        B, nf = plan.unwhiten(c["Bord"][:, :ncols])
        assert nf == 0 and B.shape == (c["n"], ncols)
        check(T, B, f"wide m={m} ncols={ncols}")


@pytest.mark.parametrize("ncols", [1, 3])
@pytest.mark.parametrize("m", [31, 70])
def test_column_counts(m, ncols):
    G = _need_gpu()
    c, T = truth(m=m)
    B, nf = TW._plan(G, c).unwhiten(c["Bord"][:, :ncols])
    assert nf == 0 and B.shape == (c["n"], ncols)
    check(T, B, f"m={m} ncols={ncols}")


@pytest.mark.parametrize("name", list(TW.SHAPES))
def test_shapes(name):
    G = _need_gpu()
    c, T = truth(**TW.SHAPES[name])
    plan = TW._plan(G, c)
    for ncols in (16, 3):
        B, nf = plan.unwhiten(c["Bord"][:, :ncols])
        assert nf == 0
        check(T, B, f"{name} ncols={ncols}")
    check_schedule(G, plan, c["va"]["U_prep"]["revNNarray"], name)


def _raw(plan, E, lde, ncols, B, ldb, nf):
    from gpvecchia_amd import _lib as L
    return L.lib().gpv_plan_unwhiten(plan._h, E, lde, ncols, B, ldb, nf)


def test_leading_dimensions_and_in_place():
    """lde, ldb > Nlocs: the padding rows are neither read into the result nor written; B_ord may be E_ord"""
    G = _need_gpu()
    from gpvecchia_amd import _lib as L
    c, T = truth(m=15)
    n, nc, pad = c["n"], 3, 7
    Ebig = np.full((n + pad, nc), np.nan, order="F")
    Ebig[:n] = c["Bord"][:, :nc]
    Bbig = np.full((n + pad + 2, nc), -7.0, order="F")
    nf = C.c_int64(-1)
    plan = TW._plan(G, c)
    assert _raw(plan, L.dptr(Ebig), n + pad, nc, L.dptr(Bbig), n + pad + 2, C.byref(nf)) == 0 and nf.value == 0
    assert np.all(Bbig[n:] == -7.0)
    check(T, Bbig[:n], "lde = n + 7, ldb = n + 9")
    Ebig[n:] = -3.0
    assert _raw(plan, L.dptr(Ebig), n + pad, nc, L.dptr(Ebig), n + pad, C.byref(nf)) == 0 and nf.value == 0
    assert np.all(Ebig[n:] == -3.0) and Ebig[:n].tobytes() == Bbig[:n].tobytes()


ANY_FAMILY = {
    "matern-nu0.8": dict(d=2, m=15, cm="matern", cp=[1.3, 0.25, 0.8], vecnug=False),
    "scaledim-3d": dict(d=3, m=20, cm="matern_scaledim", cp=[1.3, 0.1, 0.3, 0.5, 1.5], vecnug=False),
    "vector-nugget": dict(d=2, m=31, cm="matern", cp=[1.3, 0.25, 1.5], vecnug=True),
}


@pytest.mark.parametrize("name", list(ANY_FAMILY))
def test_inverse_of_whitening(name):
    """families the long-double truth does not know: whiten(unwhiten(E)) = E, and unwhiten leaves whitening's bits alone"""
    G = _need_gpu()
    k = ANY_FAMILY[name]
    rng = np.random.default_rng(11)
    n = 600
    locs = rng.random((n, k["d"]))
    E = np.asfortranarray(rng.standard_normal((n, 16)))
    va = G.vecchia_specify(locs, k["m"], cond_yz="z", nn_backend="host")
    tau = rng.uniform(0.05, 0.3, n)[va["ord_z"] - 1] if k["vecnug"] else TAU
    plan = G.Plan(va["locsord"], va["U_prep"]["revNNarray"], va["U_prep"]["revCond"])
    plan.eval(k["cm"], k["cp"], tau, G.GPV_WANT_U)
    w1 = plan.whiten(E, want_E=True)
    B, nf = plan.unwhiten(E)
    assert nf == 0 and np.all(np.isfinite(B))
    w2 = plan.whiten(E, want_E=True)
    assert w1[0].tobytes() == w2[0].tobytes() and w1[1] == w2[1] and w1[3].tobytes() == w2[3].tobytes()
    _, _, nf2, E2 = plan.whiten(B, want_E=True)
    err = np.abs(E2 - E).max(axis=0) / np.abs(E).max(axis=0)
    print(f"{name}: whiten(unwhiten(E)) - E, worst column {err.max():.3e}")
    assert nf2 == 0 and err.max() <= TOL


def test_full_conditioning_is_the_cholesky_factor():
    """n = 48, m = 47: the 48 identity columns (three calls) give the lower Cholesky factor of C_ord + tau I"""
    G = _need_gpu()
    n = 48
    locs = np.random.default_rng(3).random((n, 2))
    cm, cp = TW._family("nu1.5", 2)
    va = G.vecchia_specify(locs, n - 1, cond_yz="z", nn_backend="host")
    plan = G.Plan(va["locsord"], va["U_prep"]["revNNarray"], va["U_prep"]["revCond"])
    plan.eval(cm, cp, TAU, G.GPV_WANT_U)
    eye = np.eye(n)
    A = np.column_stack([plan.unwhiten(eye[:, c0:c0 + 16])[0] for c0 in range(0, n, 16)])
    S = np.asarray(W._cov_and_derivs(W._dist(np.asarray(va["locsord"], dtype=np.float64)), cm, cp)[0], dtype=np.float64) + TAU * np.eye(n)
    Lc = np.linalg.cholesky(S)
    err = np.abs(A - Lc).max() / np.abs(Lc).max()
    print(f"A - chol(C + tau I): {err:.3e} of the largest entry")
    assert np.all(np.triu(A, 1) == 0.0) and err <= TOL


def _state_case(G):
    """n = 600, m = 31, 16 columns: shared by the state tests and the child process (no truth needed)"""
    rng = np.random.default_rng(3)
    n = 600
    locs = rng.random((n, 2))
    E = np.asfortranarray(rng.standard_normal((n, 16)))
    va = G.vecchia_specify(locs, 31, cond_yz="z", nn_backend="host")
    cm, cp = TW._family("nu1.5", 2)
    return dict(va=va, cm=cm, cp=cp, E=E, n=n)


def _state_plan(G, s):
    plan = G.Plan(s["va"]["locsord"], s["va"]["U_prep"]["revNNarray"], s["va"]["U_prep"]["revCond"])
    plan.eval(s["cm"], s["cp"], TAU, G.GPV_WANT_U)
    return plan


def test_state_bitwise_and_last_evaluation_intact():
    G = _need_gpu()
    s = _state_case(G)
    va, prep = s["va"], s["va"]["U_prep"]
    plan = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
    plan.set_data(np.ascontiguousarray(s["E"][:, 0]))
    plan.build_posterior()
    plan.eval(s["cm"], s["cp"], TAU, G.GPV_WANT_DENOM)              # a posterior factor, so that the stamp is not 0
    plan.eval(s["cm"], s["cp"], TAU, G.GPV_WANT_U | G.GPV_WANT_LOGLIK_Z)
    sums, Lent, stamp = plan.sums(), plan.Lentries(), plan.factor_stamp()
    assert stamp != 0
    a = plan.unwhiten(s["E"])
    b = plan.unwhiten(s["E"][:, :5])                   # another padded width in between
    z = plan.simulate(7, 3)
    a2 = plan.unwhiten(s["E"])
    assert a[0].tobytes() == a2[0].tobytes() and a[1] == a2[1] == 0
    assert b[0].tobytes() == plan.unwhiten(s["E"][:, :5])[0].tobytes()
    assert z[0].tobytes() == plan.simulate(7, 3)[0].tobytes()
    assert np.array_equal(plan.sums(), sums) and np.array_equal(plan.Lentries(), Lent) and plan.factor_stamp() == stamp
    # another evaluation: the sweep follows the new factor and the new nugget
    plan.eval(s["cm"], s["cp"], 2 * TAU, G.GPV_WANT_U)
    c2 = plan.unwhiten(s["E"])[0]
    assert c2.tobytes() != a[0].tobytes()
    fresh = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
    fresh.eval(s["cm"], s["cp"], 2 * TAU, G.GPV_WANT_U)
    assert fresh.unwhiten(s["E"])[0].tobytes() == c2.tobytes()


def test_without_graph_is_bitwise_the_same(tmp_path):
    G = _need_gpu()
    s = _state_case(G)
    plan = _state_plan(G, s)
    out = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, GPV_NO_GRAPH="1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    child = np.load(out)
    assert child["B"].tobytes() == plan.unwhiten(s["E"])[0].tobytes()
    assert child["Z"].tobytes() == plan.simulate(7, 20)[0].tobytes()


def test_refusals():
    G = _need_gpu()
    from gpvecchia_amd import _lib as L
    c = TW.case(15)
    va, prep, n = c["va"], c["va"]["U_prep"], c["n"]
    E = c["Bord"]

    def status(fn):
        with pytest.raises(G.GpvError) as e:
            fn()
        return e.value.status

    def both(plan):
        return status(lambda: plan.unwhiten(E)), status(lambda: plan.simulate(1, 2))

    plan = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
    assert both(plan) == (7, 7)                                                    # GPV_ERR_STATE: no evaluation yet
    assert plan.unwhiten_levels()[0] >= 16                                         # (the schedule needs no evaluation)
    plan.set_data(np.ascontiguousarray(E[:, 0]))
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_LOGLIK_Z)
    assert both(plan) == (7, 7)                                                    # the evaluation did not ask for U
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    assert plan.unwhiten(E)[1] == 0 and plan.simulate(1, 2)[1] == 0
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_LOGLIK_Z)                          # ... and the next one did not: stale U
    assert both(plan) == (7, 7)
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    # ---- arguments (GPV_ERR_BAD_ARG = 2), straight at the C entries
    Ef, Bf = np.asfortranarray(np.zeros((n, 17))), np.zeros((n, 17), order="F")
    nf = C.c_int64(0)
    ok = (L.dptr(Ef), n, 3, L.dptr(Bf), n, C.byref(nf))
    assert _raw(plan, *ok) == 0
    for pos, val in ((0, None), (3, None), (5, None), (2, 0), (2, -1), (2, 17), (1, n - 1), (4, n - 1)):
        args = list(ok)
        args[pos] = val
        assert _raw(plan, *args) == 2, (pos, val)
    assert L.lib().gpv_plan_unwhiten(None, *ok) == 2
    sim = L.lib().gpv_plan_simulate
    oks = (5, 0, 3, L.dptr(Bf), n, C.byref(nf))
    assert sim(plan._h, *oks) == 0
    for pos, val in ((1, -1), (2, 0), (2, -4), (3, None), (4, n - 1), (5, None)):
        args = list(oks)
        args[pos] = val
        assert sim(plan._h, *args) == 2, (pos, val)
    assert sim(None, *oks) == 2
    nl = C.c_int64(0)
    assert L.lib().gpv_plan_unwhiten_levels(plan._h, None, C.byref(nl)) == 2
    assert L.lib().gpv_plan_unwhiten_levels(plan._h, C.byref(nl), None) == 2
    assert L.lib().gpv_plan_unwhiten_levels(None, C.byref(nl), C.byref(nl)) == 2
    with pytest.raises(ValueError):
        plan.unwhiten(Ef)                                                          # 17 columns
    with pytest.raises(ValueError):
        plan.unwhiten(E[:-1])
    with pytest.raises(ValueError):
        plan.simulate(1, 0)
    # ---- state
    comm = G.Comm(0, 0, 1, lambda mine: mine)
    plan.set_comm(comm)
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    assert both(plan) == (7, 7)                                                    # a communicator is attached
    plan.set_comm(None)
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    assert plan.unwhiten(E)[1] == 0
    obs = np.ones(n, dtype=bool)
    obs[5] = False
    plan.set_observed(obs)
    assert both(plan) == (7, 7)                                                    # unobserved locations
    plan.set_observed(None)
    assert plan.unwhiten(E)[1] == 0
    shard = G.Plan(va["locsord"], prep["revNNarray"], prep["revCond"], row_begin=0, row_end=n // 2)
    shard.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    assert both(shard) == (7, 7) and status(shard.unwhiten_levels) == 7            # a row shard
    sgv = G.vecchia_specify(np.array(c["locs"]), 15, ordering="coord", cond_yz="SGV", nn_backend="host")
    ps = G.Plan(sgv["locsord"], sgv["U_prep"]["revNNarray"], sgv["U_prep"]["revCond"])
    ps.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    assert both(ps) == (7, 7) and status(ps.unwhiten_levels) == 7                  # latent neighbours
    with pytest.raises(ValueError):
        G.vecchia_unwhiten(c["B"], sgv, c["cp"], TAU)
    with pytest.raises(ValueError):
        G.vecchia_simulate(sgv, c["cp"], TAU)


def test_nan_coordinate():
    """a failed row, provoked as tests/test_gpu_whiten.py provokes one: n_failed >= 1 and every entry NaN"""
    G = _need_gpu()
    c = TW.case(15)
    va, prep, n, bad = c["va"], c["va"]["U_prep"], c["n"], 300
    poisoned = np.array(va["locsord"])
    poisoned[bad, 1] = np.nan
    plan = G.Plan(poisoned, prep["revNNarray"], prep["revCond"])
    plan.eval(c["cm"], c["cp"], TAU, G.GPV_WANT_U)
    nn = np.nan_to_num(np.asarray(prep["revNNarray"], dtype=np.float64), nan=0.0).astype(np.int64)
    hit = (nn == bad + 1).any(axis=1)
    B, nf = plan.unwhiten(c["Bord"][:, :3])
    assert hit.sum() >= 1 and nf == hit.sum() and B.shape == (n, 3) and np.all(np.isnan(B))
    Z, nf = plan.simulate(3, 18)
    assert nf == hit.sum() and Z.shape == (n, 18) and np.all(np.isnan(Z))
    assert np.all(np.isnan(G.vecchia_simulate(TW._fresh(va, locsord=poisoned), c["cp"], TAU, nsim=2)))


def test_simulate_columns_are_independent_of_the_call():
    G = _need_gpu()
    s = _state_case(G)
    plan = _state_plan(G, s)
    Z, nf = plan.simulate(9, 20)
    assert nf == 0 and Z.shape == (s["n"], 20)
    assert Z[:, 17].tobytes() == plan.simulate(9, 1, col0=17)[0][:, 0].tobytes()
    assert Z[:, 14:19].tobytes() == plan.simulate(9, 5, col0=14)[0].tobytes()      # across the batch boundary at 16
    assert not np.array_equal(Z, plan.simulate(10, 20)[0])


def test_simulate_is_the_colouring_of_the_host_normals():
    G = _need_gpu()
    c = TW.case(31)
    col0, ncols = 13, 6                                                            # draws 13 .. 18: two batches
    N = np.asfortranarray(G.draws_normals_host(21, 0, c["n"], col0, ncols).T)
    T = U.unwhiten_ld(c["va"]["locsord"], c["va"]["U_prep"]["revNNarray"], N, c["cm"], c["cp"], c["tau_ord"])
    Z, nf = TW._plan(G, c).simulate(21, ncols, col0=col0)
    assert nf == 0
    check(T, Z, "simulate(21, 6, col0=13) against the long-double colouring of the host normals")


def test_vecchia_simulate_and_unwhiten():
    G = _need_gpu()
    c = TW.case(m=31, vecnug=True)
    va, n = TW._fresh(c["va"]), c["n"]
    nsim = 18
    Z = G.vecchia_simulate(va, c["cp"], c["tau"], nsim=nsim, seed=4)
    assert Z.shape == (n, nsim) and np.all(np.isfinite(Z))
    N = G.draws_normals_host(4, 0, n, 0, nsim).T
    Eback, _ = G.vecchia_whiten(Z, va, c["cp"], c["tau"])
    err = np.abs(Eback - N).max(axis=0) / np.abs(N).max(axis=0)
    print(f"vecchia_whiten(vecchia_simulate) - normals: worst column {err.max():.3e}")
    assert err.max() <= TOL
    # caller's order: the ordered rows are the long-double colouring of the normals
    T = U.unwhiten_ld(va["locsord"], va["U_prep"]["revNNarray"], np.asfortranarray(N), c["cm"], c["cp"], c["tau_ord"])
    check(T, Z[va["ord_z"] - 1], "vecchia_simulate in the ordered numbering")
    # mean, seeds
    mu = np.linspace(-1.0, 2.0, n)
    assert np.array_equal(G.vecchia_simulate(va, c["cp"], c["tau"], nsim=nsim, seed=4, mean=mu), Z + mu[:, None])
    assert np.array_equal(G.vecchia_simulate(va, c["cp"], c["tau"], nsim=nsim, seed=4, mean=2.5), Z + 2.5)
    assert np.array_equal(G.vecchia_simulate(va, c["cp"], c["tau"], nsim=3, seed=4), Z[:, :3])
    assert not np.array_equal(G.vecchia_simulate(va, c["cp"], c["tau"], nsim=nsim, seed=5), Z)
    # vecchia_unwhiten: 18 columns in two batches (16 + 2), the mirror of vecchia_whiten, from the caller's order back to it
    B = G.vecchia_unwhiten(N, va, c["cp"], c["tau"])
    check(T, B[va["ord_z"] - 1], "vecchia_unwhiten of the host normals")
    Eb2, _ = G.vecchia_whiten(B, va, c["cp"], c["tau"])
    assert (np.abs(Eb2 - N).max(axis=0) <= TOL * np.abs(N).max(axis=0)).all()


if __name__ == "__main__":
    import torch  # noqa: F401  (first: see tests/conftest.py)
    sys.path.insert(0, ROOT)
    import gpvecchia_amd as G
    s = _state_case(G)
    plan = _state_plan(G, s)
    np.savez(sys.argv[1], B=plan.unwhiten(s["E"])[0], Z=plan.simulate(7, 20)[0])
