"""covmodel='matern_scaledim' (one range per coordinate) through every evaluating entry, on the GPU.

Truth: the oracle's isotropic algorithm on locs / ranges with range 1 -- the family's definition -- so the oracle is used as it
is: its vecchia.approx gets the scaled locsord and covparms (variance, 1, smoothness).  Bars: the project's (tests/_parity.py,
tests/test_gpu_configs.py, tests/test_gpu_prediction.py): every row of Lentries within 1e-8 normwise, log-likelihoods within 1e-8
relative, posterior means within 1e-8 max|mean|, the Vecchia-Laplace mean and likelihood within 1e-7 (test_C5 of test_gpu_configs).

Shapes (n = 300 .. 600): rows of p = m + 1 = 1, 16, 17, 32, 33, 64 entries (the buckets of the set kernels and one past their
edges; the first p - 1 rows of every plan are the warm-up rows with fewer entries), dimensions 1, 2, 3 (packed records) and 5
(the coordinate array), ranges 1 : 50 apart and equal, the three closed forms and a general smoothness (its table is fitted over
the plan's distances stretched by the smallest and largest inverse range).  Neighbours are chosen on the scaled coordinates
(vecchia_specify(scale=ranges)), which keeps the blocks as well conditioned as an isotropic plan's.

  test_rows_against_oracle                 Lentries through gpv_U_NZentries (createU), cond.yz = 'z' and 'SGV'
  test_evaluations_against_oracle          loglik for cond.yz = 'z' (m = 30: the lean kernel's row length), 'SGV', 'y'; the posterior
                                           mean of a prediction plan; a Vecchia-Laplace likelihood (Poisson)
  test_without_graph_is_bitwise_the_same   the same results, and the U entries of EVERY case of test_rows_against_oracle, from a child
                                           process under GPV_NO_GRAPH=1 (a switch read once): bitwise what this process computes, so
                                           each check against the oracle holds with and without graphs
  test_two_parameter_sets_on_one_plan      ranges A, ranges B, ranges A on one plan: a stale copy or stale launch arguments
  test_set_data_between_evaluations        a stale datum slot in the copy
  test_nan_parameters_fail_every_row       NaN range / variance, like 'matern'"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROW_TOL = 1e-8
LL_RTOL = 1e-8
TAU = 0.1
FAM = "matern_scaledim"


def _need_gpu():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


def _ranges(dim, kind):
    if kind == "equal":
        return np.full(dim, 0.2)
    return np.array([0.02, 1.0, 0.2][:dim]) if dim > 1 else np.array([0.02])        # 1 : 50


def _to_oracle_va(va, ranges):
    """the oracle's vecchia.approx of the isotropic model this family is: the scaled coordinates"""
    prep = dict(va["U_prep"])
    nn = prep["revNNarray"]
    prep["revNNarray"] = np.where(nn == 0, np.nan, nn.astype(np.float64))
    prep["revCond"] = np.where(prep["revCond"] < 0, np.nan, prep["revCond"].astype(np.float64))
    out = {k: v for k, v in va.items() if not isinstance(k, tuple)}
    out["U_prep"] = prep
    out["locsord"] = va["locsord"] / np.asarray(ranges)
    return out


def _row_err(A, B):
    scale = np.maximum(np.abs(B).max(axis=1), 1e-300)
    return np.abs(A - B).max(axis=1) / scale


CASES = [  # (m, dim, ranges, smoothness, cond.yz)
    (0, 2, "far", 1.5, "z"), (15, 1, "far", 0.5, "z"), (16, 2, "far", 1.5, "SGV"), (31, 3, "far", 2.5, "z"),
    (32, 2, "equal", 0.5, "SGV"), (63, 2, "far", 1.5, "z"), (10, 5, "far5", 1.5, "SGV"), (20, 2, "far", 0.8, "z"),
    (40, 3, "far", 0.8, "z"), (30, 2, "far", 2.5, "z"),
]


def _rows_case(m, dim, kind, nu, cond):
    """the U entries of one case through gpv_U_NZentries, and what the oracle needs to state them"""
    G = _need_gpu()
    n = 300 if m == 63 else 400
    rng = np.random.default_rng(100 + m)
    locs = rng.random((n, dim))
    ranges = np.array([0.02, 1.0, 0.2, 0.5, 0.1]) if kind == "far5" else _ranges(dim, kind)
    cp = np.concatenate([[1.3], ranges, [nu]])
    va = G.vecchia_specify(locs, m, cond_yz=cond, scale=ranges, nn_backend="host")
    return G.createU(va, cp, TAU, covmodel=FAM), va, ranges


def _case_id(c):
    return "m%d-d%d-%s-nu%s-%s" % c


@pytest.mark.parametrize("m,dim,kind,nu,cond", CASES, ids=[_case_id(c) for c in CASES])
def test_rows_against_oracle(m, dim, kind, nu, cond):
    from oracle import r_side as R
    U, va, ranges = _rows_case(m, dim, kind, nu, cond)
    ref = R.createU(_to_oracle_va(va, ranges), [1.3, 1.0, nu], TAU)["U_entries"]
    assert ref["n_failed"] == 0
    err = _row_err(U["Lentries"], ref["Lentries"])
    print(f"worst row {err.max():.3e} (row {int(err.argmax())}), warm-up rows {err[:m + 1].max():.3e}")
    assert err.max() <= ROW_TOL
    np.testing.assert_array_equal(U["Lentries"] == 0, ref["Lentries"] == 0)
    # (the array the child process without graphs is compared with holds these bits)
    assert np.array_equal(U["Lentries"], _evaluated()["rows " + _case_id((m, dim, kind, nu, cond))])
    np.testing.assert_allclose(U["Zentries"], ref["Zentries"], rtol=1e-15)


# ---- one set of evaluations, computed in this process and in a child process without graphs ---------------------------------
_N, _NP = 500, 60
_RANGES = np.array([0.02, 1.0])
_CP = np.array([1.3, 0.02, 1.0, 1.5])
_CP_VL = np.array([0.5, 0.06, 0.9, 1.5])
_R_VL = np.array([0.06, 0.9])


def _inputs():
    rng = np.random.default_rng(7)
    locs, pred = rng.random((_N, 2)), rng.random((_NP, 2))
    z = rng.standard_normal(_N)
    x, y = locs[:, 0], locs[:, 1]
    zp = rng.poisson(np.exp(0.8 * np.sin(5.0 * x) * np.cos(4.0 * y) + 0.3)).astype(float)
    return locs, pred, z, zp


@functools.lru_cache(maxsize=None)
def _plans():
    G = _need_gpu()
    locs, pred, z, zp = _inputs()
    return dict(z=G.vecchia_specify(locs, 30, cond_yz="z", scale=_RANGES, nn_backend="host"),
                sgv=G.vecchia_specify(locs, 12, cond_yz="SGV", scale=_RANGES, nn_backend="host"),
                y=G.vecchia_specify(locs, 12, cond_yz="y", scale=_RANGES, nn_backend="host"),
                pred=G.vecchia_specify(locs, 12, locs_pred=pred, scale=_RANGES, nn_backend="host"),
                vl=G.vecchia_specify(locs, 10, cond_yz="SGV", scale=_R_VL, nn_backend="host"))


def _evaluate():
    """every evaluating entry once; float64 arrays by name"""
    G = _need_gpu()
    locs, pred, z, zp = _inputs()
    va = _plans()
    out = {}
    for c in ("z", "sgv", "y"):
        out["ll_" + c] = np.array([G.vecchia_likelihood(z, va[c], _CP, TAU, covmodel=FAM)])
    out["kind_z"] = np.array([float(va["z"][("_plan", 0)].last_set_kernel())])
    p = G.vecchia_prediction(z, va["pred"], _CP, TAU, covmodel=FAM)
    out["mu_obs"], out["mu_pred"] = np.asarray(p["mu_obs"]), np.asarray(p["mu_pred"])
    post = G.calculate_posterior_VL(zp, va["vl"], "poisson", _CP_VL, covmodel=FAM)
    out["vl_mean"], out["vl_iter"] = np.asarray(post["mean"]), np.array([float(post["iter"])])
    out["vl_ll"] = np.array([G.vecchia_laplace_likelihood(zp, va["vl"], "poisson", _CP_VL, covmodel=FAM)])
    out["L_sgv"] = np.asarray(G.createU(va["sgv"], _CP, TAU, covmodel=FAM)["Lentries"])
    for c in CASES:                                           # every case of test_rows_against_oracle once more: its bits
        out["rows " + _case_id(c)] = np.asarray(_rows_case(*c)[0]["Lentries"])
    return out


@functools.lru_cache(maxsize=None)
def _evaluated():
    return _evaluate()


def test_evaluations_against_oracle():
    G = _need_gpu()
    from oracle import r_side as R
    locs, pred, z, zp = _inputs()
    va, got = _plans(), _evaluated()
    iso = [1.3, 1.0, 1.5]
    assert got["kind_z"][0] == 3          # m = 30, cond.yz = 'z', a constant nugget: the lean likelihood-only kernel ran on the copy
    for c in ("z", "sgv", "y"):
        ll_ref = R.vecchia_likelihood(z, _to_oracle_va(va[c], _RANGES), iso, TAU)
        print(f"loglik cond.yz={c}: {got['ll_' + c][0]!r} oracle {ll_ref!r}")
        assert abs(got["ll_" + c][0] - ll_ref) <= LL_RTOL * abs(ll_ref), c
    mo, mp = R.vecchia_prediction_mean(z, _to_oracle_va(va["pred"], _RANGES), iso, TAU, both=True)
    sc = np.abs(mo).max()
    print("posterior mean: obs off by", np.abs(got["mu_obs"] - mo).max() / sc, "pred off by", np.abs(got["mu_pred"] - mp).max() / sc)
    np.testing.assert_allclose(got["mu_obs"], mo, rtol=0, atol=1e-8 * sc)
    np.testing.assert_allclose(got["mu_pred"], mp, rtol=0, atol=1e-8 * sc)
    vb = _to_oracle_va(va["vl"], _R_VL)
    iso_vl = [0.5, 1.0, 1.5]
    post_ref = R.calculate_posterior_VL(zp, vb, "poisson", iso_vl)
    assert post_ref["cnvgd"] and int(got["vl_iter"][0]) == post_ref["iter"]
    np.testing.assert_allclose(got["vl_mean"], post_ref["mean"], rtol=0, atol=1e-7)
    ll_ref = R.vecchia_laplace_likelihood(zp, vb, "poisson", iso_vl)
    print(f"Vecchia-Laplace likelihood {got['vl_ll'][0]!r} oracle {ll_ref!r}")
    assert abs(got["vl_ll"][0] - ll_ref) <= 1e-7 * abs(ll_ref)


def test_without_graph_is_bitwise_the_same(tmp_path):
    _need_gpu()
    out = str(tmp_path / "nograph.npz")
    env = dict(os.environ, GPV_NO_GRAPH="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    child, here = np.load(out), _evaluated()
    assert set(child.files) == set(here)
    for k in here:
        assert np.array_equal(child[k], here[k]), k


def test_two_parameter_sets_on_one_plan():
    G = _need_gpu()
    from oracle import r_side as R
    locs, pred, z, zp = _inputs()
    va = _plans()["sgv"]                                      # the posterior pass of this plan is a captured graph
    cpA, cpB = _CP, np.array([0.7, 0.3, 0.05, 1.5])           # the ranges swap their order of magnitude
    llA = G.vecchia_likelihood(z, va, cpA, TAU, covmodel=FAM)
    llB = G.vecchia_likelihood(z, va, cpB, TAU, covmodel=FAM)
    llA2 = G.vecchia_likelihood(z, va, cpA, TAU, covmodel=FAM)
    refB = R.vecchia_likelihood(z, _to_oracle_va(va, cpB[1:3]), [0.7, 1.0, 1.5], TAU)
    assert llA2 == llA == _evaluated()["ll_sgv"][0]
    assert abs(llB - refB) <= LL_RTOL * abs(refB) and llB != llA
    # an isotropic evaluation in between reads the plan's own records, and leaves the next scaled one what it was
    llM = G.vecchia_likelihood(z, va, [1.3, 0.2, 1.5], TAU)
    refM = R.vecchia_likelihood(z, _to_oracle_va(va, [1.0, 1.0]), [1.3, 0.2, 1.5], TAU)
    assert abs(llM - refM) <= LL_RTOL * abs(refM)
    assert G.vecchia_likelihood(z, va, cpA, TAU, covmodel=FAM) == llA


@pytest.mark.parametrize("dim", (2, 5))
def test_set_data_between_evaluations(dim):
    G = _need_gpu()
    from oracle import r_side as R
    rng = np.random.default_rng(9)
    n = 400
    locs = rng.random((n, dim))
    z1, z2 = rng.standard_normal(n), rng.standard_normal(n)
    ranges = np.array([0.02, 1.0, 0.2, 0.5, 0.1][:dim])
    cp = np.concatenate([[1.3], ranges, [1.5]])
    va = G.vecchia_specify(locs, 10, cond_yz="z", scale=ranges, nn_backend="host")
    ova = _to_oracle_va(va, ranges)
    for z in (z1, z2, z1):
        ll = G.vecchia_likelihood(z, va, cp, TAU, covmodel=FAM)               # one plan: set_user_data rewrites the datum slot
        ref = R.vecchia_likelihood(z, ova, [1.3, 1.0, 1.5], TAU)
        assert abs(ll - ref) <= LL_RTOL * abs(ref)


def test_nan_parameters_fail_every_row():
    G = _need_gpu()
    rng = np.random.default_rng(3)
    n, m = 300, 5
    locs = rng.random((n, 2))
    va = G.vecchia_specify(locs, m, cond_yz="z", nn_backend="host")
    prep = va["U_prep"]
    tv = np.full(n, TAU)
    want = G.U_NZentries(1, n, va["locsord"], prep["revNNarray"], prep["revCond"], tv, tv, "matern", [1.0, np.nan, 1.5])
    for cp in ([1.0, np.nan, 0.3, 1.5], [1.0, 0.3, np.nan, 1.5], [np.nan, 0.3, 0.2, 1.5]):
        got = G.U_NZentries(1, n, va["locsord"], prep["revNNarray"], prep["revCond"], tv, tv, FAM, cp)
        assert got["n_failed"] == want["n_failed"] == n
        assert np.array_equal(got["Lentries"], want["Lentries"])


if __name__ == "__main__":                                    # the child of test_without_graph_is_bitwise_the_same
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch  # noqa: F401  (first, as in conftest.py: one HIP runtime per process)
    np.savez(sys.argv[1], **_evaluate())
