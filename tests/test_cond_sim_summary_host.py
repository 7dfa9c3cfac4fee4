"""What vecchia_cond_sim_summary and its GPU tests rest on, on the CPU: the NumPy folds of tests/_csim_summary_truth.py against a
literal loop on a hand-made array (the NaN rule, overlap, weights of both signs, an empty region and one without a live member),
the regions of the public function as lists and as CSR over sweep rows, and its argument checks, which raise before a plan is
asked for.  No device."""
import math

import numpy as np
import pytest

import _csim_summary_truth as ST


def _literal(Y, mu, live, link, thr, regptr, regidx, regw):
    """the contract of include/gpvecchia.h, entry by entry"""
    nq, N = Y.shape
    nreg = len(regptr) - 1
    gf = [lambda y: y, math.exp, lambda y: 1.0 / (1.0 + math.exp(-y))][link]
    out = dict(mc_mean=[math.nan] * nq, mc_var=[math.nan] * nq, exceed=[[math.nan] * nq for _ in thr],
               total=[[0.0] * N for _ in range(nreg)], max=[[math.nan] * N for _ in range(nreg)],
               min=[[math.nan] * N for _ in range(nreg)], area=[[[0.0] * N for _ in range(nreg)] for _ in thr],
               weight=[0.0] * nreg, count=[0] * nreg)
    for i in range(nq):
        if not live[i]:
            continue
        d = [gf(Y[i, j]) - gf(mu[i]) for j in range(N)]
        s1, s2 = math.fsum(d), math.fsum(x * x for x in d)
        out["mc_mean"][i] = gf(mu[i]) + s1 / N
        out["mc_var"][i] = max((s2 - s1 * s1 / N) / (N - 1), 0.0)
        for t, v in enumerate(thr):
            out["exceed"][t][i] = sum(1 for j in range(N) if Y[i, j] > v) / N
    for r in range(nreg):
        mem = [(int(regidx[e]), 1.0 if regw is None else float(regw[e])) for e in range(regptr[r], regptr[r + 1]) if live[regidx[e]]]
        out["count"][r] = len(mem)
        out["weight"][r] = math.fsum(w for _, w in mem)
        for j in range(N):
            if not mem:
                continue
            out["total"][r][j] = math.fsum(w * gf(Y[i, j]) for i, w in mem)
            out["max"][r][j] = max(Y[i, j] for i, _ in mem)
            out["min"][r][j] = min(Y[i, j] for i, _ in mem)
            for t, v in enumerate(thr):
                out["area"][t][r][j] = math.fsum(w for i, w in mem if Y[i, j] > v)
    return {k: np.array(v, dtype=np.float64 if k != "count" else np.int64) for k, v in out.items()}


def _hand_made():
    rng = np.random.default_rng(5)
    nq, N = 9, 5
    mu = rng.standard_normal(nq)
    Y = mu[:, None] + 0.7 * rng.standard_normal((nq, N))
    live = np.ones(nq, dtype=bool)
    live[[3, 6]] = False
    Y[~live] = np.nan
    mu[~live] = np.nan
    regions = [[0, 1, 2, 3, 4], [4, 5, 8, 2], [], [3, 6], [7], [1, 1, 5]]          # overlap, empty, none live, one, a repeat
    weights = [[1.0, 2.0, -0.5, 9.0, 0.25], [1.5, -2.0, 0.125, 3.0], [], [1.0, 1.0], [-4.0], [1.0, 0.5, 2.0]]
    return Y, mu, live, regions, weights


@pytest.mark.parametrize("link", [0, 1, 2])
@pytest.mark.parametrize("weighted", [False, True])
def test_numpy_folds_against_a_literal_loop(link, weighted):
    Y, mu, live, regions, weights = _hand_made()
    thr = [-0.3, 0.4]
    regptr, regidx, regw = ST.csr(regions, weights if weighted else None)
    lit = _literal(Y, mu, live, link, thr, regptr, regidx, regw)
    loc = ST.location_truth(Y, mu, live, link, thr)
    reg = ST.region_truth(Y, live, link, thr, regptr, regidx, regw)
    for k in ("mc_mean", "mc_var", "exceed"):
        assert np.array_equal(np.isnan(loc[k]), np.isnan(lit[k])), k
        assert np.allclose(loc[k], lit[k], rtol=1e-14, atol=0, equal_nan=True), k
    assert np.array_equal(loc["exceed"], lit["exceed"], equal_nan=True)
    for k in ("max", "min", "count"):
        assert np.array_equal(reg[k], lit[k], equal_nan=True), k
    for k in ("total", "area", "weight"):
        assert np.allclose(reg[k], lit[k], rtol=1e-14, atol=1e-15), k
    if not weighted:
        assert np.array_equal(reg["area"], lit["area"]) and np.array_equal(reg["weight"], reg["count"].astype(float))
    # the rules: not live -> NaN per location and no part in a region; empty and all-dead regions
    assert np.isnan(loc["mc_mean"][[3, 6]]).all() and np.isnan(loc["exceed"][:, [3, 6]]).all()
    assert list(reg["count"]) == [4, 4, 0, 0, 1, 3]
    for r in (2, 3):
        assert np.all(reg["total"][r] == 0) and np.all(reg["area"][:, r] == 0) and np.isnan(reg["max"][r]).all() and reg["weight"][r] == 0
    assert np.all(reg["total_mag"] >= np.abs(reg["total"]) * (1 - 1e-15))
    assert np.array_equal(reg["max"][4], Y[7]) and np.array_equal(reg["min"][4], Y[7])


def test_regions_from_labels_lists_and_none():
    from gpvecchia_amd import api as A
    n_p = 7
    lab = np.array([3, -1, 0, 3, 9, 0, 3])
    mem, wts, ids = A.cond_sim_regions(lab, None, n_p)
    assert list(ids) == [0, 3, 9] and [list(x) for x in mem] == [[2, 5], [0, 3, 6], [4]] and all(np.all(w == 1.0) for w in wts)
    area = np.arange(1.0, 8.0)
    mem, wts, ids = A.cond_sim_regions(list(lab), area, n_p)                       # labels as a list, weights per location
    assert [list(w) for w in wts] == [[3.0, 6.0], [1.0, 4.0, 7.0], [5.0]]
    mem, wts, ids = A.cond_sim_regions(None, area, n_p)
    assert len(mem) == 1 and list(mem[0]) == list(range(n_p)) and list(wts[0]) == list(area)
    mem, wts, ids = A.cond_sim_regions([[6, 0], [], [0, 1, 2]], [[-1.0, 2.0], [], [0.5, 0.5, 0.5]], n_p)   # overlap, empty
    assert list(ids) == [0, 1, 2] and [list(x) for x in mem] == [[6, 0], [], [0, 1, 2]] and list(wts[0]) == [-1.0, 2.0]
    # CSR over sweep rows: position k of the sweep takes location o[k]; members in ascending sweep row, weights with them
    o = np.array([4, 6, 1, 0, 5, 3, 2])
    pos = np.empty(n_p, dtype=np.int64)
    pos[o] = np.arange(n_p)
    regptr, regidx, regw = A.cond_sim_regions_csr(mem, wts, pos)
    assert list(regptr) == [0, 2, 2, 5] and regidx.dtype == np.int32
    assert list(regidx) == [1, 3, 2, 3, 6] and list(regw) == [-1.0, 2.0, 0.5, 0.5, 0.5]
    assert list(o[regidx[:2]]) == [6, 0]
    for bad_regions, bad_weights in ((np.array([0, 1, -2, 0, 0, 0, 0]), None), (np.zeros(6, dtype=int), None), (np.zeros(7), None),
                                     ([[0, 7]], None), ([[-1]], None), ([[0.5]], None), (lab, np.ones(6)), (lab, np.full(7, np.inf)),
                                     ([[0, 1]], [[1.0]]), ([[0, 1]], [[1.0, np.nan]]), ([[0], [1]], [[1.0]]), (lab, [[1.0]] * 3)):
        with pytest.raises(ValueError):
            A.cond_sim_regions(bad_regions, bad_weights, n_p)


def test_argument_checks_raise_before_any_device_work(monkeypatch):
    import gpvecchia_amd as G
    from gpvecchia_amd import api as A

    def no_plan(*a, **k):
        raise AssertionError("the plan was asked for")
    monkeypatch.setattr(A, "_plan_for", no_plan)
    rng = np.random.default_rng(1)
    n, n_p = 40, 6
    locs, q = rng.random((n, 2)), rng.random((n_p, 2))
    z = rng.standard_normal(n)
    va = G.vecchia_specify(locs, 5, ordering="none", cond_yz="z")
    ok = dict(covparms=[1.0, 0.2, 1.5], nuggets=0.1, m=5, nsim=4)
    call = lambda **kw: G.vecchia_cond_sim_summary(kw.pop("z", z), kw.pop("va", va), q, **dict(ok, **kw))
    for kw in (dict(link="probit"), dict(nsim=1), dict(col0=-1), dict(thresholds=np.arange(9.0)), dict(thresholds=[np.nan]),
               dict(z=np.stack([z, z], axis=1)), dict(regions=np.array([0, 1, 2, 0, 1, -3])), dict(regions=[[0, 6]]),
               dict(regions=np.zeros(5, dtype=int)), dict(weights=np.ones(5)), dict(weights=np.array([1, 1, 1, 1, 1, np.nan])),
               dict(regions=[[0, 1]], weights=[[1.0]]), dict(order="random"), dict(order=[0, 1, 2, 3, 4, 4]),
               dict(va=G.vecchia_specify(locs, 5, ordering="none", cond_yz="SGV")), dict(covmodel=lambda d: d)):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(AssertionError, match="the plan was asked for"):            # valid arguments reach the plan
        call(regions=np.array([0, 1, -1, 0, 1, 1]), weights=np.ones(n_p), link="exp", thresholds=[0.0], order="given")
