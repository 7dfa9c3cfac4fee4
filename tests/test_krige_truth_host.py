"""The truth of the local-kriging tests (tests/_krige_truth.py) proves itself on the CPU, and the host search
(specify.find_query_nn) equals the search definition.

  * with m = n the per-query solve IS the dense GP conditional: mean k'K^-1 z and variance c0 - k'K^-1 k by the textbook formulas;
  * the chain rule: appending a location to a cond.yz='z' plan as its last row adds exactly log N(z0; mean, var + tau0) to the
    oracle's likelihood, wherever the location lies;
  * find_query_nn on random points, a grid full of ties, duplicates, queries on observations and outside the box, with an
    eligibility mask and with non-finite inputs.
"""
import numpy as np
import pytest

import _krige_truth as KT
from gpvecchia_amd import specify as S

FAMILIES = [("matern", [1.3, 0.25, 1.5]), ("matern", [1.3, 0.25, 0.8]), ("esqe", [1.0, 0.3, 0.5, 0.2]),
            ("matern_scaledim", [1.3, 0.2, 0.4, 2.5])]


@pytest.mark.parametrize("covmodel,cp", FAMILIES)
def test_m_equal_n_is_the_dense_conditional(covmodel, cp):
    rng = np.random.default_rng(11)
    n = 40
    locs, q = rng.random((n, 2)), np.vstack([rng.random((6, 2)), [[1.4, -0.2]]])
    Z = rng.standard_normal((n, 3))
    tau = 0.05 + 0.1 * rng.random(n)
    NN = KT.query_nn(locs, q, n)
    assert (np.sort(NN, axis=1) == np.arange(1, n + 1)).all()
    mean, var, _, failed = KT.krige_ld(locs, tau, Z, q, NN, covmodel, cp)
    m64, v64 = KT.dense_conditional_f64(locs, tau, Z, q, covmodel, cp)
    assert not failed.any()
    assert np.abs(mean - m64).max() <= 1e-9 * np.abs(Z).max() and np.abs(var - v64).max() <= 1e-9 * cp[0]


@pytest.mark.parametrize("covmodel,cp", FAMILIES)
def test_chain_rule_against_the_oracle(covmodel, cp):
    """loglik([z; z0]) = loglik(z) + log N(z0; mean(s0), var(s0) + tau0) for the oracle's cond.yz='z' likelihood with s0 as the
    LAST row, for locations inside, on the edge of and outside the observed region"""
    from oracle import r_side as R
    rng = np.random.default_rng(12)
    n, m = 60, 7
    locs, z = rng.random((n, 2)), rng.standard_normal(n)
    tau, tau0, z0 = 0.1, 0.07, 0.4
    if covmodel == "matern_scaledim":                    # the oracle's isotropic algorithm on locs / ranges at range 1
        sc = np.array(cp[1:3])
        ocov, ocp = "matern", [cp[0], 1.0, cp[3]]
    else:
        sc, ocov, ocp = np.ones(2), covmodel, cp
    ll = R.vecchia_likelihood(z, R.vecchia_specify(locs / sc, m, ordering="none", cond_yz="z"), ocp, tau, ocov)
    for s0 in ([0.5, 0.5], [0.0, 0.31], [1.7, -0.4], locs[:5].mean(axis=0)):
        s0 = np.asarray(s0, dtype=np.float64)[None, :]
        NN = KT.query_nn(locs / sc, s0 / sc, m)
        mean, var, _, failed = KT.krige_ld(locs, tau, z, s0, NN, covmodel, cp)
        assert not failed.any()
        va1 = R.vecchia_specify(np.vstack([locs, s0]) / sc, m, ordering="none", cond_yz="z")
        ll1 = R.vecchia_likelihood(np.append(z, z0), va1, ocp, np.append(np.full(n, tau), tau0), ocov)
        want = ll + KT.log_density(z0, mean[0, 0], var[0] + tau0)
        assert abs(ll1 - want) <= 1e-10 * abs(ll1), (s0, ll1, want)


def _same(locs, q, m, eligible=None):
    got = S.find_query_nn(locs, q, m, eligible=eligible)
    want = KT.query_nn(locs, q, m, eligible=eligible)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:10]


@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_host_search_random(dim):
    rng = np.random.default_rng(20 + dim)
    locs, q = rng.random((500, dim)), rng.random((130, dim))
    for m in (1, 15, 30):
        _same(locs, q, m)
    _same(locs[:5], q, 10)                               # fewer points than m: 0-padded


def test_host_search_ties_duplicates_on_points_outside():
    for locs, q in (KT.tie_grid(), KT.duplicated(), KT.on_points(), KT.outside_box()):
        for m in (1, 15, 30):
            _same(locs, q, m)


def test_host_search_mask_and_nonfinite():
    rng = np.random.default_rng(30)
    locs, q = rng.random((400, 2)), rng.random((50, 2))
    el = np.arange(400) % 3 != 0
    _same(locs, q, 15, eligible=el)
    assert not np.isin(S.find_query_nn(locs, q, 15, eligible=el), np.nonzero(~el)[0] + 1).any()
    locs[7, 1], locs[9, 0], q[3, 0], q[4, 1] = np.nan, np.inf, np.nan, -np.inf
    got = S.find_query_nn(locs, q, 15)
    _same(locs, q, 15)
    assert (got[3] == 0).all() and (got[4] == 0).all() and not np.isin(got, [8, 10]).any()
