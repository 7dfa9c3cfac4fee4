"""The truth of the grouped-kriging tests (tests/_krige_groups_truth.py) proves itself on the CPU, and the Python layer of
vecchia_krige_groups refuses what it must before any device is touched.

  * the chain rule: appending a group to a cond.yz='z' plan as its last rows, member i conditioning on J and on the members
    before it, adds exactly log N(z_G; mean_G, Sigma_G + diag tau_G) to the oracle's likelihood;
  * with m = n the group IS the dense GP conditional, and a group of one is the per-location truth (tests/_krige_truth.py);
  * the anchor arithmetic: the members summed in order in float64, then one division;
  * the refusals of the Python layer.
"""
import numpy as np
import pytest

import _krige_groups_truth as GT
import _krige_truth as KT

FAMILIES = [("matern", [1.3, 0.25, 1.5]), ("matern", [1.3, 0.25, 0.8]), ("esqe", [1.0, 0.3, 0.5, 0.2]),
            ("matern_scaledim", [1.3, 0.2, 0.4, 2.5])]


@pytest.mark.parametrize("covmodel,cp", FAMILIES)
def test_chain_rule_against_the_oracle(covmodel, cp):
    """loglik([z; z_G]) = loglik(z) + log N(z_G; mean_G, Sigma_G + diag tau_G) for the oracle's cond.yz='z' likelihood with the
    group as the LAST rows, each member conditioning on J and the members before it; groups inside, across the edge of and
    outside the observed region"""
    from oracle import r_side as R
    rng = np.random.default_rng(12)
    n, m = 60, 7
    locs, z = rng.random((n, 2)), rng.standard_normal(n)
    tau = 0.1
    if covmodel == "matern_scaledim":                    # the oracle's isotropic algorithm on locs / ranges at range 1
        sc = np.array(cp[1:3])
        ocov, ocp = "matern", [cp[0], 1.0, cp[3]]
    else:
        sc, ocov, ocp = np.ones(2), covmodel, cp
    NN0 = R.findOrderedNN(locs / sc, m)
    for centre, g in (([0.5, 0.5], 4), ([0.98, 0.3], 3), ([1.6, -0.3], 5), ([0.2, 0.7], 1)):
        xg = np.asarray(centre) + 0.05 * (rng.random((g, 2)) - 0.5)
        zg, taug = rng.standard_normal(g), 0.03 + 0.1 * rng.random(g)
        gptr = np.array([0, g])
        NN = GT.group_nn(locs, xg, gptr, m, scale=sc)
        t = GT.krige_groups_ld(locs, tau, z, xg, gptr, NN, covmodel, cp)[0]
        assert not t["failed"]
        width = m + g                                    # the row of the last member: itself, the members before it, J
        NNa = np.full((n + g, width), np.nan)
        NNa[:n, :m + 1] = NN0
        for i in range(g):
            row = [n + i + 1] + [n + j + 1 for j in range(i)] + list(NN[0][NN[0] > 0])
            NNa[n + i, :len(row)] = row
        va0 = R.vecchia_specify(locs / sc, m, ordering="none", cond_yz="z", NNarray=NNa[:n])
        va1 = R.vecchia_specify(np.vstack([locs, xg]) / sc, width - 1, ordering="none", cond_yz="z", NNarray=NNa)
        ll0 = R.vecchia_likelihood(z, va0, ocp, tau, ocov)
        ll1 = R.vecchia_likelihood(np.concatenate([z, zg]), va1, ocp, np.concatenate([np.full(n, tau), taug]), ocov)
        want = ll0 + GT.log_density_mv(zg, t["mean"][:, 0], t["cov"] + np.diag(taug))
        assert abs(ll1 - want) <= 1e-10 * abs(ll1), (centre, ll1, want)


@pytest.mark.parametrize("covmodel,cp", FAMILIES)
def test_m_equal_n_is_the_dense_conditional_and_g1_is_the_location(covmodel, cp):
    rng = np.random.default_rng(13)
    n, g = 40, 24
    locs, xg = rng.random((n, 2)), 0.4 + 0.2 * rng.random((g, 2))
    Z = rng.standard_normal((n, 3))
    tau = 0.05 + 0.1 * rng.random(n)
    gptr = np.array([0, g])
    t = GT.krige_groups_ld(locs, tau, Z, xg, gptr, GT.group_nn(locs, xg, gptr, n), covmodel, cp)[0]
    C = KT.cov_matrix(np.vstack([locs, xg]), covmodel, cp)
    K, k = C[:n, :n] + np.diag(tau), C[:n, n:]
    sol = np.linalg.solve(K, np.hstack([Z, k]))
    assert np.abs(t["mean"] - k.T @ sol[:, :3]).max() <= 1e-9 * np.abs(Z).max()
    assert np.abs(t["cov"] - (C[n:, n:] - k.T @ sol[:, 3:])).max() <= 1e-9 * cp[0]
    assert np.abs(t["cov"] - t["cov"].T).max() <= 1e-15 * cp[0]
    # groups of one: the per-location truth with the same neighbours
    g1 = np.arange(g + 1)
    NN = GT.group_nn(locs, xg, g1, 9)
    assert (NN == KT.query_nn(locs, xg, 9)).all()                    # the anchor of one member is the member
    one = GT.krige_groups_ld(locs, tau, Z, xg, g1, NN, covmodel, cp)
    mean, var, l1, failed = KT.krige_ld(locs, tau, Z, xg, NN, covmodel, cp)
    assert not failed.any()
    for i in range(g):
        assert np.abs(one[i]["mean"][0] - mean[i]).max() <= 1e-14 * l1[i] * np.abs(Z).max()
        assert abs(one[i]["cov"][0, 0] - var[i]) <= 1e-13 * var[i] and abs(one[i]["l1"][0] - l1[i]) <= 1e-13 * l1[i]


def test_truth_edges():
    """a member on an observation without a nugget fails its group alone; duplicates give equal rows and no failure; an
    empty neighbour list is the prior"""
    rng = np.random.default_rng(14)
    locs, Z = rng.random((50, 2)), rng.standard_normal((50, 2))
    x = np.vstack([locs[3], [0.5, 0.5], [0.31, 0.32], [0.31, 0.32], [0.3, 0.3]])
    gptr = np.array([0, 2, 5])
    NN = GT.group_nn(locs, x, gptr, 50)
    t = GT.krige_groups_ld(locs, 0.0, Z, x, gptr, NN, "matern", [1.0, 0.2, 1.5])
    assert t[0]["failed"] and np.isnan(t[0]["mean"]).all() and not t[1]["failed"]
    assert (t[1]["cov"][0] == t[1]["cov"][1]).all() and (t[1]["cov"][:, 0] == t[1]["cov"][:, 1]).all()
    e = GT.krige_groups_ld(locs, 0.1, Z, x[1:3], np.array([0, 2]), np.zeros((1, 4), dtype=np.int32), "matern", [1.7, 0.2, 1.5])[0]
    assert not e["failed"] and (e["mean"] == 0).all() and (e["l1"] == 0).all() and e["cov"][0, 0] == 1.7


def test_anchor_arithmetic():
    """s = x_0; s += x_i in member order; s / g: numbers whose sum depends on the order and on the rounding of every step"""
    x = np.array([[1e16, 0.1], [1.0, 0.2], [-1e16, 0.3], [1.0, 0.7], [3.0, 0.1 + 2 ** -52]])
    a = GT.anchors(x, np.array([0, 4, 5]))
    s0 = np.float64(1e16) + np.float64(1.0)                          # 1e16 + 1 rounds back to 1e16
    s0 = (s0 + np.float64(-1e16)) + np.float64(1.0)
    s1 = ((np.float64(0.1) + np.float64(0.2)) + np.float64(0.3)) + np.float64(0.7)
    assert a[0, 0] == s0 / 4.0 == 0.25 and a[0, 1] == s1 / 4.0
    assert (a[1] == x[4]).all()                                      # one member: the member itself, bit for bit
    # the search runs at the anchor
    rng = np.random.default_rng(15)
    locs, q = rng.random((200, 2)), rng.random((12, 2))
    gptr = np.array([0, 5, 6, 12])
    assert (GT.group_nn(locs, q, gptr, 8) == KT.query_nn(locs, GT.anchors(q, gptr), 8)).all()
    sc = np.array([0.1, 0.3])
    assert (GT.group_nn(locs, q, gptr, 8, scale=sc) == KT.query_nn(locs / sc, GT.anchors(q, gptr) / sc, 8)).all()


def _spec(n=30, m=5, cond_yz="z", seed=16):
    import gpvecchia_amd as G
    rng = np.random.default_rng(seed)
    locs = rng.random((n, 2))
    return G, G.vecchia_specify(locs, m, cond_yz=cond_yz), rng.standard_normal(n), rng.random((6, 2))


def test_python_layer_refusals():
    G, va, z, lp = _spec()
    lab = np.array([0, 0, 1, 1, 2, 2])
    cp = [1.0, 0.2, 1.5]
    with pytest.raises(ValueError, match="cond_yz='z'"):
        G.vecchia_krige_groups(z, _spec(cond_yz="SGV")[1], lp, lab, cp, 0.1)
    with pytest.raises(ValueError, match="one integer label"):
        G.vecchia_krige_groups(z, va, lp, lab[:5], cp, 0.1)
    with pytest.raises(ValueError, match="one integer label"):
        G.vecchia_krige_groups(z, va, lp, lab.astype(float), cp, 0.1)
    with pytest.raises(ValueError, match="finite"):
        G.vecchia_krige_groups(z, va, lp, lab, cp, 0.1, weights=[1, 1, 1, np.inf, 1, 1])
    with pytest.raises(ValueError, match="finite"):
        G.vecchia_krige_groups(z, va, lp, lab, cp, 0.1, weights=[1, 1, 1])
    with pytest.raises(ValueError, match="nugget_pred"):
        G.vecchia_krige_groups(z, va, lp, lab, cp, 0.1, predict="z")
    with pytest.raises(ValueError, match="predict must be"):
        G.vecchia_krige_groups(z, va, lp, lab, cp, 0.1, predict="w")
    with pytest.raises(ValueError, match="single column"):
        G.vecchia_krige_groups(np.where(np.arange(60).reshape(30, 2) == 4, np.nan, 1.0), va, lp, lab, cp, 0.1)
    with pytest.raises(ValueError, match="named covariance"):
        G.vecchia_krige_groups(z, va, lp, lab, cp, 0.1, covmodel=lambda d: d)
    with pytest.raises(ValueError, match="<= 64"):
        G.vecchia_krige_groups(z, va, np.random.default_rng(1).random((62, 2)), np.zeros(62, dtype=int), cp, 0.1, m=3)
    with pytest.raises(ValueError, match="local=True"):
        G.vecchia_pred(dict(theta_hat=[1.0, 0.2, 1.5, 0.1]), lp, groups=lab)
