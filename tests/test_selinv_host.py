"""gpv_plan_selinv without a GPU: the export, the truth of the GPU tests (tests/_selinv_truth.py) against np.linalg.inv, where the
recursion on the factor's own pattern is exact and where it is not (the oracle's chain, n = 300, m = 8, Matern 1.5, vector
nuggets), and the Python layer's refusals.

EXACT = 1e-10 relative to max(1, max|ref|): W = U_y U_y^T of these plans has a condition number below 1e5, so both the inverse
and the recursion carry errors of at most ~1e5 * 2^-53 ~ 1e-11; measured 4e-14 to 8e-14."""
import numpy as np
import pytest

import _selinv_truth as T

EXACT = 1e-10


def _rel(got, ref):
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


def _oracle_case(cond_yz, n=300, m=8, n_p=0, ordering_pred=None, seed=5):
    from oracle import r_side as R
    rng = np.random.default_rng(seed)
    locs = rng.random((n, 2))
    lp = rng.random((n_p, 2)) if n_p else None
    tau = 0.05 + 0.1 * rng.random(n)
    va = R.vecchia_specify(locs, m, ordering="maxmin", cond_yz=cond_yz, locs_pred=lp, ordering_pred=ordering_pred)
    Uo = R.createU(va, [1.0, 0.15, 1.5], tau)
    lat = np.asarray(Uo["latent"], dtype=bool)
    Uy = Uo["U"][lat, :]
    return Uo, Uy @ Uy.T


def test_symbol_is_exported_and_python_names_exist():
    from gpvecchia_amd import _lib
    import gpvecchia_amd as G
    from gpvecchia_amd import lincomb as LC
    assert "gpv_plan_selinv" in _lib.EXPORTS
    assert getattr(_lib.lib(), "gpv_plan_selinv") is not None
    assert callable(G.Plan.selinv) and callable(LC.selected_variances_device) and callable(G.vecchia_selinv)


def test_truth_equals_the_inverse_on_a_full_pattern():
    rng = np.random.default_rng(1)
    n = 40
    A = rng.standard_normal((n, n))
    W = A @ A.T + n * np.eye(n)
    R = T.ul_cholesky(W)
    assert np.allclose(R @ R.T, W, rtol=0, atol=1e-10) and np.all(np.tril(R, -1) == 0)
    d, dropped = T.selinv_truth(R, np.ones((n, n), dtype=bool))
    ref = np.diag(np.linalg.inv(W))
    print("full pattern: rel", _rel(d, ref))
    assert dropped == 0 and _rel(d, ref) <= EXACT
    # a diagonal factor: var = 1 / R_kk^2
    D = np.diag(1.0 + rng.random(n))
    d, dropped = T.selinv_truth(D, np.eye(n, dtype=bool))
    assert dropped == 0 and np.array_equal(d, 1.0 / np.diag(D) ** 2)


def test_sgv_fully_observed_is_exact():
    Uo, W = _oracle_case("SGV")
    R, pattern = T.latent_factor(Uo)
    assert np.all(R[~np.triu(pattern)] == 0) or np.abs(R[~np.triu(pattern)]).max() < 1e-12      # SGV: no fill
    d, dropped = T.selinv_truth(R, pattern)
    ref = np.diag(np.linalg.inv(W))
    print("SGV fully observed: dropped", dropped, "rel", _rel(d, ref))
    assert dropped == 0 and _rel(d, ref) <= EXACT


def test_y_on_the_filled_pattern_is_exact():
    Uo, W = _oracle_case("y")
    R, pattern = T.latent_factor(Uo)
    pb = np.triu(pattern).astype(np.int64)
    filled = T.filled_pattern((pb @ pb.T) > 0)
    assert filled.sum() > np.triu(pattern).sum()                         # there IS fill
    assert np.abs(R[~filled]).max() < 1e-12                              # and the factor lives on the filled pattern
    d, dropped = T.selinv_truth(R, filled)
    ref = np.diag(np.linalg.inv(W))
    print("y, filled: entries", int(filled.sum()), "of B", int(np.triu(pattern).sum()), "dropped", dropped, "rel", _rel(d, ref))
    assert dropped == 0 and _rel(d, ref) <= EXACT
    # on B's own pattern the same factor drops pairs
    assert T.selinv_truth(R, pattern)[1] > 0


def test_sgv_prediction_plan_drops_pairs_and_is_approximate():
    """The conditioning sets of prediction locations are no cliques: pairs are dropped, the diagonal is the reference's
    var.exact = FALSE approximation (the issue measured 212 dropped pairs and 12 % at its seed)."""
    Uo, W = _oracle_case("SGV", n_p=80, ordering_pred="obspred")
    R, pattern = T.latent_factor(Uo)
    assert np.abs(R[~np.triu(pattern)]).max() < 1e-12                    # obs-pred SGV: the factor has no fill
    d, dropped = T.selinv_truth(R, pattern)
    ref = np.diag(np.linalg.inv(W))
    rel = np.abs(d - ref) / ref
    print("SGV + 80 prediction locations: dropped", dropped, "max rel error of diag", rel.max())
    assert dropped > 0 and rel.max() > 1e-6
    assert np.all(d > 0)


def test_python_refusals():
    import gpvecchia_amd as G
    for bad in ({}, dict(mu_obs=np.zeros(3)), None):
        with pytest.raises(ValueError, match="meanmat"):
            G.vecchia_selinv(bad)
    with pytest.raises(ValueError, match="host route"):
        G.vecchia_selinv(dict(factor=dict(kind="host", U_obj=None, lu=None)))
