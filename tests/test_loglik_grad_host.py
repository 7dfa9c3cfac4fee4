"""gpv_plan_loglik_grad without a GPU: the export, the argument checks that come before the device is touched, the
ValueErrors of the Python layer, and the truth helper of the GPU tests (tests/_grad_truth.py) against two independent
statements of the same gradient: the dense multivariate normal at m = n - 1 and extended-precision central differences."""
import ctypes as C

import numpy as np
import pytest

import _grad_truth as T

TAU = 0.1
CASES = {"nu0.5": ("matern", [1.3, 0.25, 0.5]), "nu1.5": ("matern", [1.3, 0.25, 1.5]), "nu2.5": ("matern", [1.3, 0.25, 2.5]),
         "esqe": ("esqe", [0.8, 0.25, 0.5, 0.2])}


def _rev_nn(locs, m):
    from oracle import r_side as R
    return np.nan_to_num(R.findOrderedNN(locs, m)[:, ::-1], nan=0.0).astype(np.int64)


def test_symbol_is_exported():
    from gpvecchia_amd import _lib
    assert "gpv_plan_loglik_grad" in _lib.EXPORTS
    assert getattr(_lib.lib(), "gpv_plan_loglik_grad") is not None


def test_null_plan_is_a_bad_argument():
    from gpvecchia_amd import _lib
    cp, grad = np.array([1.0, 0.1, 1.5]), np.zeros(4)
    ll, nf = C.c_double(), C.c_int64()
    st = _lib.lib().gpv_plan_loglik_grad(None, b"matern", _lib.dptr(cp), 3, 0.1, C.byref(ll), _lib.dptr(grad), C.byref(nf), None)
    assert st == 2                                            # GPV_ERR_BAD_ARG


def test_python_layer_refuses_what_has_no_gradient():
    import gpvecchia_amd as G
    rng = np.random.default_rng(0)
    locs, z = rng.random((60, 2)), rng.standard_normal(60)
    cp = [1.0, 0.2, 1.5]
    va_z = G.vecchia_specify(locs, 5, ordering="none", cond_yz="z", nn_backend="host")
    va_sgv = G.vecchia_specify(locs, 5, ordering="none", cond_yz="SGV", nn_backend="host")
    with pytest.raises(ValueError, match="cond_yz"):
        G.vecchia_likelihood_grad(z, va_sgv, cp, TAU)
    with pytest.raises(ValueError, match="constant nugget"):
        G.vecchia_likelihood_grad(z, va_z, cp, np.full(60, TAU))
    zn = z.copy()
    zn[7] = np.nan
    with pytest.raises(ValueError, match="complete data"):
        G.vecchia_likelihood_grad(zn, va_z, cp, TAU)
    va_pred = dict(va_z)
    va_pred["obs"] = np.concatenate([np.ones(50, bool), np.zeros(10, bool)])
    with pytest.raises(ValueError, match="prediction"):
        G.vecchia_likelihood_grad(z, va_pred, cp, TAU)
    with pytest.raises(ValueError, match="named covariance"):
        G.vecchia_likelihood_grad(z, va_z, cp, TAU, covmodel=lambda d: np.exp(-d))
    with pytest.raises(ValueError, match="named covariance"):
        G.vecchia_likelihood_grad(z, va_z, cp, TAU, covmodel=np.eye(60))
    # the estimation driver: L-BFGS-B needs a fixed closed-form smoothness and cond_yz='z'
    with pytest.raises(ValueError, match="smoothness"):
        G.vecchia_estimate(z, locs, m=5, method="L-BFGS-B", cond_yz="z", output_level=0)
    with pytest.raises(ValueError, match="smoothness"):
        G.vecchia_estimate(z, locs, m=5, method="L-BFGS-B", smoothness=0.8, cond_yz="z", output_level=0)
    with pytest.raises(ValueError, match="cond_yz"):
        G.vecchia_estimate(z, locs, m=5, method="L-BFGS-B", smoothness=1.5, output_level=0)
    with pytest.raises(ValueError, match="not defined"):
        G.vecchia_estimate(z, locs, m=5, method="BFGS", output_level=0)


@pytest.mark.parametrize("fam", sorted(CASES))
def test_truth_equals_dense_mvn_at_full_conditioning(fam):
    cm, cp = CASES[fam]
    rng = np.random.default_rng(1)
    n = 40
    locs, z = rng.random((n, 2)), rng.standard_normal(n)
    rows = T.rows_f64(locs, _rev_nn(locs, n - 1), z, cm, cp, TAU)
    ll, g = T.dense_mvn(locs, z, cm, cp, TAU)
    tot, scale = rows.sum(axis=0), np.abs(rows).sum(axis=0)
    keep = ~np.isnan(g)
    assert np.array_equal(np.isnan(tot[1:]), ~keep)
    assert abs(tot[0] - ll) <= 1e-12 * scale[0]
    assert np.all(np.abs(tot[1:] - g)[keep] <= 1e-12 * scale[1:][keep])


@pytest.mark.parametrize("fam", sorted(CASES))
def test_truth_equals_its_extended_precision_central_differences(fam):
    cm, cp = CASES[fam]
    rng = np.random.default_rng(2)
    n, m = 120, 10
    locs, z = rng.random((n, 2)), rng.standard_normal(n)
    revNN = _rev_nn(locs, m)
    f64 = T.rows_f64(locs, revNN, z, cm, cp, TAU)
    ld = np.stack([T.row_ld(locs, revNN[k], z, cm, cp, TAU) for k in range(n)])
    assert T.scaled_row_error(f64, ld.astype(np.float64)).max() <= 2e-12      # float64 restatement against the adjudicator
    tot = ld.sum(axis=0)
    theta = [np.longdouble(v) for v in cp] + [np.longdouble(TAU)]
    for i in range(len(theta)):
        if cm == "matern" and i == 2:
            assert np.isnan(tot[1 + i])
            continue
        h = np.longdouble(1e-6) * theta[i]
        val = []
        for sgn in (1, -1):
            th = list(theta)
            th[i] = th[i] + sgn * h
            c = th[:-1]
            if cm == "matern":
                c[2] = cp[2]
            val.append(T.total_ld(locs, revNN, z, cm, c, th[-1])[0])
        cd = (val[0] - val[1]) / (2 * h)
        assert abs(cd - tot[1 + i]) <= 1e-9 * abs(tot[1 + i]), (i, float(cd), float(tot[1 + i]))
