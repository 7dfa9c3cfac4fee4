"""The yardstick of tests/test_gpu_loglik_grad_sgv.py kept honest, without a GPU: the dense restatement of the SGV gradient
(tests/_sgv_grad_truth.py) against long-double central differences of its own value, against the dense multivariate normal at
m = n - 1, against the 'z' restatement (tests/_grad_truth.py) on a cond 'z' plan, and float64 against long double on every case
the GPU tests run; then the export and the refusals of the Python layer that need no device."""
import ctypes as C

import numpy as np
import pytest

import _grad_truth as T
import _sgv_grad_cases as K
import _sgv_grad_truth as S

TAU = K.TAU
BAR = 1e-8                                                  # the bar of the GPU tests; the float64 truth may use 1e-4 of it


def _rel(got, want, scale):
    got, want, scale = (np.asarray(a, dtype=np.longdouble) for a in (got, want, scale))
    keep = ~np.isnan(want.reshape(-1, want.shape[-1])[0])
    return float((np.abs(got[..., keep] - want[..., keep]) / np.maximum(scale[..., keep], 1)).max())


@pytest.mark.parametrize("fam", K.FAMILIES)
def test_truth_against_long_double_central_differences(fam):
    """n = 120, m = 8: the differences' own truncation at h = 1e-5 theta is below 1e-10 relative (measured: 3e-11 .. 9e-11)"""
    m, d, n = 8, 2, 120
    locs, z, va = K.setup(m, d, n=n)
    cm, cp = K.family(fam, d)
    nn, rc = va["U_prep"]["revNNarray"], va["U_prep"]["revCond"]
    t = S.sgv_truth(va["locsord"], nn, rc, z, cm, cp, TAU, np.longdouble)
    slots = np.where(~np.isnan(t["grad"].astype(np.float64)))[0]
    theta = np.array([v for i, v in enumerate(cp) if not (cm == "matern" and i == 2)] + [TAU], dtype=np.longdouble)
    for i, slot in enumerate(slots):
        h = np.longdouble(1e-5) * theta[i]
        vals = []
        for sgn in (1, -1):
            th = theta.copy()
            th[i] += sgn * h
            cpi = list(th[:-1]) if cm == "esqe" else [th[0], th[1], cp[2]]
            vals.append(S.sgv_value(va["locsord"], nn, rc, z, cm, cpi, th[-1], np.longdouble))
        cd = (vals[0] - vals[1]) / (2 * h)
        rel = float(abs(cd - t["grad"][slot]) / abs(cd))
        print(fam, "parameter", i, "analytic", float(t["grad"][slot]), "central difference", float(cd), "relative", rel)
        assert rel <= 1e-9


@pytest.mark.parametrize("fam", ("nu0.5", "nu1.5", "nu2.5", "esqe"))
def test_truth_equals_dense_mvn_at_full_conditioning(fam):
    n = 60
    locs, z, va = K.setup(n - 1, 2, n=n)
    cm, cp = K.family(fam, 2)
    t = K.truth(n - 1, 2, fam, n=n)
    ll_d, g_d = T.dense_mvn(locs, z, cm, cp, TAU)
    off = _rel(t["grad"], g_d, t["scale"].sum(axis=0))
    print(fam, "value", abs(t["loglik"] - ll_d) / abs(ll_d), "gradient, of the scale", off)
    assert abs(t["loglik"] - ll_d) <= 1e-12 * abs(ll_d) and off <= 1e-12


@pytest.mark.parametrize("fam", ("nu1.5", "esqe"))
def test_truth_equals_the_z_restatement_on_a_z_plan(fam):
    m, d = 10, 2
    locs, z, va = K.setup(m, d, cond="z")
    cm, cp = K.family(fam, d)
    t = K.truth(m, d, fam, cond="z")
    rows = T.rows_f64(va["locsord"], va["U_prep"]["revNNarray"], z, cm, cp, TAU)
    off = _rel(t["col_terms"], rows[:, 1:], t["scale"])
    tot = _rel(t["grad"], rows[:, 1:].sum(axis=0), t["scale"].sum(axis=0))
    print(fam, "columns", off, "totals", tot, "value", abs(t["loglik"] - rows[:, 0].sum()) / abs(t["loglik"]))
    assert off <= 1e-12 and tot <= 1e-12 and abs(t["loglik"] - rows[:, 0].sum()) <= 1e-12 * abs(t["loglik"])


_GPU_CASES = [(m, d, fam, K.N, "SGV") for (m, d) in K.SHAPES for fam in K.FAMILIES] + \
             [(10, 2, fam, K.N, "z") for fam in ("nu1.5", "esqe")] + [(59, 2, fam, 60, "SGV") for fam in ("nu1.5", "esqe")]


@pytest.mark.parametrize("m,d,fam,n,cond", _GPU_CASES, ids=["m%d-d%d-%s-n%d-%s" % c for c in _GPU_CASES])
def test_float64_truth_against_long_double_on_the_gpu_cases(m, d, fam, n, cond):
    """the float64 restatement uses at most 1e-4 of the bar on the inputs the GPU tests adjudicate with it"""
    t64 = K.truth(m, d, fam, n=n, cond=cond)
    tld = K.truth(m, d, fam, n=n, cond=cond, dtype="longdouble")
    col = _rel(t64["col_terms"], tld["col_terms"], tld["scale"])
    tot = _rel(t64["grad"], tld["grad"], tld["scale"].sum(axis=0))
    val = float(abs(t64["loglik"] - tld["loglik"]) / abs(tld["loglik"]))
    print(f"columns {col:.2e} totals {tot:.2e} value {val:.2e}")
    assert max(col, tot, val) <= 1e-4 * BAR


def test_symbol_is_exported_and_null_plan_is_a_bad_argument():
    from gpvecchia_amd import _lib
    assert "gpv_plan_loglik_grad_sgv" in _lib.EXPORTS
    cp, grad = np.array([1.0, 0.1, 1.5]), np.zeros(4)
    ll, nf = C.c_double(), C.c_int64()
    st = _lib.lib().gpv_plan_loglik_grad_sgv(None, b"matern", _lib.dptr(cp), 3, 0.1, C.byref(ll), _lib.dptr(grad), C.byref(nf), None)
    assert st == 2                                            # GPV_ERR_BAD_ARG


def test_python_layer_refusals():
    import gpvecchia_amd as G
    rng = np.random.default_rng(0)
    locs, z = rng.random((60, 2)), rng.standard_normal(60)
    cp = [1.0, 0.2, 1.5]
    va = G.vecchia_specify(locs, 5, ordering="none", cond_yz="SGV", nn_backend="host")
    va_y = G.vecchia_specify(locs, 5, ordering="none", cond_yz="y", nn_backend="host")
    with pytest.raises(ValueError, match="cond_yz"):
        G.vecchia_likelihood_grad_sgv(z, va_y, cp, TAU)
    with pytest.raises(ValueError, match="constant nugget"):
        G.vecchia_likelihood_grad_sgv(z, va, cp, np.full(60, TAU))
    zn = z.copy()
    zn[7] = np.nan
    with pytest.raises(ValueError, match="complete data"):
        G.vecchia_likelihood_grad_sgv(zn, va, cp, TAU)
    va_pred = dict(va)
    va_pred["obs"] = np.concatenate([np.ones(50, bool), np.zeros(10, bool)])
    with pytest.raises(ValueError, match="prediction"):
        G.vecchia_likelihood_grad_sgv(z, va_pred, cp, TAU)
    for cm in (lambda dd: np.exp(-dd), np.eye(60), "matern_scaledim"):
        with pytest.raises(ValueError, match="named covariance"):
            G.vecchia_likelihood_grad_sgv(z, va, cp, TAU, covmodel=cm)
    # what stays as it was: the 'z' gradient refuses SGV plans, L-BFGS-B without an explicit cond_yz and Fisher scoring with SGV raise
    with pytest.raises(ValueError, match="needs cond_yz='z'"):
        G.vecchia_likelihood_grad(z, va, cp, TAU)
    with pytest.raises(ValueError, match="cond_yz"):
        G.vecchia_estimate(z, locs, m=5, method="L-BFGS-B", smoothness=1.5, output_level=0)
    with pytest.raises(ValueError, match="cond_yz"):
        G.vecchia_estimate(z, locs, m=5, method="fisher", smoothness=1.5, cond_yz="SGV", output_level=0)
    with pytest.raises(ValueError, match="cond_yz"):
        G.vecchia_estimate(z, locs, m=5, method="L-BFGS-B", smoothness=1.5, cond_yz="SGV", trend="gls", output_level=0)
    with pytest.raises(ValueError, match="cond_yz"):
        G.vecchia_estimate(np.stack([z, z], axis=1), locs, m=5, method="L-BFGS-B", smoothness=1.5, cond_yz="SGV", output_level=0)
    with pytest.raises(ValueError, match="SGV"):
        G.vecchia_estimate(z, locs, m=5, method="L-BFGS-B", cond_yz="SGV", smoothness_grad=True, output_level=0)
    with pytest.raises(ValueError, match="smoothness"):
        G.vecchia_estimate(z, locs, m=5, method="L-BFGS-B", cond_yz="SGV", smoothness=0.8, output_level=0)
