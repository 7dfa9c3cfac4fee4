"""covmodel='matern_scaledim' (one range per coordinate) without a GPU.

  the derivative formulas of tests/_scaledim_truth.py (those of gpv_grad.hip, grad_dcov_scaled) against
      - extended-precision central differences of the truth likelihood, to 2e-11 relative,
      - the dense multivariate normal at m = n - 1,
      - the isotropic truth (tests/_grad_truth.py): at equal ranges the range derivatives sum to the isotropic one;
  the argument checks that need no device: gpv_U_NZentries parses the family before it touches one, and the Python layer refuses
      what the gradient entries refuse (with a plan in hand those are checked in tests/test_gpu_scaledim_grad.py);
  vecchia_specify(scale=...) against vecchia_specify on pre-scaled locations.

The central differences: numpy.longdouble totals at theta_i (1 +- h) and (1 +- 2h), h = 1e-4, combined by Richardson's rule
(4 D(h) - D(2h)) / 3.  Its truncation error is of order h^4 = 1e-16 relative; its rounding error is about
eps_ld |l| / (h theta |dl/dtheta|), which the cases below keep under 1e-12 (|l| is a few hundred, the scaled derivatives are of
order one or more)."""
import ctypes as C

import numpy as np
import pytest

import _grad_truth as T
import _scaledim_truth as S

TAU = 0.1
NUS = (0.5, 1.5, 2.5)
RANGES = {1: [0.07], 2: [0.05, 0.4], 3: [0.3, 0.06, 0.15]}


def _rev_nn(locs, m):
    from oracle import r_side as R
    return np.nan_to_num(R.findOrderedNN(locs, m)[:, ::-1], nan=0.0).astype(np.int64)


def _cp(dim, nu, ranges=None):
    return [1.3] + list(RANGES[dim] if ranges is None else ranges) + [nu]


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("dim", (1, 2, 3))
def test_formulas_equal_extended_precision_central_differences(dim, nu):
    rng = np.random.default_rng(20 + dim)
    n, m = 60, 8
    locs, z = rng.random((n, dim)), rng.standard_normal(n)
    revNN = _rev_nn(locs / np.array(RANGES[dim]), m)
    cp = _cp(dim, nu)
    f64 = S.rows_f64(locs, revNN, z, cp, TAU)
    ld = np.stack([S.row_ld(locs, revNN[k], z, cp, TAU) for k in range(n)])
    assert T.scaled_row_error(f64, ld.astype(np.float64)).max() <= 2e-12      # float64 restatement against the adjudicator
    tot = ld.sum(axis=0)
    assert np.isnan(tot[dim + 2]) and not np.any(np.isnan(np.delete(tot, dim + 2)))
    theta = [np.longdouble(v) for v in cp[:-1]] + [np.longdouble(TAU)]          # variance, ranges, nugget
    col = list(range(1, dim + 2)) + [dim + 3]
    for i in range(len(theta)):
        def central(step):
            val = []
            for sgn in (1, -1):
                th = list(theta)
                th[i] = th[i] + sgn * step
                val.append(S.total_ld(locs, revNN, z, th[:-1] + [nu], th[-1])[0])
            return (val[0] - val[1]) / (2 * step)
        h = np.longdouble(1e-4) * theta[i]
        cd = (4 * central(h) - central(2 * h)) / 3
        rel = abs(cd - tot[col[i]]) / abs(tot[col[i]])
        print(f"dim {dim} nu {nu} parameter {i}: analytic {float(tot[col[i]]):.12e}, central differences off by {float(rel):.2e}")
        assert rel <= 2e-11, (i, float(cd), float(tot[col[i]]))


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("dim", (1, 2, 3))
def test_truth_equals_dense_mvn_at_full_conditioning(dim, nu):
    rng = np.random.default_rng(1)
    n = 40
    locs, z = rng.random((n, dim)), rng.standard_normal(n)
    cp = _cp(dim, nu)
    rows = S.rows_f64(locs, _rev_nn(locs, n - 1), z, cp, TAU)
    ll, g = S.dense_mvn(locs, z, cp, TAU)
    tot, scale = rows.sum(axis=0), np.abs(rows).sum(axis=0)
    keep = ~np.isnan(g)
    assert np.array_equal(np.isnan(tot[1:]), ~keep) and keep.sum() == dim + 2
    assert abs(tot[0] - ll) <= 1e-12 * scale[0]
    assert np.all(np.abs(tot[1:] - g)[keep] <= 1e-12 * scale[1:][keep])


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("dim", (1, 2, 3))
def test_equal_ranges_sum_to_the_isotropic_range_derivative(dim, nu):
    rng = np.random.default_rng(3)
    n, m, r = 80, 9, 0.2
    locs, z = rng.random((n, dim)), rng.standard_normal(n)
    locs[5] = locs[2]                                         # a coincident pair: the 0 / 0 of nu = 0.5
    revNN = _rev_nn(locs, m)
    sd = S.rows_f64(locs, revNN, z, _cp(dim, nu, [r] * dim), TAU)
    iso = T.rows_f64(locs, revNN, z, "matern", [1.3, r, nu], TAU)
    assert np.all(np.isfinite(np.delete(sd, dim + 2, axis=1)))
    scale = np.maximum(np.abs(iso[:, :3]).max(axis=1), 1.0)
    assert np.all(np.abs(sd[:, 0] - iso[:, 0]) <= 1e-12 * scale)                        # the value
    assert np.all(np.abs(sd[:, 1] - iso[:, 1]) <= 1e-12 * scale)                        # d / d variance
    assert np.all(np.abs(sd[:, 2:2 + dim].sum(axis=1) - iso[:, 2]) <= 1e-12 * scale)    # sum_t d / d range_t
    assert np.all(np.abs(sd[:, dim + 3] - iso[:, 4]) <= 1e-12 * scale)                  # d / d nugget


def _u_nzentries_status(dim, covparms, covtype=b"matern_scaledim"):
    """gpv_U_NZentries parses covType / covparms before anything else (no device is touched on an error)"""
    from gpvecchia_amd import _lib
    n, p = 4, 2
    locs = np.asfortranarray(np.random.default_rng(0).random((n, dim)))
    nn = np.asfortranarray(np.array([[0, 1], [1, 2], [2, 3], [3, 4]], dtype=np.int32))
    cd = np.asfortranarray(np.ones((n, p), dtype=np.int32))
    nug = np.full(n, 0.1)
    cp = np.ascontiguousarray(covparms, dtype=np.float64)
    Lent, Z = np.zeros((n, p), order="F"), np.zeros(2 * n)
    ci = lambda v: C.byref(C.c_int(int(v)))                                             # noqa: E731
    nfail, status = C.c_int(0), C.c_int(-1)
    ct = C.c_char_p(covtype)
    _lib.lib().gpv_U_NZentries(ci(1), ci(n), ci(n), ci(dim), ci(p), _lib.dptr(locs), _lib.iptr(nn), _lib.iptr(cd), _lib.dptr(nug),
                               _lib.dptr(nug), C.byref(ct), _lib.dptr(cp), ci(cp.size), _lib.dptr(Lent), _lib.dptr(Z),
                               C.byref(nfail), C.byref(status))
    return status.value


def test_argument_checks_before_the_device():
    BAD_ARG, NU, COVTYPE = 2, 4, 3
    assert _u_nzentries_status(2, [1.0, 0.1, 1.5]) == BAD_ARG                   # ncovparms = 3, dim + 2 = 4: matern's count
    assert _u_nzentries_status(2, [1.0, 0.1, 0.2, 0.3, 1.5]) == BAD_ARG         # one range too many
    assert _u_nzentries_status(1, [1.0, 0.1, 0.2, 1.5]) == BAD_ARG
    assert _u_nzentries_status(2, [1.0, 0.1, 0.0, 1.5]) == BAD_ARG              # a range of 0
    assert _u_nzentries_status(2, [1.0, -0.1, 0.2, 1.5]) == BAD_ARG             # a negative one
    assert _u_nzentries_status(2, [1.0, 0.1, np.inf, 1.5]) == BAD_ARG           # an infinite one
    assert _u_nzentries_status(9, [1.0] + [0.1] * 9 + [1.5]) == BAD_ARG         # more inverse ranges than a launch carries
    assert _u_nzentries_status(2, [1.0, 0.1, 0.2, 0.0]) == NU
    assert _u_nzentries_status(2, [1.0, 0.1, 0.2, 61.0]) == NU
    assert _u_nzentries_status(2, [1.0, 0.1, 0.2, 1.5], b"matern_scaled") == COVTYPE
    from gpvecchia_amd import _lib
    _lib.lib().gpv_status_string.restype = C.c_char_p
    assert b"matern_scaledim" in _lib.lib().gpv_status_string(COVTYPE)


def test_null_plan_is_a_bad_argument():
    from gpvecchia_amd import _lib
    cp, grad = np.array([1.0, 0.1, 0.2, 1.5]), np.zeros(5)
    ll, nf = C.c_double(), C.c_int64()
    st = _lib.lib().gpv_plan_loglik_grad(None, b"matern_scaledim", _lib.dptr(cp), 4, 0.1, C.byref(ll), _lib.dptr(grad), C.byref(nf),
                                         None)
    assert st == 2


def test_python_layer_refuses_what_the_gradient_entries_refuse():
    import gpvecchia_amd as G
    rng = np.random.default_rng(0)
    z = rng.standard_normal(60)
    l2, l4 = rng.random((60, 2)), rng.random((60, 4))
    va2 = G.vecchia_specify(l2, 5, ordering="none", cond_yz="z", nn_backend="host")
    va4 = G.vecchia_specify(l4, 5, ordering="none", cond_yz="z", nn_backend="host")
    fns = (G.vecchia_likelihood_grad, G.vecchia_likelihood_fisher, G.vecchia_likelihood_grad_replicates,
           G.vecchia_likelihood_fisher_replicates)
    for fn in fns:
        with pytest.raises(ValueError, match="three coordinates"):                  # dim > 3
            fn(z, va4, [1.0, 0.1, 0.2, 0.3, 0.4, 1.5], TAU, covmodel="matern_scaledim")
        with pytest.raises(ValueError, match="smoothness"):                         # another smoothness
            fn(z, va2, [1.0, 0.1, 0.2, 0.8], TAU, covmodel="matern_scaledim")
        with pytest.raises(ValueError, match="covparms"):                           # wrong count
            fn(z, va2, [1.0, 0.1, 1.5], TAU, covmodel="matern_scaledim")
        with pytest.raises(ValueError, match="positive"):                           # non-positive range
            fn(z, va2, [1.0, 0.1, 0.0, 1.5], TAU, covmodel="matern_scaledim")
    kw = dict(m=5, cond_yz="z", output_level=0, covmodel="matern_scaledim")
    for method in ("L-BFGS-B", "fisher"):
        with pytest.raises(ValueError, match="smoothness"):
            G.vecchia_estimate(z, l2, method=method, **kw)
        with pytest.raises(ValueError, match="smoothness"):
            G.vecchia_estimate(z, l2, method=method, smoothness=0.8, **kw)
        with pytest.raises(ValueError, match="three coordinates"):
            G.vecchia_estimate(z, l4, method=method, smoothness=1.5, **kw)
    with pytest.raises(ValueError, match="reneighbor"):
        G.vecchia_estimate(z, l2, m=5, cond_yz="z", output_level=0, reneighbor=True)
    with pytest.raises(ValueError, match="scale"):
        G.vecchia_specify(l2, 5, scale=[1.0, 0.0], nn_backend="host")
    with pytest.raises(ValueError, match="scale"):
        G.vecchia_specify(l2, 5, scale=[1.0], nn_backend="host")


@pytest.mark.parametrize("kw", [dict(ordering="maxmin", cond_yz="SGV"), dict(ordering="coord", cond_yz="z"),
                                dict(ordering="maxmin", cond_yz="zy"), dict(ordering="maxmin", pred=True)],
                         ids=["maxmin-SGV", "coord-z", "maxmin-zy", "maxmin-pred"])
def test_specify_scale_equals_specify_on_prescaled_locations(kw):
    import gpvecchia_amd as G
    kw = dict(kw)
    rng = np.random.default_rng(4)
    locs = rng.random((150, 2))
    pred = rng.random((20, 2)) if kw.pop("pred", False) else None
    sc = np.array([0.05, 2.5])                                                         # 1 : 50
    a = G.vecchia_specify(locs, 7, locs_pred=pred, nn_backend="host", scale=sc, **kw)
    b = G.vecchia_specify(locs / sc, 7, locs_pred=None if pred is None else pred / sc, nn_backend="host", **kw)
    c = G.vecchia_specify(locs, 7, locs_pred=pred, nn_backend="host", **kw)
    assert np.array_equal(a["ord"], b["ord"]) and np.array_equal(a["ord_z"], b["ord_z"]) and np.array_equal(a["obs"], b["obs"])
    for key in ("revNNarray", "revCond", "rowpointers", "colindices"):
        assert np.array_equal(a["U_prep"][key], b["U_prep"][key]), key
    assert not np.array_equal(a["U_prep"]["revNNarray"], c["U_prep"]["revNNarray"])     # the scale matters for these points
    # locsord keeps the true coordinates, bit for bit: every row is a row of the input
    allp = locs if pred is None else np.vstack([locs, pred])
    assert a["locsord"].shape == b["locsord"].shape
    rows = {r.tobytes() for r in allp}
    assert all(r.tobytes() in rows for r in a["locsord"])
    assert np.allclose(a["locsord"] / sc, b["locsord"], rtol=1e-15, atol=0)
    # scale=None is the specification it always was
    d = G.vecchia_specify(locs, 7, locs_pred=pred, nn_backend="host", scale=None, **kw)
    assert np.array_equal(d["ord"], c["ord"]) and np.array_equal(d["locsord"], c["locsord"])
    assert np.array_equal(d["U_prep"]["revNNarray"], c["U_prep"]["revNNarray"])
    assert np.array_equal(d["U_prep"]["revCond"], c["U_prep"]["revCond"])
