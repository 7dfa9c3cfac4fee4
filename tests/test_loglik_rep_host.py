"""gpv_plan_loglik_rep (value, gradient and information summed over R replicates) without a GPU: the exports, the argument checks
that come before the device is touched, the ValueErrors of the Python layer, the form the kernel computes (u, y_p, Q2, QB_p: the
identity b = z'y the design rests on) against the column-summed truth of tests/_grad_truth.py / tests/_fisher_truth.py, and
vecchia_estimate with n x R data on stubbed likelihood functions."""
import ctypes as C

import numpy as np
import pytest

import _fisher_truth as F
import _grad_truth as T

TAU = 0.1
SYMBOLS = ("gpv_plan_set_replicates", "gpv_plan_replicates", "gpv_plan_loglik_rep", "gpv_plan_loglik_rep_nu")
# the formula against the definition, both in float64, scaled per row by max(|row|_inf, 1): the documented bar of the Fisher form
# is 2e-11; the replicate form adds dot products only
FORM_BAR = 1e-11


def _rev_nn(locs, m):
    from oracle import r_side as R
    return np.nan_to_num(R.findOrderedNN(locs, m)[:, ::-1], nan=0.0).astype(np.int64)


def test_symbols_are_exported():
    from gpvecchia_amd import _lib
    import gpvecchia_amd as G
    for s in SYMBOLS:
        assert s in _lib.EXPORTS
        assert getattr(_lib.lib(), s) is not None
    assert callable(G.vecchia_likelihood_grad_replicates) and callable(G.vecchia_likelihood_fisher_replicates)
    assert callable(G.Plan.set_replicates) and callable(G.Plan.loglik_replicates)


def test_bad_arguments_need_no_device():
    from gpvecchia_amd import _lib
    L = _lib.lib()
    Z = np.zeros((8, 2), order="F")
    cp, grad, info = np.array([1.0, 0.1, 1.5]), np.zeros(4), np.zeros(16)
    ll, nf, R = C.c_double(), C.c_int64(), C.c_int()
    assert L.gpv_plan_set_replicates(None, _lib.dptr(Z), 8, 2) == 2                  # GPV_ERR_BAD_ARG
    assert L.gpv_plan_set_replicates(None, None, 8, 2) == 2
    assert L.gpv_plan_set_replicates(None, _lib.dptr(Z), 8, -1) == 2             # R < 0
    assert L.gpv_plan_set_replicates(None, _lib.dptr(Z), 7, 2) == 2              # (on a plan: tests/sanitize/loglik_rep_driver.cpp
    #                                                                                and tests/test_gpu_loglik_rep.py)
    assert L.gpv_plan_replicates(None, C.byref(R)) == 2
    for fn in (L.gpv_plan_loglik_rep, L.gpv_plan_loglik_rep_nu):
        assert fn(None, b"matern", _lib.dptr(cp), 3, 0.1, C.byref(ll), _lib.dptr(grad), _lib.dptr(info), C.byref(nf), None) == 2
        assert fn(None, None, None, 3, 0.1, None, None, None, None, None) == 2


@pytest.mark.parametrize("fn", ["vecchia_likelihood_grad_replicates", "vecchia_likelihood_fisher_replicates"])
def test_python_layer_refusals(fn):
    import gpvecchia_amd as G
    call = getattr(G, fn)
    rng = np.random.default_rng(0)
    locs, Z = rng.random((60, 2)), rng.standard_normal((60, 3))
    cp = [1.0, 0.2, 1.5]
    va_z = G.vecchia_specify(locs, 5, ordering="none", cond_yz="z", nn_backend="host")
    va_sgv = G.vecchia_specify(locs, 5, ordering="none", cond_yz="SGV", nn_backend="host")
    Zn = Z.copy()
    Zn[7, 1] = np.nan
    with pytest.raises(ValueError, match="complete, finite"):
        call(Zn, va_z, cp, TAU)
    with pytest.raises(ValueError, match="one row per location"):
        call(Z[:-1], va_z, cp, TAU)
    with pytest.raises(ValueError, match=fn + " needs cond_yz"):
        call(Z, va_sgv, cp, TAU)
    va_pred = dict(va_z)
    va_pred["obs"] = np.concatenate([np.ones(50, bool), np.zeros(10, bool)])
    with pytest.raises(ValueError, match="prediction"):
        call(Z, va_pred, cp, TAU)
    with pytest.raises(ValueError, match="constant nugget"):
        call(Z, va_z, cp, np.full(60, TAU))
    with pytest.raises(ValueError, match="named covariance"):
        call(Z, va_z, cp, TAU, covmodel=lambda d: np.exp(-d))


def test_estimate_refuses_gls_with_replicates():
    import gpvecchia_amd as G
    rng = np.random.default_rng(0)
    locs, Z = rng.random((60, 2)), rng.standard_normal((60, 3))
    with pytest.raises(ValueError, match="trend='gls'.*replicated"):
        G.vecchia_estimate(Z, locs, m=5, trend="gls", cond_yz="z", smoothness=1.5, output_level=0)
    with pytest.raises(ValueError, match="replicated data.*cond_yz='z'"):
        G.vecchia_estimate(Z, locs, m=5, smoothness=1.5, output_level=0)
    Zn = Z.copy()
    Zn[3, 0] = np.nan
    with pytest.raises(ValueError, match="replicated data.*complete"):
        G.vecchia_estimate(Zn, locs, m=5, cond_yz="z", smoothness=1.5, output_level=0)


def rep_form_rows(locsord, revNN, Z_ord, covmodel, cp, tau):
    """Every row as the kernel forms it, float64: u = S'^-1 e_last, t_p = D_p u (u for the nugget), y_p = S'^-1 t_p, a_p = u't_p,
    q_r = u'z_r, b_{p,r} = y_p'z_r, Q2 = sum_r q_r^2, QB_p = sum_r q_r b_{p,r};  {sum_r l, sum_r dl, the triangle of R F_k}."""
    locsord, Z_ord = np.asarray(locsord, dtype=np.float64), np.asarray(Z_ord, dtype=np.float64)
    R = Z_ord.shape[1]
    out = np.full((len(locsord), T.ncols(covmodel) + F.ntri(covmodel)), np.nan)
    for g, rows, idx in F._groups(revNN):
        S, D = F._blocks(locsord[idx], covmodel, cp, tau)
        e = np.zeros((len(rows), g, 1))
        e[:, -1, 0] = 1.0
        u = np.linalg.solve(S, e)                                        # (rows, g, 1)
        t = np.concatenate([d @ u for d in D], axis=-1)                  # (rows, g, k)
        y = np.linalg.solve(S, t)
        ul = u[:, -1, 0]
        a = (u * t).sum(axis=1)                                          # (rows, k)
        zJ = Z_ord[idx]                                                  # (rows, g, R)
        q = (u * zJ).sum(axis=1)                                         # (rows, R)
        b = np.swapaxes(y, -1, -2) @ zJ                                  # (rows, k, R)
        Q2 = (q * q).sum(axis=1)
        QB = (b * q[:, None, :]).sum(axis=2)                             # (rows, k)
        ell = R * (0.5 * np.log(ul) - T.HALF_LOG_2PI) - 0.5 * Q2 / ul
        d = -0.5 * R * a / ul[:, None] + QB / ul[:, None] - 0.5 * Q2[:, None] * a / (ul * ul)[:, None]
        Fk = np.swapaxes(t, -1, -2) @ y / ul[:, None, None] - 0.5 * a[:, :, None] * a[:, None, :] / (ul * ul)[:, None, None]
        dl = [d[:, i] for i in range(d.shape[1])]
        out[rows] = np.concatenate([T._spread(covmodel, ell, dl[:-1], dl[-1]), R * F.tri(F.square(covmodel, Fk))], axis=1)
    return out


def rep_truth_rows(locsord, revNN, Z_ord, covmodel, cp, tau):
    """The truth for R columns: the sum of _grad_truth.rows_f64 over the columns, then R times the Fisher rows."""
    Z_ord = np.asarray(Z_ord)
    val = sum(T.rows_f64(locsord, revNN, Z_ord[:, r], covmodel, cp, tau) for r in range(Z_ord.shape[1]))
    return np.concatenate([val, Z_ord.shape[1] * F.rows_f64(locsord, revNN, covmodel, cp, tau)], axis=1)


@pytest.mark.parametrize("fam", ("nu1.5", "esqe"))
@pytest.mark.parametrize("dup", (False, True), ids=["distinct", "coincident"])
@pytest.mark.parametrize("m,d", [(10, 2), (15, 9)], ids=["m10-d2", "m15-d9"])
def test_kernel_form_equals_the_column_summed_truth(m, d, dup, fam):
    r = 0.25 * np.sqrt(d / 2)
    cm, cp = {"nu1.5": ("matern", [1.3, r, 1.5]), "esqe": ("esqe", [0.8, r, 0.5, 0.8 * r])}[fam]
    rng = np.random.default_rng(11)                    # the inputs of tests/test_gpu_loglik_grad.py::_setup
    n, R = 300, 3
    locs = rng.random((n, d))
    rng.standard_normal(n)
    Z = np.random.default_rng(11).standard_normal((n, R))
    if dup:                                           # every third point sits on an earlier one
        for j in range(2, n, 3):
            locs[j] = locs[rng.integers(j)]
    revNN = _rev_nn(locs, m)
    if dup:                                            # a coincident earlier point wins the tie: the own point back to the end
        for j in np.where(revNN[:, -1] != np.arange(1, n + 1))[0]:
            c = int(np.where(revNN[j] == j + 1)[0][0])
            revNN[j, -1], revNN[j, c] = revNN[j, c], revNN[j, -1]
    form = rep_form_rows(locs, revNN, Z, cm, cp, TAU)
    truth = rep_truth_rows(locs, revNN, Z, cm, cp, TAU)
    err = T.scaled_row_error(form, truth)
    print(f"kernel form against the column-summed truth: {err.max():.2e} (row {int(err.argmax())})")
    assert err.max() <= FORM_BAR
    # the identity itself, per replicate: b = w'D u = z'y
    k = n - 1
    idx = T.valid_entries(revNN[k])
    S, D = F._blocks(locs[idx][None], cm, cp, TAU)
    e = np.zeros(len(idx))
    e[-1] = 1.0
    u = np.linalg.solve(S[0], e)
    for Dp in D:
        tp = Dp[0] @ u
        for rr in range(R):
            w = np.linalg.solve(S[0], Z[idx, rr])
            assert abs(w @ tp - Z[idx, rr] @ np.linalg.solve(S[0], tp)) <= 1e-11 * max(abs(w @ tp), 1.0)


@pytest.mark.parametrize("method", ["Nelder-Mead", "L-BFGS-B", "fisher"])
@pytest.mark.parametrize("xkind", ["missing", "none", "given"])
def test_estimate_with_replicates_on_stubbed_likelihoods(monkeypatch, method, xkind):
    """Trend handling, n_replicates and the calls that are made, on a smooth stub of the parameters and of the data it is handed;
    the 1-D call goes on calling the one-column functions with the arguments it always passed."""
    import gpvecchia_amd as G
    from gpvecchia_amd import api as A
    rng = np.random.default_rng(5)
    n, R = 80, 4
    locs = rng.random((n, 2))
    Xm = np.column_stack([np.ones(n), locs[:, 0]])
    data = (Xm @ [2.0, -1.5])[:, None] + rng.standard_normal((n, R))
    target = np.log([1.4, 0.2, 0.3])
    seen = dict(rep=0, one=0, z=None)

    def parts(z, cp, nug):
        seen["z"] = np.array(z)
        cols = z.shape[1] if z.ndim == 2 else 1
        th = np.array([cp[0], cp[1], nug])
        d = np.log(th) - target
        ll = cols * (-float(d @ d) - 0.3 * float(d[0] * d[1])) - 0.5 * float((z * z).sum()) / len(z)
        g = -cols * (2 * d + 0.3 * np.array([d[1], d[0], 0.0])) / th
        info = cols * (2 * np.eye(3) + 0.3 * np.array([[0, 1, 0], [1, 0, 0], [0, 0, 0]])) / np.outer(th, th)
        info4 = np.full((4, 4), np.nan)
        info4[np.ix_([0, 1, 3], [0, 1, 3])] = info
        return ll, np.array([g[0], g[1], np.nan, g[2]]), info4

    def one(k):
        def fn(z, va, cp, nug, covmodel="matern", device=0):          # (no smoothness_grad: the default call passes none)
            assert np.ndim(z) == 1
            seen["one"] += 1
            out = parts(z, cp, nug)
            return out[0] if k == 1 else out[:k]
        return fn

    def rep(k):
        def fn(Z, va, cp, nug, covmodel="matern", device=0):
            assert np.ndim(Z) == 2 and Z.shape[1] == R
            seen["rep"] += 1
            out = parts(Z, cp, nug)
            if k == 1:                                                # per-replicate likelihoods: anything that sums to the total
                return np.full(R, out[0] / R)
            return out[:k]
        return fn

    monkeypatch.setattr(A, "vecchia_likelihood", one(1))
    monkeypatch.setattr(A, "vecchia_likelihood_grad", one(2))
    monkeypatch.setattr(A, "vecchia_likelihood_fisher", one(3))
    monkeypatch.setattr(A, "vecchia_likelihood_replicates", rep(1))
    monkeypatch.setattr(A, "vecchia_likelihood_grad_replicates", rep(2))
    monkeypatch.setattr(A, "vecchia_likelihood_fisher_replicates", rep(3))
    X = {"missing": "missing", "none": None, "given": Xm}[xkind]
    kw = dict(X=X, m=5, cond_yz="z", output_level=0, smoothness=1.5, method=method, nn_backend="host")
    res = G.vecchia_estimate(data, locs, **kw)
    assert res["n_replicates"] == R and seen["one"] == 0 and seen["rep"] == res["n_evals"] > 0
    assert res["trend"] == {"missing": "constant", "none": "none", "given": "userspecified"}[xkind]
    assert res["z"].shape == (n, R) and np.array_equal(seen["z"], res["z"])
    if xkind == "missing":                                            # the grand mean
        assert np.array_equal(res["beta_hat"], [data.mean()]) and np.array_equal(res["z"], data - data.mean())
    elif xkind == "none":
        assert res["beta_hat"].size == 0 and np.array_equal(res["z"], data)
    else:                                                             # one common beta_hat: OLS on the replicate mean
        want = np.linalg.lstsq(Xm, data.mean(axis=1), rcond=None)[0]
        assert np.allclose(res["beta_hat"], want, rtol=1e-10, atol=0)
        assert np.allclose(res["z"], data - (Xm @ want)[:, None], rtol=0, atol=1e-12)
    assert np.allclose(res["theta_hat"], np.exp(target), rtol=2e-2)
    if method == "fisher":                                            # the R-fold information
        th = res["theta_hat"]
        one_col = (2 * np.eye(3) + 0.3 * np.array([[0, 1, 0], [1, 0, 0], [0, 0, 0]])) / np.outer(th, th)
        assert np.allclose(res["fisher_info"], R * one_col, rtol=1e-12, atol=0)
        assert np.allclose(res["theta_se"], np.sqrt(np.diag(np.linalg.inv(R * one_col))), rtol=1e-9, atol=0)
    # the 1-D call: the one-column functions only, no n_replicates
    seen.update(rep=0, one=0)
    res1 = G.vecchia_estimate(data[:, 0], locs, **kw)
    assert "n_replicates" not in res1 and seen["rep"] == 0 and seen["one"] == res1["n_evals"] > 0
    assert res1["z"].shape == (n,)
