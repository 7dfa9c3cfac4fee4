"""gpv_plan_loglik_fisher and Fisher scoring without a GPU: the export, the argument checks that come before the device is
touched, the ValueErrors of the Python layer, the truth helper of the GPU tests (tests/_fisher_truth.py) against independent
statements of the same information -- the dense multivariate normal at m = n - 1, the form the product computes, and the
Monte-Carlo covariance of the score -- and the scoring loop of vecchia_estimate(method="fisher") on that truth as its callback."""
import ctypes as C

import numpy as np
import pytest

import _fisher_truth as F
import _grad_truth as T

TAU = 0.1
CASES = {"nu0.5": ("matern", [1.3, 0.25, 0.5]), "nu1.5": ("matern", [1.3, 0.25, 1.5]), "nu2.5": ("matern", [1.3, 0.25, 2.5]),
         "esqe": ("esqe", [0.8, 0.25, 0.5, 0.2])}
# float64 restatements against the long-double definition, scaled per row by max(|row|_inf, 1): the bound the GPU tests assert
# (tests/test_gpu_loglik_fisher.py, measured there over all rows of all its cases)
F64_VS_LD = 1e-12


def _rev_nn(locs, m):
    from oracle import r_side as R
    if m == 0:
        return np.arange(1, len(locs) + 1, dtype=np.int64)[:, None]
    return np.nan_to_num(R.findOrderedNN(locs, m)[:, ::-1], nan=0.0).astype(np.int64)


def test_symbol_is_exported():
    from gpvecchia_amd import _lib
    import gpvecchia_amd as G
    assert "gpv_plan_loglik_fisher" in _lib.EXPORTS
    assert getattr(_lib.lib(), "gpv_plan_loglik_fisher") is not None
    assert callable(G.vecchia_likelihood_fisher) and callable(G.Plan.loglik_fisher)


def test_null_pointers_are_bad_arguments():
    from gpvecchia_amd import _lib
    cp, grad, info = np.array([1.0, 0.1, 1.5]), np.zeros(4), np.zeros(16)
    ll, nf = C.c_double(), C.c_int64()
    fn = _lib.lib().gpv_plan_loglik_fisher
    assert fn(None, b"matern", _lib.dptr(cp), 3, 0.1, C.byref(ll), _lib.dptr(grad), _lib.dptr(info), C.byref(nf), None) == 2
    assert fn(None, b"matern", _lib.dptr(cp), 3, 0.1, C.byref(ll), _lib.dptr(grad), None, C.byref(nf), None) == 2
    assert fn(None, None, None, 3, 0.1, None, None, None, None, None) == 2       # GPV_ERR_BAD_ARG


def test_python_layer_refuses_what_has_no_gradient():
    import gpvecchia_amd as G
    rng = np.random.default_rng(0)
    locs, z = rng.random((60, 2)), rng.standard_normal(60)
    cp = [1.0, 0.2, 1.5]
    va_z = G.vecchia_specify(locs, 5, ordering="none", cond_yz="z", nn_backend="host")
    va_sgv = G.vecchia_specify(locs, 5, ordering="none", cond_yz="SGV", nn_backend="host")
    with pytest.raises(ValueError, match="vecchia_likelihood_fisher needs cond_yz"):
        G.vecchia_likelihood_fisher(z, va_sgv, cp, TAU)
    with pytest.raises(ValueError, match="constant nugget"):
        G.vecchia_likelihood_fisher(z, va_z, cp, np.full(60, TAU))
    zn = z.copy()
    zn[7] = np.nan
    with pytest.raises(ValueError, match="complete data"):
        G.vecchia_likelihood_fisher(zn, va_z, cp, TAU)
    va_pred = dict(va_z)
    va_pred["obs"] = np.concatenate([np.ones(50, bool), np.zeros(10, bool)])
    with pytest.raises(ValueError, match="prediction"):
        G.vecchia_likelihood_fisher(z, va_pred, cp, TAU)
    with pytest.raises(ValueError, match="named covariance"):
        G.vecchia_likelihood_fisher(z, va_z, cp, TAU, covmodel=lambda d: np.exp(-d))
    # the estimation driver: the preconditions of L-BFGS-B
    with pytest.raises(ValueError, match="method='fisher'.*smoothness"):
        G.vecchia_estimate(z, locs, m=5, method="fisher", cond_yz="z", output_level=0)
    with pytest.raises(ValueError, match="method='fisher'.*smoothness"):
        G.vecchia_estimate(z, locs, m=5, method="fisher", smoothness=0.8, cond_yz="z", output_level=0)
    with pytest.raises(ValueError, match="method='fisher' needs cond_yz"):
        G.vecchia_estimate(z, locs, m=5, method="fisher", smoothness=1.5, output_level=0)
    with pytest.raises(ValueError, match="named covariance"):
        G.vecchia_estimate(z, locs, m=5, method="fisher", cond_yz="z", covmodel=lambda d: np.exp(-d), output_level=0)


@pytest.mark.parametrize("fam", sorted(CASES))
def test_definition_sums_to_the_dense_information_at_full_conditioning(fam):
    cm, cp = CASES[fam]
    rng = np.random.default_rng(1)
    n = 40
    locs = rng.random((n, 2))
    revNN = _rev_nn(locs, n - 1)
    want = F.tri(F.dense(locs, cm, cp, TAU))
    keep = ~np.isnan(want)
    for rows in (F.rows_f64(locs, revNN, cm, cp, TAU), F.rows_form_f64(locs, revNN, cm, cp, TAU)):
        tot, scale = rows.sum(axis=0), np.abs(rows).sum(axis=0)
        assert np.array_equal(np.isnan(tot), ~keep)
        assert np.all(np.abs(tot - want)[keep] <= 1e-12 * scale[keep]), (tot, want)


def _plan_case(m, d, dup):
    rng = np.random.default_rng(3)
    n = 120 if m < 63 else 160
    locs = rng.random((n, d))
    if dup:                                            # every third point sits on an earlier one
        for j in range(2, n, 3):
            locs[j] = locs[rng.integers(j)]
    revNN = _rev_nn(locs, m)
    if dup:                                            # a coincident earlier point wins the tie: the own point back to the end
        for j in np.where(revNN[:, -1] != np.arange(1, n + 1))[0]:
            c = int(np.where(revNN[j] == j + 1)[0][0])
            revNN[j, -1], revNN[j, c] = revNN[j, c], revNN[j, -1]
    return locs, revNN


@pytest.mark.parametrize("fam", ("nu0.5", "nu2.5", "esqe"))
@pytest.mark.parametrize("m,d,dup", [(30, 2, False), (63, 2, False), (15, 9, False), (0, 2, False), (10, 2, True)],
                         ids=["m30-d2", "m63-d2", "m15-d9", "m0-d2", "m10-d2-coincident"])
def test_computed_form_equals_the_definition(m, d, dup, fam):
    """t_i'y_j / u_last - 1/2 a_i a_j / u_last^2 against the two traces: all rows in float64 against each other, every fourth
    row of both against the long-double definition."""
    cm, cp = CASES[fam]
    cp = list(cp)
    cp[1] = 0.25 * np.sqrt(d / 2)
    if cm == "esqe":
        cp[3] = 0.8 * cp[1]
    locs, revNN = _plan_case(m, d, dup)
    definition = F.rows_f64(locs, revNN, cm, cp, TAU)
    form = F.rows_form_f64(locs, revNN, cm, cp, TAU)
    pick = np.arange(0, len(locs), 4)
    ld = np.stack([F.row_ld(locs, revNN[k], cm, cp, TAU) for k in pick]).astype(np.float64)
    e_def, e_form = T.scaled_row_error(definition[pick], ld).max(), T.scaled_row_error(form[pick], ld).max()
    e_both = T.scaled_row_error(form, definition).max()
    print(f"definition against long double {e_def:.2e}, computed form against long double {e_form:.2e}, form against definition "
          f"{e_both:.2e}")
    assert e_def <= F64_VS_LD and e_form <= F64_VS_LD
    assert e_both <= 2 * F64_VS_LD                          # each within the bound of the same long-double figures


def _draw_field(rng, locs, cp, tau, ndraws):
    r = T._dist(locs)
    C_, _ = T._cov_and_derivs(r, "matern", cp)
    return np.linalg.cholesky(C_ + tau * np.eye(len(locs))) @ rng.standard_normal((len(locs), ndraws))


def test_information_is_the_covariance_of_the_score():
    """4000 draws of the exact process at n = 60, m = 5: the mean outer product of the total score (tests/_grad_truth.py) against
    sum_k F_k, every entry within 5 of its own Monte-Carlo standard errors.  (The Vecchia score has expectation zero under the
    exact process and its rows are uncorrelated, so the information is the second moment of the total.)"""
    cm, cp = CASES["nu1.5"]
    rng = np.random.default_rng(7)
    n, m, ndraws = 60, 5, 4000
    locs = rng.random((n, 2))
    revNN = _rev_nn(locs, m)
    Z = _draw_field(rng, locs, cp, TAU, ndraws)
    pos = F._positions(cm)
    score = np.stack([T.rows_f64(locs, revNN, Z[:, t], cm, cp, TAU)[:, 1:].sum(axis=0)[pos] for t in range(ndraws)])
    outer = score[:, :, None] * score[:, None, :]
    mean, se = outer.mean(axis=0), outer.std(axis=0, ddof=1) / np.sqrt(ndraws)
    info = F.untri(F.rows_f64(locs, revNN, cm, cp, TAU).sum(axis=0), F.npar(cm))[np.ix_(pos, pos)]
    dev = np.abs(mean - info) / se
    print("information\n", info, "\nmean outer product of the score\n", mean, "\ndeviation in standard errors\n", dev)
    assert np.all(dev <= 5.0)
    assert np.all(np.abs(score.mean(axis=0)) <= 5.0 * score.std(axis=0, ddof=1) / np.sqrt(ndraws))


def _scoring_problem():
    """A Matern-1.5 field at n = 400, m = 10, and the callback of the scoring loop in the log-parameters (variance, range, nugget)
    from the numpy truth alone."""
    rng = np.random.default_rng(12)
    n, m = 400, 10
    locs = rng.random((n, 2))
    z = _draw_field(rng, locs, [2.0, 0.2, 1.5], 0.3, 1)[:, 0]
    revNN = _rev_nn(locs, m)
    pos = [0, 1, 3]
    calls = []

    def fn(lg):
        th = np.exp(lg)
        cp = [th[0], th[1], 1.5]
        with np.errstate(all="ignore"):
            try:
                rows = T.rows_f64(locs, revNN, z, "matern", cp, th[2])
                tri = F.rows_f64(locs, revNN, "matern", cp, th[2])
            except np.linalg.LinAlgError:
                calls.append((lg.copy(), -np.inf))
                return -np.inf, np.full(3, np.nan), np.full((3, 3), np.nan)
        tot = rows.sum(axis=0)
        info = F.untri(tri.sum(axis=0), 4)[np.ix_(pos, pos)]
        calls.append((lg.copy(), float(tot[0])))
        return float(tot[0]), tot[1:][pos] * th, info * np.outer(th, th)
    return fn, calls, z


def test_scoring_loop_converges_to_the_stationary_point():
    from gpvecchia_amd.wrappers import _fisher_scoring
    fn, calls, z = _scoring_problem()
    reltol = np.sqrt(np.finfo(float).eps)
    x0 = np.log([0.9 * np.var(z, ddof=1), 0.13, 0.1 * np.var(z, ddof=1)])          # vecchia_estimate's kind of start
    x, f, g, info, n_evals, code = _fisher_scoring(fn, x0, reltol=reltol, maxit=300)
    print("theta", np.exp(x), "value", f, "gradient", g, "evaluations", n_evals, "code", code)
    assert code == 0 and n_evals == len(calls) and n_evals <= 12
    vals = [v for _, v in calls]
    assert f == max(vals) and np.array_equal(x, calls[int(np.argmax(vals))][0])
    # the stopping rule, and what it says about the gradient: g'I^-1 g >= |g|^2 / lambda_max
    gain = float(g @ np.linalg.solve(info, g))
    assert 0 <= gain <= reltol * abs(f)
    assert np.sqrt(g @ g) <= np.sqrt(reltol * abs(f) * np.linalg.eigvalsh(info).max())
    # the stationary point: a far tighter search from there moves the value by less than the rule's reltol |value|
    x2, f2, g2, info2, _, code2 = _fisher_scoring(fn, x, reltol=1e-14, maxit=300)
    print("tight search: theta", np.exp(x2), "value", f2, "gradient", g2)
    assert code2 == 0 and f <= f2 <= f + reltol * abs(f)
    assert np.sqrt(g2 @ g2) <= np.sqrt(1e-14 * abs(f2) * np.linalg.eigvalsh(info2).max())


def test_scoring_loop_halves_a_step_that_is_too_long():
    from gpvecchia_amd.wrappers import _fisher_scoring
    fn, calls, z = _scoring_problem()
    reltol = np.sqrt(np.finfo(float).eps)
    x0 = np.log([5.0, 0.05, 0.02])                                                 # off, and no cap on the step's length
    x, f, g, info, n_evals, code = _fisher_scoring(fn, x0, reltol=reltol, maxit=300, max_step=np.inf)
    vals = np.array([v for _, v in calls])
    best = np.maximum.accumulate(vals)
    rejected = np.where(~(vals[1:] > best[:-1]))[0] + 1
    print("values", vals, "rejected evaluations", rejected, "code", code)
    assert len(rejected) >= 1 and rejected[0] == 1           # the first step overshoots: the halving branch is taken ...
    assert np.sqrt(((calls[1][0] - x0) ** 2).sum()) > 1.0    # (it is longer than the default cap)
    assert np.allclose(calls[2][0] - x0, 0.5 * (calls[1][0] - x0), rtol=1e-12, atol=0)
    assert code == 0 and n_evals == len(calls)
    ref, _, _ = _scoring_problem()
    x_ref = _fisher_scoring(ref, np.log([0.9 * np.var(z, ddof=1), 0.13, 0.1 * np.var(z, ddof=1)]), reltol=1e-14, maxit=300)
    assert abs(f - x_ref[1]) <= reltol * abs(x_ref[1])       # ... and the search still ends at the same maximum

    # ten halvings without an increase: the search gives up with code 1 where it stands
    def flat(lg):
        return (0.0 if np.array_equal(lg, np.zeros(2)) else -1.0), np.ones(2), np.eye(2)
    x, f, _, _, n_evals, code = _fisher_scoring(flat, np.zeros(2), reltol=reltol, maxit=300)
    assert code == 1 and n_evals == 12 and np.array_equal(x, np.zeros(2)) and f == 0.0
