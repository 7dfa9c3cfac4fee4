"""Cost of one gpv_plan_loglik_grad call (gpv_grad.hip) beside one likelihood-only evaluation of the same plan:

    python tools/grad_timing.py [--n 1000000] [--m 30] [--nu 1.5] [--rounds 9] [--reps 7] [--fisher]

One process, one plan (d = 2, cond.yz = 'z', maxmin ordering).  After a clock warm-up of likelihood evaluations (as bench.py
does) the two legs run in alternating rounds -- `reps` gradient calls, `reps` plan.eval(GPV_WANT_LOGLIK_Z) + sums() -- and each
is reported as the median over the rounds of the round's median, wall clock around the blocking calls.  The second leg is the
code the benchmark measures and is the yardstick; central differences over the 3 parameters would cost 2 * 3 + 1 = 7 of them.
--fisher adds a third leg to every round, `reps` calls of gpv_plan_loglik_fisher (gpv_grad.hip), and
reports it beside the gradient call of the same build, which is its yardstick (loglik_fisher_ms, fisher_over_grad).
--nu-leg NU (a general smoothness, e.g. 0.8) adds the legs of DESIGN.md §4j to every round, on the same plan: `reps` calls of
gpv_plan_loglik_grad_nu and of gpv_plan_loglik_fisher_nu at that smoothness, and `reps` general-nu likelihood-only evaluations,
of which central differences over the four parameters would cost 2 * 4 + 1 = 9 (nu_central_difference_ms).  The closed-form legs
at --nu stay in the rounds: they are the parent's code and the yardstick.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (first: see tests/conftest.py)
import gpvecchia_amd as G  # noqa: E402


def med(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=30)
    ap.add_argument("--nu", type=float, default=1.5)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--fisher", action="store_true", help="also time gpv_plan_loglik_fisher, in the same alternating rounds")
    ap.add_argument("--nu-leg", type=float, default=None, metavar="NU",
                    help="also time the _nu entries and the likelihood at this general smoothness, in the same alternating rounds")
    a = ap.parse_args()
    n, m = a.n, a.m
    locs = np.random.default_rng(0).random((n, 2))
    z = np.random.default_rng(1).standard_normal(n)
    cp, tau = [1.0, 0.02 if n >= 500_000 else 0.05, a.nu], 0.1
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="z", nn_backend="gpu")
    plan = G.api._plan_for(va, 0)
    plan.set_data(z[va["ord_z"] - 1])
    nug = np.array([tau])

    def lik():
        plan.eval("matern", cp, nug, G.GPV_WANT_LOGLIK_Z)
        return plan.sums()

    def grad():
        return plan.loglik_grad("matern", cp, tau)

    def fisher():
        return plan.loglik_fisher("matern", cp, tau)
    cpn = [cp[0], cp[1], a.nu_leg] if a.nu_leg is not None else None  # (the three legs below run only with --nu-leg)

    def lik_nu():
        plan.eval("matern", cpn, nug, G.GPV_WANT_LOGLIK_Z)
        return plan.sums()

    def grad_nu():
        return plan.loglik_grad("matern", cpn, tau, smoothness_grad=True)

    def fisher_nu():
        return plan.loglik_fisher("matern", cpn, tau, smoothness_grad=True)
    for _ in range(30):                                               # clock warm-up
        lik()
    ll, g, nfail = grad()                                             # first use: buffers
    ll_ref = G.loglik_z_from_sums(lik(), n)
    if a.fisher:
        ll_f, g_f, info, nfail_f = fisher()                           # first use: buffers
    if a.nu_leg is not None:
        ll_n, g_n, nfail_n = grad_nu()                                # first use: buffers
        ll_fn, g_fn, info_n, nfail_fn = fisher_nu()
        ll_nref = G.loglik_z_from_sums(lik_nu(), n)
    t_grad, t_lik, t_fi, t_gn, t_fn, t_ln = [], [], [], [], [], []
    for _ in range(a.rounds):
        if a.nu_leg is not None:
            t_gn.append(med(grad_nu, a.reps))
            t_fn.append(med(fisher_nu, a.reps))
            t_ln.append(med(lik_nu, a.reps))
        t_grad.append(med(grad, a.reps))
        if a.fisher:
            t_fi.append(med(fisher, a.reps))
        t_lik.append(med(lik, a.reps))
    out = dict(n=n, m=m, nu=a.nu, rounds=a.rounds, reps=a.reps, loglik_grad_ms=float(np.median(t_grad)),
               loglik_only_ms=float(np.median(t_lik)), loglik_grad_ms_rounds=[round(t, 4) for t in t_grad],
               loglik_only_ms_rounds=[round(t, 4) for t in t_lik], n_failed=nfail,
               value_rel_diff=abs(ll - ll_ref) / abs(ll_ref))
    out["ratio"] = out["loglik_grad_ms"] / out["loglik_only_ms"]
    out["central_difference_break_even"] = 7
    if a.fisher:
        keep = ~np.isnan(g)
        out.update(loglik_fisher_ms=float(np.median(t_fi)), loglik_fisher_ms_rounds=[round(t, 4) for t in t_fi],
                   fisher_n_failed=nfail_f, fisher_value_rel_diff=abs(ll_f - ll) / abs(ll),
                   fisher_grad_rel_diff=float((np.abs(g_f - g)[keep] / np.abs(g)[keep]).max()))
        out["fisher_over_grad"] = out["loglik_fisher_ms"] / out["loglik_grad_ms"]
    if a.nu_leg is not None:
        out.update(nu_leg=a.nu_leg, loglik_grad_nu_ms=float(np.median(t_gn)), loglik_fisher_nu_ms=float(np.median(t_fn)),
                   loglik_only_nu_ms=float(np.median(t_ln)), loglik_grad_nu_ms_rounds=[round(t, 4) for t in t_gn],
                   loglik_fisher_nu_ms_rounds=[round(t, 4) for t in t_fn], loglik_only_nu_ms_rounds=[round(t, 4) for t in t_ln],
                   nu_n_failed=[nfail_n, nfail_fn], nu_value_rel_diff=abs(ll_n - ll_nref) / abs(ll_nref),
                   nu_fisher_grad_rel_diff=float((np.abs(g_fn - g_n) / np.abs(g_n)).max()),
                   nu_grad_finite=bool(np.all(np.isfinite(g_n))), nu_info_finite=bool(np.all(np.isfinite(info_n))))
        out["nu_central_difference_ms"] = 9 * out["loglik_only_nu_ms"]
        out["nu_grad_over_central_differences"] = out["loglik_grad_nu_ms"] / out["nu_central_difference_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
