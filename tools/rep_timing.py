"""Cost of one gpv_plan_loglik_rep call (gpv_rep_kernel.hpp) for R replicates beside the one-column entries of the
same plan, with the protocol of tools/grad_timing.py:

    python tools/rep_timing.py [--n 1000000] [--m 30] [--nu 1.5] [--R 1,16,64] [--rounds 9] [--reps 7]

One process, one plan (d = 2, cond.yz = 'z', maxmin ordering).  After a clock warm-up of likelihood evaluations (as bench.py does)
the legs run in alternating rounds -- `reps` calls of gpv_plan_loglik_rep at each R (the replicates are uploaded before the leg and
the upload is not timed: an optimiser uploads once), `reps` calls of gpv_plan_loglik_fisher and `reps` of gpv_plan_loglik_grad on
one column -- and each is reported as the median over the rounds of the round's median, wall clock around the blocking calls.
The yardsticks are the two one-column calls: R gradient calls are what a user with R columns pays without the replicate entry.
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (first: see tests/conftest.py)
import gpvecchia_amd as G  # noqa: E402
from grad_timing import med  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=30)
    ap.add_argument("--nu", type=float, default=1.5)
    ap.add_argument("--R", type=str, default="1,16,64")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    n, m = a.n, a.m
    Rs = [int(r) for r in a.R.split(",")]
    locs = np.random.default_rng(0).random((n, 2))
    Z = np.random.default_rng(1).standard_normal((n, max(Rs)))
    cp, tau = [1.0, 0.02 if n >= 500_000 else 0.05, a.nu], 0.1
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="z", nn_backend="gpu")
    plan = G.api._plan_for(va, 0)
    Zord = np.asfortranarray(Z[va["ord_z"] - 1])
    plan.set_data(Zord[:, 0])
    nug = np.array([tau])

    def lik():
        plan.eval("matern", cp, nug, G.GPV_WANT_LOGLIK_Z)
        return plan.sums()

    def grad():
        return plan.loglik_grad("matern", cp, tau)

    def fisher():
        return plan.loglik_fisher("matern", cp, tau)

    def rep():
        return plan.loglik_replicates("matern", cp, tau)
    for _ in range(30):                                               # clock warm-up
        lik()
    ll, g, nfail = grad()                                             # first use: buffers
    ll_f, g_f, info, nfail_f = fisher()
    check = {}
    for R in Rs:                                                      # first use, and what the call returns against the yardsticks
        plan.set_replicates(Zord[:, :R])
        ll_r, g_r, info_r, nfail_r = rep()
        check[R] = dict(n_failed=nfail_r, info_over_R_rel_diff=float(np.nanmax(np.abs(info_r / R - info) / np.abs(info))))
        if R == 1:
            keep = ~np.isnan(g)
            check[R].update(value_rel_diff=abs(ll_r - ll) / abs(ll),
                            grad_rel_diff=float((np.abs(g_r - g)[keep] / np.abs(g)[keep]).max()))
    t_rep, t_grad, t_fi = {R: [] for R in Rs}, [], []
    for _ in range(a.rounds):
        for R in Rs:
            plan.set_replicates(Zord[:, :R])
            t_rep[R].append(med(rep, a.reps))
        t_fi.append(med(fisher, a.reps))
        t_grad.append(med(grad, a.reps))
    out = dict(n=n, m=m, nu=a.nu, rounds=a.rounds, reps=a.reps, loglik_grad_ms=float(np.median(t_grad)),
               loglik_fisher_ms=float(np.median(t_fi)), loglik_grad_ms_rounds=[round(t, 4) for t in t_grad],
               loglik_fisher_ms_rounds=[round(t, 4) for t in t_fi], n_failed=[nfail, nfail_f], replicates={})
    for R in Rs:
        t = float(np.median(t_rep[R]))
        out["replicates"][str(R)] = dict(loglik_rep_ms=t, loglik_rep_ms_rounds=[round(v, 4) for v in t_rep[R]],
                                         over_fisher=t / out["loglik_fisher_ms"], R_grad_calls_ms=R * out["loglik_grad_ms"],
                                         over_R_grad_calls=t / (R * out["loglik_grad_ms"]), **check[R])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
