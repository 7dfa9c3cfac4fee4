"""Cost of gpv_plan_loglik_grad_sgv (gpv_grad_sgv.hip): wall time of ONE blocking gradient call (an evaluation
with the posterior mean, the selected inverse, the per-set pass, the copy of the totals) beside
  (a) one SGV evaluation of the same plan (GPV_WANT_DENOM, the totals fetched), and
  (b) six such evaluations: what central differences over the three parameters of a Matern at a fixed smoothness cost.

    python tools/sgv_grad_timing.py [--n 100000 1000000] [--m 30] [--rounds 9] [--out profiles/sgv_grad_timing.json]

maxmin ordering, cond.yz = 'SGV', Matern 1.5, 2-D uniform locations, a constant nugget.  All legs run in ONE process, in --rounds
alternating rounds after a clock warm-up of evaluations, and are reported as median with minimum and maximum over the rounds.
The first call (index data built on the host from the plan's arrays, allocations, graph capture) is reported separately.  Prints
one JSON line per n and writes all of them to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (first: see tests/conftest.py)
import gpvecchia_amd as G  # noqa: E402


def wall_ms(f):
    t0 = time.perf_counter()
    f()
    return 1e3 * (time.perf_counter() - t0)


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def one_size(n, m, rounds):
    locs = np.random.default_rng(0).random((n, 2))
    z = np.random.default_rng(1).standard_normal(n)
    cp, nug = [1.0, 0.02 if n >= 500_000 else 0.05, 1.5], 0.1
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="SGV", nn_backend="gpu")
    plan = G.api._plan_for(va, 0)
    assert plan.ensure_posterior()
    plan.set_data(z[va["ord_z"] - 1])

    def ev(cp_=cp, nug_=nug):
        plan.eval("matern", cp_, nug_, G.GPV_WANT_DENOM)
        return G.loglik_from_sums(plan.sums(), n)

    def six():
        for i in range(3):
            for sgn in (1.0, -1.0):
                th = [cp[0], cp[1], nug]
                th[i] *= 1.0 + sgn * 1e-4
                ev([th[0], th[1], cp[2]], th[2])
    for _ in range(30):                                               # clock warm-up
        ev()
    first = wall_ms(lambda: plan.loglik_grad_sgv("matern", cp, nug))  # first use: index data, buffers, graphs
    ll, grad, nfail = plan.loglik_grad_sgv("matern", cp, nug)
    assert nfail == 0 and ll == ev()
    legs = dict(grad=[], eval=[], six=[])
    for _ in range(rounds):
        legs["grad"].append(wall_ms(lambda: plan.loglik_grad_sgv("matern", cp, nug)))
        legs["eval"].append(wall_ms(ev))
        legs["six"].append(wall_ms(six))
    out = dict(n=n, m=m, rounds=rounds, levels=plan.posterior_levels(), grad_first_call_ms=first, loglik=ll,
               grad=[None if np.isnan(g) else float(g) for g in grad], grad_call_ms=spread(legs["grad"]),
               sgv_eval_ms=spread(legs["eval"]), six_sgv_evals_ms=spread(legs["six"]))
    out["grad_call_over_six_evals"] = out["grad_call_ms"]["median"] / max(out["six_sgv_evals_ms"]["median"], 1e-9)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--m", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join("profiles", "sgv_grad_timing.json"))
    a = ap.parse_args()
    res = []
    for n in a.n:
        res.append(one_size(n, a.m, a.rounds))
        print(json.dumps(res[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
