"""Cost of covmodel='matern_scaledim' (one range per coordinate) beside 'matern' on the same plan:

    python tools/scaledim_timing.py [--n 1000000] [--m 30] [--dim 2] [--nu 1.5] [--R 4] [--rounds 9] [--reps 7]

One process, one plan (cond.yz = 'z', maxmin ordering), `R` replicate columns.  After a clock warm-up of likelihood evaluations (as
bench.py does) eight legs run in alternating rounds, each family's call next to its counterpart:
    a likelihood-only evaluation (plan.eval(GPV_WANT_LOGLIK_Z) + sums())   'matern' | 'matern_scaledim'
    gpv_plan_loglik_grad, gpv_plan_loglik_fisher, gpv_plan_loglik_rep      'matern' | 'matern_scaledim'
The scaled family runs at EQUAL ranges, the isotropic leg's range, so both legs see the same distances and covariances: what
differs is the streaming pass that writes the scaled copy of the records in front of every call, and in the gradient-type kernels
dim - 1 more bilinear forms (and, for dim < 3, slots that sum exact zeros).  Each leg is reported as the median over the rounds of
the round's median, wall clock around the blocking calls; `copy_bytes` is what the scaling pass reads and writes.  Prints one JSON
line."""
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
    ap.add_argument("--dim", type=int, default=2)
    ap.add_argument("--nu", type=float, default=1.5)
    ap.add_argument("--R", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    n, m, d = a.n, a.m, a.dim
    locs = np.random.default_rng(0).random((n, d))
    z = np.random.default_rng(1).standard_normal(n)
    Z = np.random.default_rng(2).standard_normal((n, a.R))
    rho = (0.02 if n >= 500_000 else 0.05) * (1.0 if d <= 2 else 4.0)   # a few neighbours per range (3-D: spacing 0.01 at n = 1e6)
    tau = 0.1
    cp = {"matern": [1.0, rho, a.nu], "matern_scaledim": [1.0] + [rho] * d + [a.nu]}
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="z", nn_backend="gpu")
    plan = G.api._plan_for(va, 0)
    plan.set_data(z[va["ord_z"] - 1])
    plan.set_replicates(Z[va["ord_z"] - 1])
    nug = np.array([tau])

    def lik(fam):
        plan.eval(fam, cp[fam], nug, G.GPV_WANT_LOGLIK_Z)
        return plan.sums()
    legs = {}
    for fam, tag in (("matern", "iso"), ("matern_scaledim", "sd")):
        legs["lik_" + tag] = lambda fam=fam: lik(fam)
        legs["grad_" + tag] = lambda fam=fam: plan.loglik_grad(fam, cp[fam], tau)
        legs["fisher_" + tag] = lambda fam=fam: plan.loglik_fisher(fam, cp[fam], tau)
        legs["rep_" + tag] = lambda fam=fam: plan.loglik_replicates(fam, cp[fam], tau)
    order = [k + t for k in ("lik_", "grad_", "fisher_", "rep_") for t in ("iso", "sd")]
    for _ in range(30):                                               # clock warm-up
        lik("matern")
    first = {k: legs[k]() for k in order}                             # first use: buffers; and the two families agree
    ll = {t: G.loglik_z_from_sums(first["lik_" + t], n) for t in ("iso", "sd")}
    times = {k: [] for k in order}
    for _ in range(a.rounds):
        for k in order:
            times[k].append(med(legs[k], a.reps))
    out = dict(n=n, m=m, dim=d, nu=a.nu, R=a.R, range=rho, rounds=a.rounds, reps=a.reps,
               copy_bytes=2 * 8 * n * (4 if d <= 3 else d), last_set_kernel=plan.last_set_kernel(),
               lik_value_rel_diff=abs(ll["sd"] - ll["iso"]) / abs(ll["iso"]),
               grad_value_rel_diff=abs(first["grad_sd"][0] - first["grad_iso"][0]) / abs(first["grad_iso"][0]),
               grad_range_sum_rel_diff=abs(first["grad_sd"][1][1:1 + d].sum() - first["grad_iso"][1][1]) / abs(first["grad_iso"][1][1]),
               n_failed=[int(first[k][-1]) if k[:3] != "lik" else int(first[k][6]) for k in order])
    for k in order:
        out[k + "_ms"] = float(np.median(times[k]))
        out[k + "_ms_rounds"] = [round(t, 4) for t in times[k]]
    for k in ("lik", "grad", "fisher", "rep"):
        out[k + "_sd_minus_iso_ms"] = out[k + "_sd_ms"] - out[k + "_iso_ms"]
        out[k + "_sd_over_iso"] = out[k + "_sd_ms"] / out[k + "_iso_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
