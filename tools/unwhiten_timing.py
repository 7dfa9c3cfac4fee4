"""Cost of gpv_plan_unwhiten / gpv_plan_simulate (gpv_unwhiten.hip) beside the whitening of the same columns and
beside the evaluation that leaves the factor:

    python tools/unwhiten_timing.py [--n 1000000] [--m 30] [--ordering maxmin] [--rounds 7] [--reps 5] [--cols 1,16]

One process, one plan (d = 2, cond.yz = 'z', Matern 1.5).  After a clock warm-up of likelihood evaluations (as bench.py does) the
legs run in alternating rounds and each is reported as the median over the rounds of the round's median:
  eval_U_ms            plan.eval(GPV_WANT_U) + sums(): the evaluation that leaves the factor in HBM, wall clock
  levels, launches     gpv_plan_unwhiten_levels: the schedule's levels and the launches of one sweep
  for every column count c:
    sweep_ms[c]        the level sweep alone over resident columns, by an event pair around it (gpv_plan_debug_unwhiten_ms)
    unwhiten_ms[c]     one blocking Plan.unwhiten call, wall clock: the sweep plus the columns' trip over PCIe and their packing
    whiten_pass_ms[c]  the whitening and Gram passes alone over the same columns (gpv_plan_debug_whiten_ms)
    whiten_ms[c]       one blocking Plan.whiten call of the same columns with E returned, wall clock
    floor_ms           launches x the launch floor of a dependent launch (--floor-us, DESIGN.md §4b: 4.7 - 5 us)
  simulate16_ms        one Plan.simulate(seed, 16) call, wall clock: normals on the device, the sweep, 16 columns back over PCIe
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (first: see tests/conftest.py)
import gpvecchia_amd as G  # noqa: E402
from gpvecchia_amd import _lib as L  # noqa: E402


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
    ap.add_argument("--ordering", default="maxmin")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cols", default="1,16")
    ap.add_argument("--floor-us", type=float, default=4.85)
    a = ap.parse_args()
    n, m = a.n, a.m
    cols = [int(c) for c in a.cols.split(",")]
    rng = np.random.default_rng(0)
    locs = rng.random((n, 2))
    z = rng.standard_normal(n)
    Eord = np.asfortranarray(rng.standard_normal((n, max(cols))))
    cp, tau = [1.0, 0.02 if n >= 500_000 else 0.05, 1.5], 0.1
    print(f"specify: n={n} m={m} ordering={a.ordering}", file=sys.stderr, flush=True)
    va = G.vecchia_specify(locs, m, ordering=a.ordering, cond_yz="z", nn_backend="gpu")
    plan = G.api._plan_for(va, 0)
    plan.set_data(z[va["ord_z"] - 1])
    nug = np.array([tau])
    lib = L.lib()
    lib.gpv_plan_debug_whiten_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    lib.gpv_plan_debug_unwhiten_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]

    def lik():
        plan.eval("matern", cp, nug, G.GPV_WANT_LOGLIK_Z)
        return plan.sums()

    def eval_u():
        plan.eval("matern", cp, nug, G.GPV_WANT_U)
        return plan.sums()

    def device_ms(entry, reps):
        ms = np.zeros(reps)
        L.check(getattr(lib, entry)(plan._h, reps, L.dptr(ms)), entry)
        return float(np.median(ms))
    for _ in range(30):                                               # clock warm-up
        lik()
    eval_u()
    t0 = time.perf_counter()
    levels, launches = plan.unwhiten_levels()                         # first use: the schedule
    schedule_ms = 1e3 * (time.perf_counter() - t0)
    print(f"schedule: {levels} levels, {launches} launches, {schedule_ms:.0f} ms", file=sys.stderr, flush=True)
    for c in cols:                                                    # first use: buffers, graphs
        plan.unwhiten(Eord[:, :c])
        plan.whiten(Eord[:, :c], want_E=True)
    plan.simulate(1, 16)
    legs = ("sweep_ms", "unwhiten_ms", "whiten_pass_ms", "whiten_ms")
    t_eval, t_sim, t = [], [], {k: {c: [] for c in cols} for k in legs}
    for r in range(a.rounds):
        t_eval.append(med(eval_u, a.reps))                            # (a new evaluation: every sweep graph is captured again)
        for c in cols:
            Ec = np.asfortranarray(Eord[:, :c])
            plan.unwhiten(Ec)                                         # the capture stays out of the timed calls
            t["unwhiten_ms"][c].append(med(lambda: plan.unwhiten(Ec), a.reps))
            t["sweep_ms"][c].append(device_ms("gpv_plan_debug_unwhiten_ms", a.reps))       # (over the columns that call left)
            t["whiten_ms"][c].append(med(lambda: plan.whiten(Ec, want_E=True), a.reps))
            t["whiten_pass_ms"][c].append(device_ms("gpv_plan_debug_whiten_ms", a.reps))
        plan.simulate(1, 16)
        t_sim.append(med(lambda: plan.simulate(1, 16), a.reps))
        print(f"round {r + 1} of {a.rounds}", file=sys.stderr, flush=True)
    ev = float(np.median(t_eval))
    floor = 1e-3 * a.floor_us * launches
    out = dict(n=n, m=m, ordering=a.ordering, rounds=a.rounds, reps=a.reps, narrow=lib.gpv_unwhiten_narrow(), levels=levels,
               launches=launches, schedule_ms=schedule_ms, eval_U_ms=ev, floor_us=a.floor_us, floor_ms=floor,
               simulate16_ms=float(np.median(t_sim)), sweep_over_whiten_pass={}, sweep_over_floor={}, sweep_over_eval={})
    for k in legs:
        out[k] = {c: float(np.median(t[k][c])) for c in cols}
    for c in cols:
        out["sweep_over_whiten_pass"][c] = out["sweep_ms"][c] / out["whiten_pass_ms"][c]
        out["sweep_over_floor"][c] = out["sweep_ms"][c] / floor
        out["sweep_over_eval"][c] = out["sweep_ms"][c] / ev
    print(json.dumps(out))


if __name__ == "__main__":
    main()
