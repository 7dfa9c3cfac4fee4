"""Cost of gpv_plan_selinv (gpv_selinv.hip): device time of ONE pass of the selected inverse, which gives every
posterior variance of the plan, beside
  (a) one batch of gpv_plan_solve_t (the transposed sweep over the same schedule, NB right-hand sides),
  (b) one batch of gpv_plan_lincomb with NB unit rows, and
  (c) that batch time x n / NB: what the exact route (lincomb.exact_variances_device) costs for the whole field.

    python tools/selinv_timing.py [--n 100000 1000000] [--m 30] [--rounds 9] [--out profiles/selinv_timing.json]

maxmin ordering, cond.yz = 'SGV', Matern 1.5, 2-D uniform locations, a constant nugget.  The pass and the transposed sweep are
timed on the device by a pair of events around the captured graph alone (gpv_plan_debug_selinv_ms, gpv_plan_debug_solve_t_ms:
no copies); the lincomb batch as in tools/lincomb_timing.py, wall clock around the blocking call with 1 and with 1 + batches
batches, the difference divided.  All legs run in ONE process, in --rounds alternating rounds after a clock warm-up of
evaluations, and are reported as median with minimum and maximum over the rounds.  The first call of the pass (records built on
the host from the plan's structure, allocations, graph capture) is reported separately.  Prints one JSON line per n and writes
all of them to --out."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (first: see tests/conftest.py)
import gpvecchia_amd as G  # noqa: E402
from gpvecchia_amd import _lib as L  # noqa: E402


def wall_ms(f):
    t0 = time.perf_counter()
    f()
    return 1e3 * (time.perf_counter() - t0)


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def one_size(n, m, rounds, batches):
    import scipy.sparse as sp
    lib = L.lib()
    lib.gpv_plan_debug_solve_t_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    lib.gpv_plan_debug_selinv_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    NB = lib.gpv_lincomb_batch()
    locs = np.random.default_rng(0).random((n, 2))
    z = np.random.default_rng(1).standard_normal(n)
    cp, nug = [1.0, 0.02 if n >= 500_000 else 0.05, 1.5], np.array([0.1])
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="SGV", nn_backend="gpu")
    plan = G.api._plan_for(va, 0)
    assert plan.ensure_posterior()
    plan.set_data(z[va["ord_z"] - 1])

    def ev():
        plan.eval("matern", cp, nug, G.GPV_WANT_MEAN)
        plan.sums()
    for _ in range(30):                                               # clock warm-up
        ev()
    rng = np.random.default_rng(2)

    def H(nb):
        rows = nb * NB
        idx = rng.choice(n, rows, replace=False)
        return sp.csr_matrix((np.ones(rows), idx, np.arange(rows + 1)), shape=(rows, n))
    H1, Hk = H(1), H(1 + batches)
    plan.lincomb(H1)                                                  # first use: records, X, graph
    plan.solve_t(rng.standard_normal((NB, n)))                        # first use: staging buffers, graph
    first = wall_ms(lambda: plan.selinv())                            # first use: records, Sigma, graph
    v, dropped = plan.selinv()
    check = plan.lincomb(H1)                                          # the exact route at NB locations: the same numbers
    err = float(np.abs(v[H1.indices] - check).max() / max(1.0, np.abs(check).max()))
    assert dropped == 0 and err <= 1e-8, (dropped, err)
    one = np.zeros(1)

    def dev_ms(fn, name):
        L.check(fn(plan._h, 1, L.dptr(one)), name)
        return float(one[0])
    legs = dict(selinv=[], solve_t=[], lc1=[], lck=[], selinv_call=[])
    for _ in range(rounds):
        legs["selinv"].append(dev_ms(lib.gpv_plan_debug_selinv_ms, "gpv_plan_debug_selinv_ms"))
        legs["solve_t"].append(dev_ms(lib.gpv_plan_debug_solve_t_ms, "gpv_plan_debug_solve_t_ms"))
        legs["lc1"].append(wall_ms(lambda: plan.lincomb(H1)))
        legs["lck"].append(wall_ms(lambda: plan.lincomb(Hk)))
        legs["selinv_call"].append(wall_ms(lambda: plan.selinv()))
    lc = (np.array(legs["lck"]) - np.array(legs["lc1"])) / batches
    out = dict(n=n, m=m, NB=NB, rounds=rounds, levels=plan.posterior_levels(), selinv_first_call_ms=first,
               selinv_vs_exact_route_max_rel_diff=err, selinv_pass_device_ms=spread(legs["selinv"]),
               selinv_call_wall_ms=spread(legs["selinv_call"]), solve_t_batch_device_ms=spread(legs["solve_t"]),
               lincomb_batch_ms=spread(lc))
    out["exact_route_whole_field_ms"] = out["lincomb_batch_ms"]["median"] * n / NB
    out["exact_route_over_selinv_pass"] = out["exact_route_whole_field_ms"] / max(out["selinv_pass_device_ms"]["median"], 1e-9)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--m", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--out", default=os.path.join("profiles", "selinv_timing.json"))
    a = ap.parse_args()
    res = []
    for n in a.n:
        res.append(one_size(n, a.m, a.rounds, a.batches))
        print(json.dumps(res[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
