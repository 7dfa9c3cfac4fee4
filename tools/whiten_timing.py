"""Cost of gpv_plan_whiten (gpv_whiten.hip) beside the evaluation that feeds it and beside the bytes it must move:

    python tools/whiten_timing.py [--n 1000000] [--m 30] [--rounds 7] [--reps 5] [--cols 1,4,16]

One process, one plan (d = 2, cond.yz = 'z', maxmin ordering, Matern 1.5).  After a clock warm-up of likelihood evaluations (as
bench.py does) the legs run in alternating rounds and each is reported as the median over the rounds of the round's median:
  eval_U_ms          plan.eval(GPV_WANT_U) + sums(): the evaluation that leaves the factor in HBM, wall clock
  for every column count c:
    pass_ms[c]       the two device passes alone (whitening, Gram with its fixed-order sum) over resident columns, by an event
                     pair around them (gpv_plan_debug_whiten_ms): what compares with the evaluation's kernel
    call_ms[c]       one blocking Plan.whiten call, wall clock: the passes plus the columns' trip over PCIe and their packing
    stream_ms[c]     the bytes the pass must move -- Lentries, the neighbour indices and E, n ((m + 1) (8 + 4) + 8 c) -- at the
                     device-to-device copy rate measured in the same run (copy_GBps: bytes read + written per second)
  profile_ms / loglik_ms   one vecchia_profile_likelihood call (constant and x1 trend: 3 columns) against one
                     vecchia_likelihood call of the same data, wall clock
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: see tests/conftest.py)
import gpvecchia_amd as G  # noqa: E402
from gpvecchia_amd import _lib as L  # noqa: E402


def med(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def copy_rate():
    """device-to-device copy of 256 MiB: (bytes read + bytes written) / second, median of 9 after 3 warm-up copies"""
    a = torch.empty(1 << 25, dtype=torch.float64, device="cuda")
    b = torch.empty_like(a)
    ts = []
    for i in range(12):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append(e0.elapsed_time(e1))
    return 2.0 * a.numel() * 8 / (1e-3 * float(np.median(ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cols", default="1,4,16")
    a = ap.parse_args()
    n, m = a.n, a.m
    cols = [int(c) for c in a.cols.split(",")]
    rng = np.random.default_rng(0)
    locs = rng.random((n, 2))
    z = rng.standard_normal(n)
    Bord = np.asfortranarray(rng.standard_normal((n, max(cols))))
    cp, tau = [1.0, 0.02 if n >= 500_000 else 0.05, 1.5], 0.1
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="z", nn_backend="gpu")
    plan = G.api._plan_for(va, 0)
    plan.set_data(z[va["ord_z"] - 1])
    nug = np.array([tau])
    lib = L.lib()
    lib.gpv_plan_debug_whiten_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]

    def lik():
        plan.eval("matern", cp, nug, G.GPV_WANT_LOGLIK_Z)
        return plan.sums()

    def eval_u():
        plan.eval("matern", cp, nug, G.GPV_WANT_U)
        return plan.sums()

    def passes(reps):
        ms = np.zeros(reps)
        L.check(lib.gpv_plan_debug_whiten_ms(plan._h, reps, L.dptr(ms)), "gpv_plan_debug_whiten_ms")
        return float(np.median(ms))
    for _ in range(30):                                               # clock warm-up
        lik()
    eval_u()
    for c in cols:                                                    # first use: buffers
        plan.whiten(Bord[:, :c])
    rate = copy_rate()
    t_eval, t_pass, t_call = [], {c: [] for c in cols}, {c: [] for c in cols}
    for _ in range(a.rounds):
        t_eval.append(med(eval_u, a.reps))
        for c in cols:
            Bc = np.asfortranarray(Bord[:, :c])
            t_call[c].append(med(lambda: plan.whiten(Bc), a.reps))
            t_pass[c].append(passes(a.reps))                          # (over the columns that call left on the device)
    X = np.column_stack([np.ones(n), locs[:, 0]])
    G.vecchia_profile_likelihood(z, X, va, cp, tau)
    G.vecchia_likelihood(z, va, cp, tau)
    t_prof, t_lik = [], []
    for _ in range(a.rounds):
        t_prof.append(med(lambda: G.vecchia_profile_likelihood(z, X, va, cp, tau), 3))
        t_lik.append(med(lambda: G.vecchia_likelihood(z, va, cp, tau), 3))
    ev = float(np.median(t_eval))
    out = dict(n=n, m=m, rounds=a.rounds, reps=a.reps, eval_U_ms=ev, eval_U_ms_rounds=[round(t, 4) for t in t_eval],
               copy_GBps=rate / 1e9, pass_ms={}, call_ms={}, stream_ms={}, pass_over_eval={}, pass_over_stream={},
               profile_ms=float(np.median(t_prof)), loglik_ms=float(np.median(t_lik)))
    for c in cols:
        p = float(np.median(t_pass[c]))
        s = 1e3 * n * ((m + 1) * 12 + 8 * c) / rate
        out["pass_ms"][c], out["call_ms"][c], out["stream_ms"][c] = p, float(np.median(t_call[c])), s
        out["pass_over_eval"][c], out["pass_over_stream"][c] = p / ev, p / s
    out["profile_over_loglik"] = out["profile_ms"] / out["loglik_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
