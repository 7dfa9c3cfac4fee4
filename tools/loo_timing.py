"""Cost of gpv_plan_loo / gpv_plan_whiten_t (gpv_loo.hip) beside the whitening pass of the same columns and beside
the bytes the transposed pass must move:

    python tools/loo_timing.py [--n 1000000] [--m 30] [--rounds 7] [--reps 5] [--cols 1,4,16] [--out profiles/loo_timing.json]

One process, one plan (d = 2, cond.yz = 'z', maxmin ordering, Matern 1.5).  After a clock warm-up of likelihood evaluations (as
bench.py does) the legs run in alternating rounds; each is reported as the median over the rounds of the round's median, with
the smallest and largest round:
  index_build_ms     the one-off build of the transposed index (Plan.loo_index, first call: read-back, host build, upload), wall
  for every column count c:
    loo_ms[c]        the device passes of one gpv_plan_loo call alone (pack, forward, transposed, unpack, scores) over resident
                     columns, by an event pair around them (gpv_plan_debug_loo_ms)
    whiten_t_ms[c]   the same for gpv_plan_whiten_t (pack, transposed, unpack): the transposed pass
    whiten_ms[c]     the whitening pass with its Gram pass over the same columns (gpv_plan_debug_whiten_ms)
    stream_ms[c]     the bytes the transposed pass must move -- Lentries 8 n (m + 1), the transposed index 4 nnz + 8 n, g 8 n and
                     the columns in and out 16 n c -- at the device-to-device copy rate measured in the same run (copy_GBps:
                     bytes read + written per second)
Prints one JSON line and, with --out, writes it there."""
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


def summary(ts):
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cols", default="1,4,16")
    ap.add_argument("--out", default="")
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
    for name in ("gpv_plan_debug_whiten_ms", "gpv_plan_debug_loo_ms"):
        getattr(lib, name).argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]

    def passes(name, reps):
        ms = np.zeros(reps)
        L.check(getattr(lib, name)(plan._h, reps, L.dptr(ms)), name)
        return float(np.median(ms))
    for _ in range(30):                                               # clock warm-up
        plan.eval("matern", cp, nug, G.GPV_WANT_LOGLIK_Z)
        plan.sums()
    plan.eval("matern", cp, nug, G.GPV_WANT_U)
    plan.sums()
    t0 = time.perf_counter()
    nnz, longest, empty = plan.loo_index()
    t_index = 1e3 * (time.perf_counter() - t0)
    for c in cols:                                                    # first use: buffers, the scale pre-pass
        plan.whiten(Bord[:, :c])
        plan.loo(Bord[:, :c])
    rate = copy_rate()
    t_loo, t_wt, t_wh = ({c: [] for c in cols} for _ in range(3))
    for _ in range(a.rounds):
        for c in cols:
            Bc = np.asfortranarray(Bord[:, :c])
            plan.loo(Bc, want_mean=False, want_var=False)
            t_loo[c].append(passes("gpv_plan_debug_loo_ms", a.reps))  # (over the columns that call left on the device)
            plan.whiten_t(Bc)
            t_wt[c].append(passes("gpv_plan_debug_loo_ms", a.reps))
            plan.whiten(Bc)
            t_wh[c].append(passes("gpv_plan_debug_whiten_ms", a.reps))
    out = dict(n=n, m=m, rounds=a.rounds, reps=a.reps, index_entries=nnz, longest_column=longest, empty_columns=empty,
               index_build_ms=t_index, copy_GBps=rate / 1e9, loo_ms={}, whiten_t_ms={}, whiten_ms={}, stream_ms={},
               loo_over_whiten={}, whiten_t_over_whiten={}, whiten_t_over_stream={})
    for c in cols:
        s = 1e3 * (8.0 * n * (m + 1) + 4.0 * nnz + 16.0 * n + 16.0 * n * c) / rate
        out["loo_ms"][c], out["whiten_t_ms"][c], out["whiten_ms"][c] = summary(t_loo[c]), summary(t_wt[c]), summary(t_wh[c])
        out["stream_ms"][c] = s
        out["loo_over_whiten"][c] = out["loo_ms"][c]["median"] / out["whiten_ms"][c]["median"]
        out["whiten_t_over_whiten"][c] = out["whiten_t_ms"][c]["median"] / out["whiten_ms"][c]["median"]
        out["whiten_t_over_stream"][c] = out["whiten_t_ms"][c]["median"] / s
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
