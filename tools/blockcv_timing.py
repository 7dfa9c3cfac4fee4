"""Cost of gpv_plan_block_cv (gpv_blockcv.hip) beside gpv_plan_loo on the same plan and columns in the same process:

    python tools/blockcv_timing.py [--n 1000000] [--m 30] [--rounds 7] [--reps 5] [--cols 1,4,16] [--out profiles/blockcv_timing.json]

One process, one plan (d = 2, cond.yz = 'z', maxmin ordering, Matern 1.5), the blocks the cells of spatial_blocks (at most 64
points).  After a clock warm-up of likelihood evaluations (as bench.py does) the legs run in alternating rounds; each is
reported as the median over the rounds of the round's median, with the smallest and largest round:
  spatial_blocks_ms  the host bisection that makes the labels, wall
  set_blocks_ms      the one-off gpv_plan_set_blocks (read-back of the index arrays, host build of the block index, upload), wall
  n_blocks, n_heldout, max_size, n_set_refs, set_refs_per_location
  for every column count c:
    block_cv_ms[c]   the device passes of one gpv_plan_block_cv call alone over resident columns, by an event pair around them
                     (gpv_plan_debug_blockcv_ms): r = Q z, the fills and the block pass, unpack and scores
    qz_ms / blocks_ms / scores_ms [c]   the three parts by event pairs of their own (the block pass is ONE kernel: assembly and
                     factor + solves are not separable from outside it)
    loo_ms[c]        the device passes of one gpv_plan_loo call (gpv_plan_debug_loo_ms): the yardstick
    block_cv_over_loo[c]
Prints one JSON line and, with --out, writes it there."""
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
    lib.gpv_plan_debug_loo_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    lib.gpv_plan_debug_blockcv_ms.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]

    def loo_passes(reps):
        ms = np.zeros(reps)
        L.check(lib.gpv_plan_debug_loo_ms(plan._h, reps, L.dptr(ms)), "gpv_plan_debug_loo_ms")
        return float(np.median(ms))

    def bcv_passes(reps, parts):
        ms = np.zeros(reps)
        L.check(lib.gpv_plan_debug_blockcv_ms(plan._h, reps, parts, L.dptr(ms)), "gpv_plan_debug_blockcv_ms")
        return float(np.median(ms))
    for _ in range(30):                                               # clock warm-up
        plan.eval("matern", cp, nug, G.GPV_WANT_LOGLIK_Z)
        plan.sums()
    plan.eval("matern", cp, nug, G.GPV_WANT_U)
    plan.sums()
    t0 = time.perf_counter()
    lab = G.spatial_blocks(va["locsord"]).astype(np.int32)
    t_labels = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    n_blocks, n_heldout, max_size, n_refs = plan.set_blocks(lab)
    t_set = 1e3 * (time.perf_counter() - t0)
    n_bad = 0
    for c in cols:                                                    # first use: buffers, the transposed index, the scale pre-pass
        plan.loo(Bord[:, :c])
        n_bad = max(n_bad, plan.block_cv(Bord[:, :c])[4])
    keys = ("block_cv_ms", "qz_ms", "blocks_ms", "scores_ms", "loo_ms")
    t = {k: {c: [] for c in cols} for k in keys}
    for _ in range(a.rounds):
        for c in cols:
            Bc = np.asfortranarray(Bord[:, :c])
            plan.block_cv(Bc, want_mean=False, want_var=False)
            t["block_cv_ms"][c].append(bcv_passes(a.reps, 7))         # (over the columns that call left on the device)
            t["qz_ms"][c].append(bcv_passes(a.reps, 1))
            t["blocks_ms"][c].append(bcv_passes(a.reps, 2))
            t["scores_ms"][c].append(bcv_passes(a.reps, 4))
            plan.loo(Bc, want_mean=False, want_var=False)
            t["loo_ms"][c].append(loo_passes(a.reps))
    out = dict(n=n, m=m, rounds=a.rounds, reps=a.reps, spatial_blocks_ms=t_labels, set_blocks_ms=t_set, n_blocks=n_blocks,
               n_heldout=n_heldout, max_size=max_size, n_set_refs=n_refs, set_refs_per_location=n_refs / n, n_bad_blocks=n_bad,
               block_cv_over_loo={}, blocks_share={}, **{k: {} for k in keys})
    for c in cols:
        for k in keys:
            out[k][c] = summary(t[k][c])
        out["block_cv_over_loo"][c] = out["block_cv_ms"][c]["median"] / out["loo_ms"][c]["median"]
        out["blocks_share"][c] = out["blocks_ms"][c]["median"] / out["block_cv_ms"][c]["median"]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
