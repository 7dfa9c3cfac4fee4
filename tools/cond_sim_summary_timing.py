"""Cost of gpv_plan_cond_sim_summary (gpv_csim_summary.hip) beside the route it replaces, in the setting of
tools/cond_sim_timing.py:

    python tools/cond_sim_summary_timing.py [--n 1000000] [--np 100000,1000000] [--m 30] [--ndraws 64] [--rounds 3]
                                            [--out profiles/cond_sim_summary_timing.json]

One process; one plan (d = 2, cond.yz = 'z', Matern 1.5, n uniform points in the unit square), the prediction locations a
regular raster in its max-min order.  After a clock warm-up of 40 likelihood evaluations the two routes run in alternating
rounds, per region layout ("one": one region of every pixel; "cells": runs of 10 pixels of the raster, n_p / 10 regions):
  device  Plan.cond_sim_summary(ndraws, one threshold, identity link): the draws stay on the device
  host    Plan.cond_sim(seed=, nsim=ndraws), the draws delivered, then the same folds in NumPy (moments and exceedance per pixel;
          total, max, min and area per region and draw)
Each figure is the median over the rounds with the smallest and largest:
  e2e_ms              wall time of the route (host: draws_ms for Plan.cond_sim + numpy_ms for the folds)
  per batch of 16     sweep_ms, fold_ms, copy_ms: device time by event pairs of the last batch's sweep (gpv_plan_debug_csim_ms), of
                      its folds and of the copies of its region block (gpv_plan_debug_csim_summary_ms)
  search_ms, factor_ms  of the device route's call, as tools/cond_sim_timing.py reports them
  peak_host_mb        the largest amount of host memory held in NumPy arrays during the route (tracemalloc; the library's own
                      host vectors, the same in both routes, are not in it)
The JSON is rewritten after every leg.  Prints the last JSON line."""
import argparse
import json
import os
import sys
import time
import tracemalloc

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (first: see tests/conftest.py)
import gpvecchia_amd as G  # noqa: E402
from gpvecchia_amd import _lib as L  # noqa: E402
from gpvecchia_amd import specify as S  # noqa: E402


def summary(ts):
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)))


def raster(n_p):
    side = int(np.ceil(np.sqrt(n_p)))
    g = (np.arange(side) + 0.5) / side
    return np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)[:n_p]


def numpy_folds(mean, dev, thr, regptr, regidx):
    """the folds of the device route on delivered draws (identity link, unit weights, every location live or NaN)"""
    Y = mean[:, None] + dev
    N = Y.shape[1]
    D = Y - mean[:, None]
    s1, s2 = D.sum(axis=1), (D * D).sum(axis=1)
    out = dict(mc_mean=mean + s1 / N, mc_var=np.maximum((s2 - s1 * s1 / N) / (N - 1), 0.0), exceed=(Y > thr).mean(axis=1))
    if regptr.size == 2:                                                  # one region of everything
        out.update(total=np.nansum(Y, axis=0)[None], max=np.nanmax(Y, axis=0)[None], min=np.nanmin(Y, axis=0)[None],
                   area=(Y > thr).sum(axis=0, dtype=np.float64)[None])
    else:
        Yr = Y[regidx]
        st = regptr[:-1]
        out.update(total=np.add.reduceat(np.nan_to_num(Yr), st, axis=0), max=np.fmax.reduceat(Yr, st, axis=0),
                   min=np.fmin.reduceat(Yr, st, axis=0), area=np.add.reduceat((Yr > thr).astype(np.float64), st, axis=0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--np", default="100000,1000000")
    ap.add_argument("--m", type=int, default=30)
    ap.add_argument("--ndraws", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, m, tau, nd, thr = a.n, a.m, 0.1, a.ndraws, 0.0
    lib = L.lib()
    out = dict(n=n, m=m, ndraws=nd, rounds=a.rounds, device=torch.cuda.get_device_name(0), np={})

    def flush():
        line = json.dumps(out)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
        return line

    rng = np.random.default_rng(n)
    locs = rng.random((n, 2))
    z = rng.standard_normal(n)
    cp = [1.0, 0.02 if n >= 500_000 else 0.05, 1.5]
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="z", nn_backend="gpu")
    plan = G.api._plan_for(va, 0)
    zord = np.ascontiguousarray(z[va["ord_z"] - 1])
    plan.set_data(zord)
    nug = np.array([tau])
    for i in range(40):                                                   # clock warm-up
        plan.eval("matern", cp, nug, G.GPV_WANT_LOGLIK_Z)
        plan.sums()
    tracemalloc.start()

    def device_route(q, csr):
        tracemalloc.reset_peak()
        t0 = time.perf_counter()
        r = plan.cond_sim_summary("matern", cp, tau, q, m, nd, seed=1, Z_ord=zord, thresholds=[thr], regions=csr)
        e2e = 1e3 * (time.perf_counter() - t0)
        peak = tracemalloc.get_traced_memory()[1] / 2 ** 20
        ms, fs = np.zeros(4), np.zeros(4)
        L.check(lib.gpv_plan_debug_csim_ms(plan._h, L.dptr(ms)), "gpv_plan_debug_csim_ms")
        L.check(lib.gpv_plan_debug_csim_summary_ms(plan._h, L.dptr(fs)), "gpv_plan_debug_csim_summary_ms")
        return dict(e2e_ms=e2e, search_ms=ms[0], factor_ms=ms[1], sweep_ms=ms[3], fold_ms=fs[1], copy_ms=fs[3], peak_host_mb=peak), r

    def host_route(q, csr):
        tracemalloc.reset_peak()
        t0 = time.perf_counter()
        r = plan.cond_sim("matern", cp, tau, q, m, Z_ord=zord, seed=1, nsim=nd)
        t1 = time.perf_counter()
        f = numpy_folds(r["mean"][:, 0], r["dev"], thr, csr[0], csr[1])
        t2 = time.perf_counter()
        peak = tracemalloc.get_traced_memory()[1] / 2 ** 20
        return dict(e2e_ms=1e3 * (t2 - t0), draws_ms=1e3 * (t1 - t0), numpy_ms=1e3 * (t2 - t1), peak_host_mb=peak), f

    for n_p in [int(x) for x in a.np.split(",") if x]:
        q = raster(n_p)
        o = S.order_maxmin_exact(q) - 1
        q = np.asfortranarray(q[o])
        pos = np.empty(n_p, dtype=np.int64)
        pos[o] = np.arange(n_p)
        cells = np.sort(pos[: n_p // 10 * 10].reshape(-1, 10), axis=1)    # runs of 10 raster pixels, members in ascending sweep row
        layouts = dict(one=(np.array([0, n_p], dtype=np.int64), np.arange(n_p, dtype=np.int32), None),
                       cells=(np.arange(0, cells.size + 1, 10, dtype=np.int64), cells.reshape(-1).astype(np.int32), None))
        device_route(q[:4096], (np.array([0, 4096], dtype=np.int64), np.arange(4096, dtype=np.int32), None))      # first use: code objects
        run = {}
        out["np"][n_p] = run
        for name, csr in layouts.items():
            t = dict(device={}, host={})
            for _ in range(a.rounds):
                d, rd = device_route(q, csr)
                h, fh = host_route(q, csr)
                for k, v in d.items():
                    t["device"].setdefault(k, []).append(v)
                for k, v in h.items():
                    t["host"].setdefault(k, []).append(v)
            agree = float(np.nanmax(np.abs(rd["reg_total"] - fh["total"]) / np.maximum(1.0, np.abs(fh["total"]))))
            run[name] = dict(nreg=int(csr[0].size - 1), device={k: summary(v) for k, v in t["device"].items()},
                             host={k: summary(v) for k, v in t["host"].items()}, levels=rd["n_levels"], launches=rd["n_launches"],
                             n_failed=rd["n_failed"], batches=(nd + 15) // 16, total_rel_diff=agree,
                             max_equal=bool(np.array_equal(rd["reg_max"], fh["max"], equal_nan=True)))
            flush()
    print(flush())


if __name__ == "__main__":
    main()
