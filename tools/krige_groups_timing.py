"""Cost of gpv_plan_krige_groups (gpv_krige_groups.hip) beside gpv_plan_krige over the same pixels:

    python tools/krige_groups_timing.py [--n 1000000] [--side 1000,3160] [--cells 2,4,5] [--m 30] [--rounds 3]
                                        [--ordering maxmin] [--out profiles/krige_groups_timing.json]

One process; one plan (d = 2, cond.yz = 'z', Matern 1.5, uniform points in the unit square); the prediction locations a regular
side x side raster over it (side a multiple of every cell edge), grouped in c x c cells, the members of a cell contiguous.  After
a clock warm-up of likelihood evaluations (as bench.py does) the legs run in alternating rounds: the per-pixel pass (the
yardstick), then every cell edge without and with the packed covariances; each figure is the median over the rounds, with the
smallest and largest round:
  pixel                search_ms, pass_ms (device time by event pairs, summed over the call's chunks: gpv_plan_debug_krige_ms),
                       e2e_ms (wall time of Plan.krige), one data column
  cells[c][cov]        the same of Plan.krige_groups, and ns per pixel and per group of the pass
  mean_shift_sd        (only at the first side) how far the grouped per-pixel means lie from the per-pixel means, in predictive
                       standard deviations of the per-pixel call: max and root mean square.  Another conditioning set: no bar
The JSON is rewritten after every leg, so a run that is cut short leaves what it measured.  Prints the last JSON line."""
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


def cell_raster(side, c):
    """the side x side raster with the pixels of a c x c cell contiguous: (locations (side^2, 2), for each its raster index)"""
    i = np.arange(side)
    I, J = np.meshgrid(i, i, indexing="ij")
    idx = (I * side + J).reshape(side // c, c, side // c, c).transpose(0, 2, 1, 3).reshape(-1)
    g = (i + 0.5) / side
    return np.stack([g[idx // side], g[idx % side]], axis=1), idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--side", default="1000,3160")
    ap.add_argument("--cells", default="2,4,5")
    ap.add_argument("--m", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ordering", default="maxmin")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sides = [int(x) for x in a.side.split(",") if x]
    cells = [int(x) for x in a.cells.split(",") if x]
    n, m, tau = a.n, a.m, 0.1
    lib = L.lib()
    lib.gpv_plan_debug_krige_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    out = dict(n=n, m=m, rounds=a.rounds, ordering=a.ordering, device=torch.cuda.get_device_name(0), sides={})

    def flush():
        line = json.dumps(out)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
        return line

    rng = np.random.default_rng(n)
    locs = rng.random((n, 2))
    cp = [1.0, 0.02 if n >= 500_000 else 0.05, 1.5]
    t0 = time.perf_counter()
    va = G.vecchia_specify(locs, m, ordering=a.ordering, cond_yz="z", nn_backend="gpu")
    out["specify_s"] = time.perf_counter() - t0
    z = G.vecchia_simulate(va, cp, tau, seed=1)[:, 0]                      # data of the model itself: mean_shift_sd means something
    plan = G.api._plan_for(va, 0)
    zord = np.ascontiguousarray(z[va["ord_z"] - 1])
    plan.set_data(zord)
    nug = np.array([tau])
    lik = []
    for i in range(40):                                                   # clock warm-up
        plan.eval("matern", cp, nug, G.GPV_WANT_LOGLIK_Z)
        plan.sums()
        if i >= 30:
            lik.append(plan.last_kernel_ms())
    out["lik_ms"] = summary(lik)
    flush()

    def device_ms():
        ms = np.zeros(2)
        L.check(lib.gpv_plan_debug_krige_ms(plan._h, L.dptr(ms)), "gpv_plan_debug_krige_ms")
        return ms

    def pixel_leg(q):
        t0 = time.perf_counter()
        mean, var, nf = plan.krige("matern", cp, tau, q, m, Z_ord=zord)
        e2e = 1e3 * (time.perf_counter() - t0)
        ms = device_ms()
        return dict(e2e_ms=e2e, search_ms=ms[0], pass_ms=ms[1]), nf, mean, var

    def group_leg(q, gptr, cov):
        t0 = time.perf_counter()
        res = plan.krige_groups("matern", cp, tau, q, gptr, m, Z_ord=zord, want_cov=cov)
        e2e = 1e3 * (time.perf_counter() - t0)
        ms = device_ms()
        return dict(e2e_ms=e2e, search_ms=ms[0], pass_ms=ms[1]), res[5], res[0]

    for si, side in enumerate(sides):
        if any(side % c for c in cells):
            raise SystemExit(f"side {side} is no multiple of every cell edge {cells}")
        n_p = side * side
        run = dict(n_p=n_p, cells={})
        out["sides"][side] = run
        q1, _ = cell_raster(side, 1)
        q1 = np.asfortranarray(q1)
        lay = {c: cell_raster(side, c) for c in cells}
        gp = {c: np.arange(0, n_p + 1, c * c, dtype=np.int64) for c in cells}
        pixel_leg(q1[:4096])                                              # first use: code objects
        for c in cells:
            group_leg(lay[c][0][:4096 // (c * c) * c * c], gp[c][:4096 // (c * c) + 1], True)
        tp = {k: [] for k in ("e2e_ms", "search_ms", "pass_ms")}
        tg = {(c, cov): {k: [] for k in tp} for c in cells for cov in (False, True)}
        failed = 0
        ref = None
        for r in range(a.rounds):
            t, nf, mean, var = pixel_leg(q1)
            failed = max(failed, nf)
            for k in tp:
                tp[k].append(t[k])
            if si == 0 and r == 0:
                ref = (mean[:, 0].copy(), np.sqrt(var))
            for c in cells:
                for cov in (False, True):
                    t, nf, gmean = group_leg(lay[c][0], gp[c], cov)
                    failed = max(failed, nf)
                    for k in tp:
                        tg[(c, cov)][k].append(t[k])
                    if ref is not None and r == 0 and not cov:
                        d = (gmean[:, 0] - ref[0][lay[c][1]]) / ref[1][lay[c][1]]
                        run.setdefault("mean_shift_sd", {})[c] = dict(max=float(np.abs(d).max()), rms=float(np.sqrt(np.mean(d * d))))
        run["pixel"] = {k: summary(v) for k, v in tp.items()}
        run["pixel"]["pass_ns_per_pixel"] = 1e6 * run["pixel"]["pass_ms"]["median"] / n_p
        for (c, cov), t in tg.items():
            s = {k: summary(v) for k, v in t.items()}
            s["pass_ns_per_pixel"] = 1e6 * s["pass_ms"]["median"] / n_p
            s["pass_ns_per_group"] = 1e6 * s["pass_ms"]["median"] / (n_p // (c * c))
            s["search_ns_per_group"] = 1e6 * s["search_ms"]["median"] / (n_p // (c * c))
            run["cells"].setdefault(c, {})["cov" if cov else "nocov"] = s
        run["n_failed"] = failed
        flush()
    print(flush())


if __name__ == "__main__":
    main()
