"""Cost of gpv_plan_krige (gpv_krige.hip): the map of a cond.yz='z' model by local kriging, beside a likelihood-only
evaluation of the same plan (the floor for one set solve) and beside the other route to a map, vecchia_prediction on a 'zy'
plan with prediction locations:

    python tools/krige_timing.py [--n 100000,1000000] [--np 100000,1000000,10000000] [--m 30] [--rounds 3] [--zy-np 10000,100000]
                                 [--ordering maxmin] [--out profiles/krige_timing.json]

One process; per n one plan (d = 2, cond.yz = 'z', Matern 1.5, uniform points in the unit square, the prediction locations a
regular raster over it).  After a clock warm-up of likelihood evaluations (as bench.py does) the legs run in alternating
rounds (R = 1, R = 16 for every n_p); each figure is the median over the rounds, with the smallest and largest round:
  lik_ms            kernel time of one likelihood-only evaluation of the plan (n sets): lik_ms / n is the floor for one set solve
  per n_p:
    search_ms       device time of the searches of one call, summed over its chunks (event pairs: gpv_plan_debug_krige_ms)
    pass_ms[R]      device time of the predict passes of one call of R columns, the same way
    e2e_ms[R]       wall time of Plan.krige: host re-layout, the index of the search, transfers both ways, searches and passes
    pass_over_floor[R]   (pass_ms / n_p) / (lik_ms / n)
  zy (only for the n named first, and only the n_p of --zy-np): wall time of vecchia_specify(locs_pred=) and of
    vecchia_prediction(return_values='meanvar') on the (2 n + n_p)-row 'zy' plan, the route vecchia_pred takes by default
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


def raster(n_p):
    side = int(np.ceil(np.sqrt(n_p)))
    g = (np.arange(side) + 0.5) / side
    return np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)[:n_p]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="100000,1000000")
    ap.add_argument("--np", default="100000,1000000,10000000")
    ap.add_argument("--m", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--zy-np", default="10000,100000")
    ap.add_argument("--ordering", default="maxmin")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ns = [int(x) for x in a.n.split(",") if x]
    nps = [int(x) for x in a.np.split(",") if x]
    zy_nps = [int(x) for x in a.zy_np.split(",") if x]
    m, tau = a.m, 0.1
    lib = L.lib()
    lib.gpv_plan_debug_krige_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    out = dict(m=m, rounds=a.rounds, ordering=a.ordering, device=torch.cuda.get_device_name(0), runs={}, zy={})

    def flush():
        line = json.dumps(out)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
        return line

    for n in ns:
        rng = np.random.default_rng(n)
        locs = rng.random((n, 2))
        Z = rng.standard_normal((n, 16))
        cp = [1.0, 0.02 if n >= 500_000 else 0.05, 1.5]
        t0 = time.perf_counter()
        va = G.vecchia_specify(locs, m, ordering=a.ordering, cond_yz="z", nn_backend="gpu")
        run = dict(specify_s=time.perf_counter() - t0, np={})
        out["runs"][n] = run
        plan = G.api._plan_for(va, 0)
        Zord = np.asfortranarray(Z[va["ord_z"] - 1])
        plan.set_data(Zord[:, 0])
        nug = np.array([tau])
        lik = []
        for i in range(40):                                               # clock warm-up, then the floor
            plan.eval("matern", cp, nug, G.GPV_WANT_LOGLIK_Z)
            plan.sums()
            if i >= 30:
                lik.append(plan.last_kernel_ms())
        run["lik_ms"] = summary(lik)
        flush()

        def leg(q, R):
            t0 = time.perf_counter()
            _, _, nf = plan.krige("matern", cp, tau, q, m, Z_ord=Zord[:, :R])
            e2e = 1e3 * (time.perf_counter() - t0)
            ms = np.zeros(2)
            L.check(lib.gpv_plan_debug_krige_ms(plan._h, L.dptr(ms)), "gpv_plan_debug_krige_ms")
            return e2e, ms[0], ms[1], nf
        for n_p in nps:
            q = np.asfortranarray(raster(n_p))
            leg(q[:4096], 1)                                              # first use: code objects
            leg(q[:4096], 16)
            t = {k: [] for k in ("search_ms", "pass_ms_1", "pass_ms_16", "e2e_ms_1", "e2e_ms_16")}
            n_failed = 0
            for _ in range(a.rounds):
                for R in (1, 16):
                    e2e, s_ms, p_ms, nf = leg(q, R)
                    t["search_ms"].append(s_ms)
                    t[f"pass_ms_{R}"].append(p_ms)
                    t[f"e2e_ms_{R}"].append(e2e)
                    n_failed = max(n_failed, nf)
            r = {k: summary(v) for k, v in t.items()}
            floor = run["lik_ms"]["median"] / n
            r["n_failed"] = n_failed
            r["pass_over_floor"] = {R: r[f"pass_ms_{R}"]["median"] / n_p / floor for R in (1, 16)}
            run["np"][n_p] = r
            flush()
        if n == ns[0]:                                                    # the default route of vecchia_pred, for comparison
            from gpvecchia_amd.laplace import vecchia_prediction
            for n_p in zy_nps:
                q = raster(n_p) + 1e-7                                    # (off the observations: the route refuses coincident points)
                t0 = time.perf_counter()
                vz = G.vecchia_specify(locs, m, locs_pred=q)
                t1 = time.perf_counter()
                vecchia_prediction(Z[:, 0], vz, cp, tau, covmodel="matern", return_values="meanvar")
                t2 = time.perf_counter()
                out["zy"][n_p] = dict(n=n, rows=int(vz["locsord"].shape[0]), specify_s=t1 - t0, prediction_s=t2 - t1)
                del vz
                flush()
    print(flush())


if __name__ == "__main__":
    main()
