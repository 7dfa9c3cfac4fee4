"""Cost of gpv_plan_cond_sim (gpv_csim.hip): conditional simulation of a map under a cond.yz='z' model by the
sequential kriging sweep, beside the local-kriging pass over the same locations (gpv_plan_krige, §4s) and beside the colouring
sweep of a plan with as many rows (gpv_plan_unwhiten, §4n):

    python tools/cond_sim_timing.py [--n 1000000] [--np 100000,1000000] [--m 30] [--rounds 3] [--order maxmin]
                                    [--out profiles/cond_sim_timing.json]

One process; per n one plan (d = 2, cond.yz = 'z', Matern 1.5, uniform points in the unit square), the prediction locations a
regular raster over it, swept in the max-min order of the raster.  After a clock warm-up of 40 likelihood evaluations (as
bench.py does) the legs run in alternating rounds; each figure is the median over the rounds, with the smallest and largest:
  order_s             host time of the max-min ordering of the raster (once)
  per call (gpv_plan_debug_csim_ms; device times by event pairs):
    search_ms         the ordered search on [observations ; raster], host clock around it (coordinates down, index, kernels, lists back)
    factor_ms[R]      device time of the factor pass with R data columns
    sweep_ms[CP]      device time of ONE sweep at the padded column count CP: the means of R = 1 (CP = 1) and R = 16 (CP = 16)
    draws16_ms        device time of the sweep of one batch of 16 seeded draws; normals16_e2e_ms: the wall time 16 draws add to a call
    e2e_ms            wall time of Plan.cond_sim (R = 1, no draws | R = 1, 16 draws)
  krige_pass_ms[R]    device time of the gpv_plan_krige pass over the same locations at the same m (gpv_plan_debug_krige_ms)
  unwhiten_ms[CP]     device time of the colouring sweep of a 'z' plan with n_p rows at m (gpv_plan_debug_unwhiten_ms), its
                      levels and launches
  levels, launches    of the sweep
  ratios              factor / krige pass; sweep / unwhiten sweep
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
from gpvecchia_amd import specify as S  # noqa: E402


def summary(ts):
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)))


def raster(n_p):
    side = int(np.ceil(np.sqrt(n_p)))
    g = (np.arange(side) + 0.5) / side
    return np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)[:n_p]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1000000")
    ap.add_argument("--np", default="100000,1000000")
    ap.add_argument("--m", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--order", default="maxmin", choices=["maxmin", "given"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ns = [int(x) for x in a.n.split(",") if x]
    nps = [int(x) for x in a.np.split(",") if x]
    m, tau = a.m, 0.1
    lib = L.lib()
    lib.gpv_plan_debug_krige_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    lib.gpv_plan_debug_unwhiten_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    out = dict(m=m, rounds=a.rounds, order=a.order, device=torch.cuda.get_device_name(0), runs={})

    def flush():
        line = json.dumps(out)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
        return line

    def z_plan(locs):
        va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="z", nn_backend="gpu")
        return va, G.api._plan_for(va, 0)

    for n in ns:
        rng = np.random.default_rng(n)
        locs = rng.random((n, 2))
        Z = rng.standard_normal((n, 16))
        cp = [1.0, 0.02 if n >= 500_000 else 0.05, 1.5]
        t0 = time.perf_counter()
        va, plan = z_plan(locs)
        run = dict(specify_s=time.perf_counter() - t0, np={})
        out["runs"][n] = run
        Zord = np.asfortranarray(Z[va["ord_z"] - 1])
        plan.set_data(Zord[:, 0])
        nug = np.array([tau])
        for i in range(40):                                               # clock warm-up
            plan.eval("matern", cp, nug, G.GPV_WANT_LOGLIK_Z)
            plan.sums()
        flush()

        def csim(q, R, nsim):
            t0 = time.perf_counter()
            r = plan.cond_sim("matern", cp, tau, q, m, Z_ord=Zord[:, :R], seed=1, nsim=nsim)
            e2e = 1e3 * (time.perf_counter() - t0)
            ms = np.zeros(4)
            L.check(lib.gpv_plan_debug_csim_ms(plan._h, L.dptr(ms)), "gpv_plan_debug_csim_ms")
            return e2e, ms, r

        def krige(q, R):
            plan.krige("matern", cp, tau, q, m, Z_ord=Zord[:, :R])
            ms = np.zeros(2)
            L.check(lib.gpv_plan_debug_krige_ms(plan._h, L.dptr(ms)), "gpv_plan_debug_krige_ms")
            return ms[1]

        for n_p in nps:
            q = raster(n_p)
            t0 = time.perf_counter()
            if a.order == "maxmin":
                q = q[S.order_maxmin_exact(q) - 1]
            r = dict(order_s=time.perf_counter() - t0)
            q = np.asfortranarray(q)
            csim(q[:4096], 1, 16)                                         # first use: code objects
            csim(q[:4096], 16, 0)
            krige(q[:4096], 1)
            krige(q[:4096], 16)
            t = {k: [] for k in ("search_ms", "factor_ms_1", "factor_ms_16", "sweep_ms_1", "sweep_ms_16", "draws16_ms", "e2e_ms_means",
                                 "e2e_ms_16draws", "krige_pass_ms_1", "krige_pass_ms_16")}
            for _ in range(a.rounds):
                e2e, ms, res = csim(q, 1, 0)
                t["search_ms"].append(ms[0]); t["factor_ms_1"].append(ms[1]); t["sweep_ms_1"].append(ms[3]); t["e2e_ms_means"].append(e2e)
                e2e, ms, res = csim(q, 16, 0)
                t["factor_ms_16"].append(ms[1]); t["sweep_ms_16"].append(ms[3])
                e2e, ms, res = csim(q, 1, 16)
                t["draws16_ms"].append(ms[3]); t["e2e_ms_16draws"].append(e2e)
                t["krige_pass_ms_1"].append(krige(q, 1))
                t["krige_pass_ms_16"].append(krige(q, 16))
            r.update({k: summary(v) for k, v in t.items()})
            r.update(levels=res["n_levels"], launches=res["n_launches"], n_failed=res["n_failed"])
            r["normals16_e2e_ms"] = r["e2e_ms_16draws"]["median"] - r["e2e_ms_means"]["median"]
            run["np"][n_p] = r
            flush()
            # the colouring sweep of a plan with n_p rows
            if n_p == n:
                up, uZ = plan, Zord
            else:
                ulocs = np.random.default_rng(n_p).random((n_p, 2))
                uva, up = z_plan(ulocs)
                uZ = np.asfortranarray(np.random.default_rng(1).standard_normal((n_p, 16)))
                up.set_data(uZ[:, 0])
            up.eval("matern", cp, nug, G.GPV_WANT_U | G.GPV_WANT_LOGLIK_Z)
            up.sums()
            r["unwhiten_levels"], r["unwhiten_launches"] = up.unwhiten_levels()
            for CP in (1, 16):
                up.unwhiten(uZ[:, :CP])
                ts = []
                for _ in range(a.rounds):
                    ms1 = C.c_double(0.0)
                    L.check(lib.gpv_plan_debug_unwhiten_ms(up._h, 1, C.byref(ms1)), "gpv_plan_debug_unwhiten_ms")
                    ts.append(ms1.value)
                r[f"unwhiten_ms_{CP}"] = summary(ts)
            r["ratios"] = dict(factor_over_krige_1=r["factor_ms_1"]["median"] / r["krige_pass_ms_1"]["median"],
                               factor_over_krige_16=r["factor_ms_16"]["median"] / r["krige_pass_ms_16"]["median"],
                               sweep_over_unwhiten_1=r["sweep_ms_1"]["median"] / r["unwhiten_ms_1"]["median"],
                               sweep_over_unwhiten_16=r["sweep_ms_16"]["median"] / r["unwhiten_ms_16"]["median"])
            r["factor_ns_per_location"] = 1e6 * r["factor_ms_1"]["median"] / n_p
            r["krige_ns_per_location"] = 1e6 * r["krige_pass_ms_1"]["median"] / n_p
            flush()
            if up is not plan:
                del up, uva
    print(flush())


if __name__ == "__main__":
    main()
