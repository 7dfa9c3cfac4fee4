"""Cost of gpv_plan_lincomb (gpv_lincomb.hip): ms per batch of NB solves, beside
  (a) ONE mean sweep of the same plan (GPV_WANT_MEAN minus GPV_WANT_DENOM evaluation time: the same level structure for one
      right-hand side), and
  (b) scipy's spsolve_triangular for the same NB right-hand sides on the oracle's V on the host (--host; n <= 1e5).

    python tools/lincomb_timing.py [--n 1000000] [--m 30] [--batches 8] [--host] [--pred] [--summary]

The transposed solve (gpv_plan_solve_t, posterior draws) is timed twice: the sweep alone on the device (a pair of events around
the captured graph, gpv_plan_debug_solve_t_ms), which is what compares with one mean sweep and with one lincomb batch, and the
whole call per batch, which at n = 1e6 is mostly the 2 x 256 MB of the batch crossing PCIe from and to pageable memory.  These
legs are measured in --rounds alternating rounds (mean evaluation, denominator evaluation, lincomb, transposed sweep, ...) and
reported as medians over the rounds.

--summary: the Monte-Carlo summaries (gpv_plan_draws_summary: normals made on the device, the same sweep, sums folded on the
device) in alternating rounds of their own with the parent route they replace: (i) the device time per batch of fill, sweep
and accumulation between events (gpv_plan_debug_draws_ms), (ii) the wall time per batch of the call (96 draws minus 32 draws,
halved), beside the sweep alone and gpv_plan_solve_t per batch from the same rounds.

Times are wall clock around the blocking calls after a clock warm-up of evaluations (as bench.py does); the lincomb call is
timed with 1 and with 1 + batches batches and the difference divided, so that the upload of H and the call's fixed cost drop out.
--pred: also vecchia_prediction(..., 'meanvar') at 4e4 + 1e4 locations.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (first: see tests/conftest.py)
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
    import scipy.sparse as sp
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=30)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--pred", action="store_true")
    ap.add_argument("--summary", action="store_true")
    a = ap.parse_args()
    NB = L.lib().gpv_lincomb_batch()
    n, m = a.n, a.m
    locs = np.random.default_rng(0).random((n, 2))
    z = np.random.default_rng(1).standard_normal(n)
    cp, tau = [1.0, 0.02 if n >= 500_000 else 0.05, 1.5], 0.1
    va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="SGV", nn_backend="gpu")
    plan = G.api._plan_for(va, 0)
    assert plan.ensure_posterior()
    plan.set_data(z[va["ord_z"] - 1])
    nug = np.array([tau])

    def ev(flags):
        plan.eval("matern", cp, nug, flags)
        plan.sums()
    for _ in range(30):                                               # clock warm-up
        ev(G.GPV_WANT_MEAN)
    t_mean, t_den = med(lambda: ev(G.GPV_WANT_MEAN), 15), med(lambda: ev(G.GPV_WANT_DENOM), 15)
    ev(G.GPV_WANT_MEAN)
    rng = np.random.default_rng(2)

    def H(nb):
        rows = nb * NB
        idx = rng.choice(n, rows, replace=False)
        return sp.csr_matrix((np.ones(rows), idx, np.arange(rows + 1)), shape=(rows, n))
    H1, Hk = H(1), H(1 + a.batches)
    plan.lincomb(H1)                                                  # first use: records, X, graph
    t1, tk = med(lambda: plan.lincomb(H1), a.reps), med(lambda: plan.lincomb(Hk), a.reps)
    per_batch = (tk - t1) / a.batches
    out = dict(n=n, m=m, NB=NB, levels=plan.posterior_levels(), eval_mean_ms=t_mean, eval_denom_ms=t_den,
               one_mean_sweep_ms=t_mean - t_den, lincomb_first_batch_call_ms=t1, lincomb_ms_per_batch=per_batch,
               lincomb_ms_per_solve=per_batch / NB, batch_over_single_sweep=per_batch / max(t_mean - t_den, 1e-9),
               X_bytes=n * NB * 8)
    # the transposed sweep, in alternating rounds with what it is compared to
    import ctypes as C
    lib = L.lib()
    lib.gpv_plan_debug_solve_t_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    E1 = rng.standard_normal((NB, n))
    Ek = np.ascontiguousarray(np.broadcast_to(E1, (3, NB, n)).reshape(3 * NB, n))
    plan.solve_t(E1)                                                  # first use: staging buffers, graph
    one = np.zeros(1)

    def sweep_ms():
        L.check(lib.gpv_plan_debug_solve_t_ms(plan._h, 1, L.dptr(one)), "gpv_plan_debug_solve_t_ms")
        return float(one[0])
    legs = dict(mean=[], denom=[], lc1=[], lck=[], st_sweep=[], st1=[], stk=[])
    for _ in range(a.rounds):
        legs["mean"].append(med(lambda: ev(G.GPV_WANT_MEAN), 1))
        legs["denom"].append(med(lambda: ev(G.GPV_WANT_DENOM), 1))
        ev(G.GPV_WANT_MEAN)
        legs["lc1"].append(med(lambda: plan.lincomb(H1), 1))
        legs["lck"].append(med(lambda: plan.lincomb(Hk), 1))
        legs["st_sweep"].append(sweep_ms())
        legs["st1"].append(med(lambda: plan.solve_t(E1), 1))
        legs["stk"].append(med(lambda: plan.solve_t(Ek), 1))
    m_ = {k: float(np.median(v)) for k, v in legs.items()}
    r_sweep = m_["mean"] - m_["denom"]
    r_lc = (m_["lck"] - m_["lc1"]) / a.batches
    out.update(rounds=a.rounds, rounds_eval_mean_ms=m_["mean"], rounds_eval_denom_ms=m_["denom"], rounds_one_mean_sweep_ms=r_sweep,
               rounds_lincomb_ms_per_batch=r_lc, solve_t_sweep_ms_per_batch=m_["st_sweep"],
               solve_t_sweep_min_max_ms=[float(np.min(legs["st_sweep"])), float(np.max(legs["st_sweep"]))],
               solve_t_sweep_ms_per_solve=m_["st_sweep"] / NB, solve_t_sweep_over_single_sweep=m_["st_sweep"] / max(r_sweep, 1e-9),
               solve_t_sweep_over_lincomb_batch=m_["st_sweep"] / max(r_lc, 1e-9),
               solve_t_call_ms_per_batch=(m_["stk"] - m_["st1"]) / 2, solve_t_first_batch_call_ms=m_["st1"])
    if a.summary:
        lib.gpv_plan_debug_draws_ms.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_double)]
        mu = plan.posterior_mean()
        kw = dict(seed=1, mu_ord=mu, link=0, thresholds=[-0.5, 0.0, 0.5])
        plan.draws_summary(3 * NB, **kw)                                  # first use: buffers
        three = np.zeros(3)

        def parts_ms():
            L.check(lib.gpv_plan_debug_draws_ms(plan._h, 1, L.dptr(three)), "gpv_plan_debug_draws_ms")
            return three.copy()
        sl = dict(st_sweep=[], st1=[], stk=[], parts=[], ds1=[], dsk=[])
        for _ in range(a.rounds):
            sl["st_sweep"].append(sweep_ms())
            sl["st1"].append(med(lambda: plan.solve_t(E1), 1))
            sl["stk"].append(med(lambda: plan.solve_t(Ek), 1))
            sl["parts"].append(parts_ms())
            sl["ds1"].append(med(lambda: plan.draws_summary(NB, **kw), 1))
            sl["dsk"].append(med(lambda: plan.draws_summary(3 * NB, **kw), 1))
        parts = np.median(np.array(sl["parts"]), axis=0)
        s_ = {k: float(np.median(v)) for k, v in sl.items() if k != "parts"}
        out.update(summary_rounds=a.rounds, summary_fill_ms_per_batch=float(parts[0]), summary_sweep_ms_per_batch=float(parts[1]),
                   summary_accum_ms_per_batch=float(parts[2]), summary_device_ms_per_batch=float(parts.sum()),
                   summary_call_ms_per_batch=(s_["dsk"] - s_["ds1"]) / 2, summary_first_batch_call_ms=s_["ds1"],
                   summary_rounds_solve_t_sweep_ms_per_batch=s_["st_sweep"],
                   summary_rounds_solve_t_call_ms_per_batch=(s_["stk"] - s_["st1"]) / 2,
                   summary_call_below_solve_t_call=bool((s_["dsk"] - s_["ds1"]) < (s_["stk"] - s_["st1"])))
    if a.host:
        import scipy.sparse.linalg as spla
        from oracle import r_side as R
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        from test_gpu_lincomb import _to_oracle_va
        V = sp.csr_matrix(R.U2V_sparse(R.createU_sparse(_to_oracle_va(va), cp, tau)))
        B = np.asarray(H1[:, (va["ord"] - 1)[::-1]].T.todense())
        out["host_spsolve_triangular_ms_per_batch"] = med(lambda: spla.spsolve_triangular(V, B, lower=True), 3)
    if a.pred:
        r2 = np.random.default_rng(11)
        lo, lp = r2.random((40_000, 2)), r2.random((10_000, 2))
        z2 = r2.standard_normal(40_000)
        t2 = 0.05 + 0.1 * r2.random(40_000)
        va2 = G.vecchia_specify(lo, 15, ordering="maxmin", cond_yz="SGV", locs_pred=lp, ordering_pred="obspred")
        G.vecchia_prediction(z2, va2, [1.0, 0.05, 1.5], t2, return_values="meanvar")
        out["prediction_meanvar_4e4_1e4_ms"] = med(lambda: G.vecchia_prediction(z2, va2, [1.0, 0.05, 1.5], t2, return_values="meanvar"), 3)
        out["prediction_mean_4e4_1e4_ms"] = med(lambda: G.vecchia_prediction(z2, va2, [1.0, 0.05, 1.5], t2), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
