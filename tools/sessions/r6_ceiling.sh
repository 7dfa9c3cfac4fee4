#!/bin/bash
# round 6: what evaluating shared point pairs once could save AT MOST (timing-only builds that skip covariance rounds:
# keep 9 of 15 = 60 %, keep 10 = 67 %; tools/stat_pairs_and_tiles.py finds 63-74 % distinct pairs per task), same box, alternating;
# and the shipped general-nu table against the oracle on the cases the F64 variant was measured on
cd $GRAFT_REPO_ROOT
O=gpurun_out/r06c; mkdir -p $O
for rep in 1 2 3; do
  for lib in base keep10 keep9; do
    if [ $lib = base ]; then unset GPV_LIB; else export GPV_LIB=$GRAFT_REPO_ROOT/gpvecchia_amd/libgpvecchia_hip_$lib.so; fi
    python bench.py --no-secondary --no-cpu-baseline --steps 20 --warmup 5 2>/dev/null | python3 -c "
import sys, json
j = json.loads([l for l in sys.stdin if l.startswith('{')][-1])
print('$lib rep $rep: evals/s %.1f kernel_ms %.4f' % (j['value'], j['roofline']['kernel_ms']))" | tee -a $O/ab.txt
  done
done
unset GPV_LIB
python3 - <<'PY' 2>&1 | tee $O/parity_base.txt
import os, sys, numpy as np
sys.path.insert(0, os.getcwd())
import gpvecchia_amd as G
from oracle import r_side as R
rng = np.random.default_rng(3)
n, m = 4000, 30
locs = rng.random((n, 2))
va = G.vecchia_specify(locs, m, ordering="maxmin", cond_yz="SGV")
prep = va["U_prep"]
tau = 0.05 + 0.1 * rng.random(n)
for nu, rg in ((0.3, 0.05), (1.1, 0.02), (1.1, 0.3), (2.2, 0.1), (7.5, 0.05), (0.9, 2.0)):
    cp = [1.3, rg, nu]
    out = G.U_NZentries(1, n, va["locsord"], prep["revNNarray"], prep["revCond"], tau, tau, "matern", cp)
    ref = R.U_NZentries(1, n, va["locsord"], prep["revNNarray"], np.where(prep["revCond"] < 0, 0, prep["revCond"]), tau, tau, "matern", cp)
    err = np.abs(out["Lentries"] - ref["Lentries"]).max(axis=1) / np.abs(ref["Lentries"]).max(axis=1)
    print(f"shipped table nu={nu} range={rg}: max row err {err.max():.2e}, rows beyond 1e-8: {(err > 1e-8).sum()}, beyond 1e-10: {(err > 1e-10).sum()}, median {np.median(err):.1e}, failed rows hip {out['n_failed']} oracle {ref['n_failed']}")
PY
python bench.py --full --no-secondary --steps 20 --warmup 5 2>/dev/null | python3 -c "
import sys, json
j = json.loads([l for l in sys.stdin if l.startswith('{')][-1])
print('headline', j['value'], j['roofline']['frac'], 'speedup', j['speedup_vs_cpu_port']); print(json.dumps(j['cpu_baseline'])[:3000])" | tee $O/cpu_baseline.txt
