"""Bit record of the set kernels across a change of their LDS layout ("LDS layout of the 2-D set kernels").

    python tools/lds_layout_record.py OUT.json           # GPV_LIB=... selects a tagged build

Where the staged coordinates lie in LDS and how wide the covariance rounds read them must not move a bit of any result.  This
runs the smallest cases that reach every path the layout touches (cases() below) through whatever library is loaded and writes
one JSON: per case the SHA-256 of the eight sums (and, for mode U, of the U rows behind them) and the set kernel that ran,
beside the device's CU count (the sums run over the workgroups in workgroup order) and the compiler's version lines.
tests/test_gpu_lds_layout_bits.py replays the cases and compares them with tests/golden/lds_layout_bits.json, recorded with
the library of the commit BEFORE the layout changed.

Cases: n = 4099 uniform points (seed 0), ordering 'none', so that the first m sets are padded, the rest are straight tasks and
the last task is ragged (4099 = 4 * 1024 + 3), 1025 tasks over the four wavefronts of each workgroup, which sit at four
different offsets of the workgroup's LDS; two dimensions at m = 30, 25, 20, whole and in two row shards cut inside a task; one
and three dimensions at m = 30, whose layout must be untouched; Matern 0.5 / 1.5 / 2.5; mode L through the lean kernel, mode L
through the general likelihood-only kernel (a child process with GPV_NO_LEAN=1) and mode U through the Gauss-Jordan kernel.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4099
CUT = 2050                                                   # 4 * 512 + 2: the shards meet inside a task of the whole plan
NUS = (0.5, 1.5, 2.5)
PLANS = [(2, 30, "whole"), (2, 25, "whole"), (2, 20, "whole"),
         (2, 30, "shard0"), (2, 30, "shard1"), (2, 25, "shard0"), (2, 25, "shard1"), (2, 20, "shard0"), (2, 20, "shard1"),
         (1, 30, "whole"), (3, 30, "whole")]
LIK, LEAN = 1, 2                                             # bits of Plan.last_set_kernel()
NO_LEAN = "L-general"                                        # the mode that runs with GPV_NO_LEAN=1


def cases():
    """[(group, name, (d, m, rows), nu, mode)]; mode: 'L' (lean kernel) | 'L-general' (GPV_NO_LEAN=1) | 'U'"""
    out = []
    for d, m, rows in PLANS:
        for nu in NUS:
            for mode in ("L", NO_LEAN, "U"):
                out.append((f"d{d}-m{m}", f"d{d}/m{m}/{rows}/nu{nu}/{mode}", (d, m, rows), nu, mode))
    assert len({c[1] for c in out}) == len(out)
    return out


def _covparms(d, nu):
    # ranges of a few neighbour spacings: well inside what the lean kernel accepts (scaled distances below 500)
    return [1.3, {1: 0.02, 2: 0.1, 3: 0.3}[d], nu]


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def run(todo):
    """{name: record} of the cases in todo, through the loaded library and this process's environment"""
    import gpvecchia_amd as G
    specs, plans, out = {}, {}, {}
    for group, name, key, nu, mode in todo:
        d, m, rows = key
        if (d, m) not in specs:
            rng = np.random.default_rng(0)
            locs = rng.random((N, d))
            z = rng.standard_normal(N)
            va = G.vecchia_specify(locs, m, ordering="none", cond_yz="z", nn_backend="host")
            prep = va["U_prep"]
            specs[(d, m)] = (np.array(va["locsord"], dtype=np.float64), np.nan_to_num(prep["revNNarray"], nan=0.0).astype(np.int32),
                             np.nan_to_num(prep["revCond"], nan=-1.0).astype(np.int8), z[va["ord_z"] - 1])
        if key not in plans:
            locsord, nn, cond, zord = specs[(d, m)]
            kw = {"whole": {}, "shard0": dict(row_begin=0, row_end=CUT), "shard1": dict(row_begin=CUT, row_end=N)}[rows]
            plans[key] = G.Plan(locsord, nn, cond, **kw)
            plans[key].set_data(zord)
        plan = plans[key]
        nug = np.array([0.1])
        if mode == "U":
            plan.eval("matern", _covparms(d, nu), nug, G.GPV_WANT_U | G.GPV_WANT_LOGLIK_Z)
            sums = np.array(plan.sums(), dtype=np.float64)
            rec = dict(sha256=_sha(sums, plan.Lentries()))
        else:
            plan.eval("matern", _covparms(d, nu), nug, G.GPV_WANT_LOGLIK_Z)
            sums = np.array(plan.sums(), dtype=np.float64)
            rec = dict(sha256=_sha(sums))
        rec.update(kernel=int(plan.last_set_kernel()), failed=float(sums[6]), sets=float(sums[7]),
                   finite=bool(np.all(np.isfinite(sums))))
        out[name] = rec
    return out


def check_not_degenerate(todo, recs):
    """what is recorded has to say something: every set done, none failed, finite sums, and the kernel the mode is about"""
    for group, name, key, nu, mode in todo:
        rec = recs[name]
        nsets = {"whole": N, "shard0": CUT, "shard1": N - CUT}[key[2]]
        assert rec["finite"] and rec["failed"] == 0 and rec["sets"] == nsets, (name, rec)
        assert rec["kernel"] == {"L": LIK | LEAN, NO_LEAN: LIK, "U": 0}[mode], (name, rec)


def run_no_lean():
    """the NO_LEAN cases from a child process with GPV_NO_LEAN=1 (the library reads it when it is loaded)"""
    env = dict(os.environ, GPV_NO_LEAN="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"child process failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def environment():
    """what the bits depend on beside the code: the CU count (grid size, hence the order of the sums) and the compiler"""
    import torch
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        ver = subprocess.run([hipcc, "--version"], capture_output=True, text=True, timeout=60).stdout
        ver = "\n".join(ver.strip().splitlines()[:2])              # HIP and clang versions (the rest names install paths)
    except OSError:
        ver = None
    return dict(cu_count=int(torch.cuda.get_device_properties(0).multi_processor_count), hipcc_version=ver)


def main():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (first: see tests/conftest.py)
    if len(sys.argv) == 2 and sys.argv[1] == "--child":
        assert os.environ.get("GPV_NO_LEAN")
        print(json.dumps(run([c for c in cases() if c[4] == NO_LEAN])))
        return
    todo = cases()
    recs = run([c for c in todo if c[4] != NO_LEAN])
    recs.update(run_no_lean())
    check_not_degenerate(todo, recs)
    out = dict(environment(), cases=recs)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(recs)} cases -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
