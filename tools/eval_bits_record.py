"""Bits of a few 'matern' and 'esqe' evaluations and gradient calls, for comparing two builds of the library:

    python tools/eval_bits_record.py OUT.json            # GPV_LIB=... selects the other build
    python tools/eval_bits_record.py --compare A.json B.json
    python tools/eval_bits_record.py --parent-library    # builds (once) and prints the library of the commit before 'matern_scaledim'

The families that existed before 'matern_scaledim' must compute what the commit before it computed, bit for bit:
tests/test_gpu_unchanged_bits.py runs record() in two fresh child processes, one with GPV_LIB naming the parent's library, and
asserts that the records are equal.  Cases: n = 3000, m = 10 and 30 (the general, the likelihood-only and the lean set kernels),
d = 2 and 5, Matern 0.5, 1.5, 2.5 and 0.8 and esqe, cond.yz = 'z' with the U entries and the likelihood-only sums, one
gpv_plan_loglik_grad each, cond.yz = 'SGV' with the posterior pass (twice: the captured graph's replay).  Each record is the
SHA-256 of the bytes of what the calls returned.  Every row length is one the short parent build compiles (PARENT_PLIST).

parent_library(): GPV_PARENT_LIB if set; else the newest commit whose gpv_api.hip does not know the family is exported from git
into gpvecchia_amd/csrc/build_parent_<commit>/ (ignored by git, kept for the next run) and built there by ITS OWN build.py as a
tagged library with the row lengths of PARENT_PLIST only; in a copy of the tree without its history, the one such build an
earlier run left behind; None where there is none of these."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARENT_PLIST = (11, 31)                                   # m = 10 and m = 30
API = "gpvecchia_amd/csrc/gpv_api.hip"


def parent_library():
    env = os.environ.get("GPV_PARENT_LIB")
    if env:
        return env if os.path.exists(env) else None

    def git(*args, **kw):
        return subprocess.run(["git", "-C", ROOT] + list(args), capture_output=True, **kw)
    r = git("log", "--format=%H", "--", API)
    if r.returncode != 0:                                # no history here: the one parent build an earlier run left, if any
        import glob
        left = glob.glob(os.path.join(ROOT, "gpvecchia_amd", "csrc", "build_parent_*", "gpvecchia_amd", "libgpvecchia_hip_parent.so"))
        return left[0] if len(left) == 1 else None
    parent = None
    for rev in r.stdout.decode().split():
        s = git("show", f"{rev}:{API}")
        if s.returncode == 0 and b"matern_scaledim" not in s.stdout:
            parent = rev
            break
    if parent is None:
        return None
    work = os.path.join(ROOT, "gpvecchia_amd", "csrc", "build_parent_" + parent[:12])
    lib = os.path.join(work, "gpvecchia_amd", "libgpvecchia_hip_parent.so")
    if os.path.exists(lib):
        return lib
    os.makedirs(work, exist_ok=True)
    a = git("archive", parent, "gpvecchia_amd", "include")
    if a.returncode != 0:
        return None
    subprocess.run(["tar", "-x", "-C", work], input=a.stdout, check=True)
    jobs = str(min(16, os.cpu_count() or 1))
    b = subprocess.run([sys.executable, "-m", "gpvecchia_amd.build", "--tag", "_parent", "--jobs", jobs,
                        "--plist", ",".join(str(p) for p in PARENT_PLIST)], cwd=work, capture_output=True, text=True)
    if b.returncode != 0 or not os.path.exists(lib):
        raise RuntimeError("the parent's library did not build:\n" + b.stdout[-2000:] + b.stderr[-2000:])
    return lib


def record():
    import torch  # noqa: F401  (first: see tests/conftest.py)
    import gpvecchia_amd as G
    out = {}

    def sha(*arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        return h.hexdigest()
    n, tau = 3000, 0.1
    fams = {"nu0.5": ("matern", [1.3, 0.1, 0.5]), "nu1.5": ("matern", [1.3, 0.1, 1.5]), "nu2.5": ("matern", [1.3, 0.1, 2.5]),
            "nu0.8": ("matern", [1.3, 0.1, 0.8]), "esqe": ("esqe", [0.8, 0.1, 0.5, 0.08])}
    for d in (2, 5):
        locs = np.random.default_rng(d).random((n, d))
        z = np.random.default_rng(10 + d).standard_normal(n)
        for m in (10, 30):
            va = G.vecchia_specify(locs, m, cond_yz="z", nn_backend="host")
            plan = G.api._plan_for(va, 0)
            plan.set_data(z[va["ord_z"] - 1])
            for name, (cm, cp) in fams.items():
                key = f"z d{d} m{m} {name}"
                plan.eval(cm, cp, np.array([tau]), G.GPV_WANT_U | G.GPV_WANT_LOGLIK_Z)
                out[key + " U"] = sha(plan.sums(), plan.Lentries())
                plan.eval(cm, cp, np.array([tau]), G.GPV_WANT_LOGLIK_Z)
                out[key + " lik kernel %d" % plan.last_set_kernel()] = sha(plan.sums())
                if name != "nu0.8":
                    ll, g, nf = plan.loglik_grad(cm, cp, tau)
                    out[key + " grad"] = sha([ll], g, [nf])
        va = G.vecchia_specify(locs, 10, cond_yz="SGV", nn_backend="host")
        for name, (cm, cp) in fams.items():
            a = G.vecchia_likelihood(z, va, cp, tau, covmodel=cm)
            b = G.vecchia_likelihood(z, va, cp, tau, covmodel=cm)
            out[f"SGV d{d} {name}"] = sha([a, b])
    return out


def main(argv):
    if argv[1] == "--parent-library":
        print(parent_library())
        return 0
    if argv[1] == "--compare":
        A, B = (json.load(open(p)) for p in argv[2:4])
        diff = sorted(k for k in set(A) | set(B) if A.get(k) != B.get(k))
        print(f"{len(A)} records, {len(diff)} differ", diff[:10])
        return 1 if diff or not A else 0
    with open(argv[1], "w") as f:
        json.dump(record(), f, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
