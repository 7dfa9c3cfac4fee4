"""Bit record of the analytic-derivative family: gpv_plan_loglik_{grad,fisher,rep}{,_nu} (gpv_grad.hip).

    python tools/grad_family_record.py OUT.json          # GPV_LIB=... selects a tagged build

Runs the six entries through whatever library is loaded, over the smallest cases that reach every kernel instantiation and edge
(cases() below), and writes one JSON: per case loglik, grad, the upper triangle of fisher and n_failed as hex floats and the
SHA-256 of the row_terms bytes, beside the device's CU count (the grid cap depends on it) and the version lines of
`hipcc --version`.
tests/test_gpu_grad_family_bits.py replays the cases and compares them with tests/golden/grad_family_bits.json, recorded with the
library of the commit BEFORE the kernels' phases were shared: a refactor of these kernels has to keep every bit.  The general-nu
cases with GPV_NO_MATERN_TABLE=1 (every pair takes the quadrature) run in a child process of their own, which sets the variable.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 0.1
FAMILIES = ("nu0.5", "nu1.5", "nu2.5", "esqe", "nu0.8")
NO_TABLE = "no_table"                                         # the group that runs with GPV_NO_MATERN_TABLE=1


def family(name, d):
    """(covmodel, covparms, smoothness_grad); nu0.8 is a general smoothness and goes through the _nu entries"""
    r = 0.25 * np.sqrt(d / 2)
    if name == "esqe":
        return "esqe", [0.8, r, 0.5, 0.8 * r], False
    nu = float(name[2:])
    return "matern", [1.3, r, nu], nu not in (0.5, 1.5, 2.5)


def cases():
    """[(group, name, plan key (n, m, d, kind), family, entry, R)]; kind: '' | 'dup' (coincident points) | 'nan' (a NaN coordinate)"""
    out = []
    for fam in FAMILIES:                                      # every family, both sides of every row-length bucket, both layouts
        for m in (3, 15, 16, 31, 32, 63):
            for d in (2, 5):
                for entry, R in (("grad", 0), ("fisher", 0), ("rep", 5)):
                    out.append(("buckets-" + fam, f"{fam}/m{m}/d{d}/{entry}", (600, m, d, ""), fam, entry, R))
    for fam in FAMILIES:                                      # replicate counts: one chunk exactly filled or not, two chunks
        for R in (1, 9):
            out.append(("replicates", f"{fam}/m10/d2/rep{R}", (600, 10, 2, ""), fam, "rep", R))
    for entry, R in (("grad", 0), ("fisher", 0), ("rep", 5)):
        out.append((NO_TABLE, f"no-table/nu0.8/m10/d2/{entry}", (600, 10, 2, ""), "nu0.8", entry, R))
        out.append((NO_TABLE, f"no-table/nu0.8/m31/d5/{entry}", (600, 31, 5, ""), "nu0.8", entry, R))
        for kind in ("dup", "nan"):
            for fam in ("nu1.5", "nu0.8"):
                out.append(("edges", f"{kind}/{fam}/m10/d2/{entry}", (600, 10, 2, kind), fam, entry, R))
        out.append(("grid-cap", f"nu1.5/n6000/m10/d2/{entry}", (6000, 10, 2, ""), "nu1.5", entry, R))
    assert len({c[1] for c in out}) == len(out)
    return out


def _inputs(n, m, d, kind):
    """seeded locations, data, replicates and the m nearest earlier points of every point (ties: the earlier index), 1-based"""
    rng = np.random.default_rng(1000 * m + d)
    locs = rng.random((n, d))
    z = rng.standard_normal(n)
    Z = rng.standard_normal((n, 9))
    if kind == "dup":                                         # every third point sits on an earlier one
        for j in range(2, n, 3):
            locs[j] = locs[rng.integers(j)]
    NN = np.zeros((n, m + 1), dtype=np.int32)
    for i in range(n):
        d2 = ((locs[:i] - locs[i]) ** 2).sum(axis=1)
        near = np.argsort(d2, kind="stable")[:m]
        NN[i, 0] = i + 1
        NN[i, 1:1 + near.size] = near + 1
    return locs, z, Z, NN


def _hex(a):
    return [float(x).hex() for x in np.ravel(a)]


def run(todo):
    """{name: record} of the cases in todo, through the loaded library"""
    import gpvecchia_amd as G
    plans, out = {}, {}
    for group, name, key, fam, entry, R in todo:
        if key not in plans:
            n, m, d, kind = key
            locs, z, Z, NN = _inputs(*key)
            va = G.vecchia_specify(locs, m, ordering="none", cond_yz="z", NNarray=NN)
            ordered = np.array(va["locsord"])
            if kind == "nan":
                ordered[n // 2, d - 1] = np.nan
            prep = va["U_prep"]
            plan = G.Plan(ordered, prep["revNNarray"], prep["revCond"])
            plan.set_data(z)
            plans[key] = (plan, Z)
        plan, Z = plans[key]
        cm, cp, sg = family(fam, key[2])
        info = None
        if entry == "grad":
            ll, grad, nfail, rows = plan.loglik_grad(cm, cp, TAU, row_terms=True, smoothness_grad=sg)
        elif entry == "fisher":
            ll, grad, info, nfail, rows = plan.loglik_fisher(cm, cp, TAU, row_terms=True, smoothness_grad=sg)
        else:
            plan.set_replicates(Z[:, :R])
            ll, grad, info, nfail, rows = plan.loglik_replicates(cm, cp, TAU, row_terms=True, smoothness_grad=sg)
        rec = dict(loglik=float(ll).hex(), grad=_hex(grad), n_failed=float(nfail).hex(),
                   row_terms_sha256=hashlib.sha256(np.ascontiguousarray(rows).tobytes()).hexdigest())
        if info is not None:
            assert np.array_equal(info.view(np.int64), info.T.view(np.int64))          # mirrored by the library: bitwise symmetric
            rec["fisher"] = _hex(info[np.triu_indices(info.shape[0])])
        out[name] = rec
    return out


def check_not_degenerate(todo, recs):
    """what is recorded has to say something: no failed set and finite totals everywhere but where the case is about failing
    (a NaN coordinate) and in the slots that are NaN by design (the smoothness of a closed-form matern)"""
    for group, name, key, fam, entry, R in todo:
        rec, (cm, cp, sg) = recs[name], family(fam, key[2])
        if key[3] == "nan":
            assert float.fromhex(rec["n_failed"]) > 0 and float.fromhex(rec["loglik"]) == -np.inf, name
            continue
        keep = np.array([not (cm == "matern" and not sg and t == 2) for t in range(len(cp) + 1)])
        grad = np.array([float.fromhex(x) for x in rec["grad"]])
        assert float.fromhex(rec["n_failed"]) == 0 and np.isfinite(float.fromhex(rec["loglik"])), name
        assert np.all(np.isfinite(grad[keep])) and np.all(np.isnan(grad[~keep])), name
        if "fisher" in rec:
            tri = np.array([float.fromhex(x) for x in rec["fisher"]])
            i, j = np.triu_indices(keep.size)
            assert np.all(np.isfinite(tri[keep[i] & keep[j]])) and np.all(np.isnan(tri[~(keep[i] & keep[j])])), name


def run_no_table():
    """the NO_TABLE group from a child process with GPV_NO_MATERN_TABLE=1"""
    env = dict(os.environ, GPV_NO_MATERN_TABLE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", NO_TABLE], env=env, capture_output=True, text=True,
                       timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"child process failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def environment():
    """what the bits depend on beside the code: the CU count (grid cap, hence the order of the sums) and the compiler"""
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
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        assert sys.argv[2] != NO_TABLE or os.environ.get("GPV_NO_MATERN_TABLE")
        print(json.dumps(run([c for c in cases() if c[0] == sys.argv[2]])))
        return
    todo = cases()
    recs = run([c for c in todo if c[0] != NO_TABLE])
    recs.update(run_no_table())
    check_not_degenerate(todo, recs)
    out = dict(environment(), cases=recs)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{len(recs)} cases -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
