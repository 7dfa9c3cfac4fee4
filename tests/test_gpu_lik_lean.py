"""The lean likelihood-only set kernel (gpv_sets_kernel<P, D, COV | 16, true>, m + 1 = 21, 26, 31, closed-form Matern in 1
to 3 dimensions) leaves out work that facts of the plan and of the launch make a no-op: the clamp on the scaled distance,
the NaN / Inf tests on coordinates and diagonal, the discovery of padded tasks (read from the plan's byte per task
instead), 64-bit index products, the pivot owner's EXEC-masked bookkeeping and 1 / sqrt(v).  It must therefore give the
general likelihood-only kernel's sums BIT FOR BIT wherever it is selected, and must not be selected where a fact fails.

The comparison side is one fresh child process with GPV_NO_LEAN=1 (the launcher then always takes the general kernel), which
evaluates every case of this file once; Plan.last_set_kernel() tells "lean ran and agreed" from "lean was not selected".
Shapes: n = 603, m = 30 in 2-D (the first 30 sets have missing neighbours: padded and complete tasks mix in Morton order,
and 603 = 4 * 150 + 3 leaves a ragged last task), n = 403 with m = 20 in 1-D and m = 25 in 3-D."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL_RTOL = 1e-12            # log-likelihood against the oracle's closed form
LIK, LEAN = 1, 2           # bits of Plan.last_set_kernel()
Z, NUM = 2, 4              # GPV_WANT_LOGLIK_Z, GPV_WANT_NUMERATOR
SHAPES = {"2d": (603, 30, 2), "1d": (403, 20, 1), "3d": (403, 25, 3)}
NUS = (0.5, 1.5, 2.5)


def _spec(shape, nu=1.5, nug="s", rows=None, nan_coord=False, inf_nug=False, neg_nug=False, zero_diag=False, rg=None, flags=Z,
          twice=False):
    return dict(shape=shape, nu=nu, nug=nug, rows=rows, nan_coord=nan_coord, inf_nug=inf_nug, neg_nug=neg_nug,
                zero_diag=zero_diag, rg=rg, flags=flags, twice=twice)


CASES = {f"{sh}-nu{nu}-{nug}": _spec(sh, nu, nug) for sh in SHAPES for nu in NUS for nug in ("s", "v")}
CASES.update({
    "whole": _spec("2d", nug="v"),
    "shard0": _spec("2d", nug="v", rows=(0, 301)),           # 301 = 4 * 75 + 1: both shards end in a ragged task, and the
    "shard1": _spec("2d", nug="v", rows=(301, 603)),         # second one starts in the middle of a task of the whole plan
    "nan-coord": _spec("2d", nan_coord=True),
    "inf-nugget": _spec("2d", nug="v", inf_nug=True),
    "short-range": _spec("2d", rg=1e-4),                     # cA * diameter = sqrt(3) / 1e-4 * sqrt(2) = 2.4e4 > 500
    "numerator-too": _spec("2d", flags=Z | NUM),
    "neg-nugget": _spec("2d", nug="v", neg_nug=True),
    "zero-diag": _spec("2d", nug="v", zero_diag=True),
    "twice": _spec("2d", nug="v", twice=True),
})


def _need_gpu():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


@functools.lru_cache(maxsize=None)
def _problem(shape):
    from oracle import r_side as R
    n, m, d = SHAPES[shape]
    rng = np.random.default_rng(7000 + 10 * m + d)
    locs = rng.random((n, d))
    z = rng.standard_normal(n)
    tau = 0.05 + rng.random(n)
    va = R.vecchia_specify(locs, m, ordering="none", cond_yz="z")
    return z, tau, va


def _inputs(spec):
    """(z, va, covparms, nuggets in the caller's order) of a case"""
    z, tau, va = _problem(spec["shape"])
    n, m, d = SHAPES[spec["shape"]]
    rg = spec["rg"] if spec["rg"] is not None else (0.2 * np.sqrt(d) if d > 1 else 0.02)
    cp = [1.3, rg, spec["nu"]]
    nug = np.array([0.1]) if spec["nug"] == "s" else tau.copy()
    if spec["inf_nug"]:
        nug[n // 3] = np.inf
    if spec["neg_nug"]:
        nug[n // 2] = -1.5                                   # sigma^2 + nugget < 0 in every set that holds the point as an observation
    if spec["zero_diag"]:
        nug[n // 2] = -1.3                                   # sigma^2 + nugget = +0 exactly: a ZERO first pivot where the point leads a set
    if spec["nan_coord"]:
        va = dict(va)
        va["locsord"] = va["locsord"].copy()
        va["locsord"][n // 2, 0] = np.nan
    return z, va, cp, nug


def _evaluate(name):
    """[(8 sums, last_set_kernel), ...] of the case's evaluations with the library and environment of THIS process"""
    G = _need_gpu()
    spec = CASES[name]
    z, va, cp, nug = _inputs(spec)
    prep = va["U_prep"]
    kw = {} if spec["rows"] is None else dict(row_begin=spec["rows"][0], row_end=spec["rows"][1])
    plan = G.Plan(va["locsord"], np.nan_to_num(prep["revNNarray"], nan=0.0).astype(np.int32),
                  np.nan_to_num(prep["revCond"], nan=-1.0).astype(np.int8), **kw)
    plan.set_data(z[va["ord_z"] - 1])
    out = []
    for _ in range(2 if spec["twice"] else 1):
        plan.eval("matern", cp, nug if nug.size == 1 else nug[va["ord"] - 1], spec["flags"])
        out.append((np.array(plan.sums(), dtype=np.float64), plan.last_set_kernel()))
    return out


@functools.lru_cache(maxsize=None)
def _general_kernel():
    """every case through the general likelihood-only kernel: one child process with GPV_NO_LEAN=1"""
    env = dict(os.environ, GPV_NO_LEAN="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    lines = [l for l in r.stdout.splitlines() if l.startswith("LEANREF ")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    ref = json.loads(lines[-1][len("LEANREF "):])
    return {k: [(np.array([int(h, 16) for h in bits], dtype=np.uint64), kind) for bits, kind in v] for k, v in ref.items()}


@functools.lru_cache(maxsize=None)
def _both(name):
    return _evaluate(name), _general_kernel()[name]


def _bits(s):
    return np.ascontiguousarray(s, dtype=np.float64).view(np.uint64)


def _assert_bitwise(name, want_lean):
    here, ref = _both(name)
    for (s, kind), (rbits, rkind) in zip(here, ref):
        assert rkind == LIK, (name, rkind)                    # the child never takes the lean kernel
        assert kind == ((LIK | LEAN) if want_lean else LIK), (name, kind)
        assert np.array_equal(_bits(s), rbits), (name, s, rbits.view(np.float64))
    return here


@pytest.mark.parametrize("nug", ["s", "v"])
@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_lean_kernel_equals_general_kernel_bitwise_and_follows_the_oracle(shape, nu, nug):
    from oracle import r_side as R
    G = _need_gpu()
    name = f"{shape}-nu{nu}-{nug}"
    (s, _), = _assert_bitwise(name, want_lean=True)
    n = SHAPES[shape][0]
    assert s[6] == 0 and s[7] == n
    z, va, cp, nug_v = _inputs(CASES[name])
    ref = R.createU(va, cp, nug_v if nug_v.size > 1 else float(nug_v[0]))
    ll_ref, _ = R.separable_loglik_condz(va, ref["U_entries"], z, nug_v)
    ll = G.loglik_z_from_sums(s, n)
    print(f"{name}: loglik {ll!r} oracle {ll_ref!r} rel {abs(ll - ll_ref) / abs(ll_ref):.2e}")
    assert abs(ll - ll_ref) <= LL_RTOL * abs(ll_ref)


def test_shards_use_their_own_task_bytes():
    """Two shards of the n = 603 plan (row_begin / row_end): each has its own tasks, so its own bytes of padding.  Each shard's
    lean sums equal the general kernel's on the same shard bit for bit; the sets that failed and the sets done add up to the
    whole plan's exactly, and the floating-point sums of the two shards -- other partial sums in another order than the
    whole plan's -- to the whole plan's within the rounding of that order (1e-12, as tests/test_gpu_parity.py asks of shards)."""
    (whole, _), = _assert_bitwise("whole", want_lean=True)
    (a, _), = _assert_bitwise("shard0", want_lean=True)
    (b, _), = _assert_bitwise("shard1", want_lean=True)
    tot = a + b
    print("shards", _bits(tot), "whole", _bits(whole), "bitwise equal:", bool(np.array_equal(_bits(tot), _bits(whole))))
    assert tot[6] == whole[6] == 0 and tot[7] == whole[7] == 603 and a[7] == 301
    np.testing.assert_allclose(tot, whole, rtol=1e-12)


@pytest.mark.parametrize("name", ["nan-coord", "inf-nugget", "short-range", "numerator-too"])
def test_general_kernel_where_a_fact_fails(name):
    (s, kind), = _assert_bitwise(name, want_lean=False)
    assert s[7] == 603
    if name == "nan-coord":
        assert s[6] >= 1                                      # every set that holds the point fails
    elif name != "inf-nugget":                                # (the set of the point with the infinite nugget fails, on any kernel)
        assert s[6] == 0


def test_failure_verdicts_from_the_pivot_signs():
    """A nugget of -1.5 under sigma^2 = 1.3: a negative diagonal, so a negative pivot, in every set that holds the point as
    an observation.  The lean kernel is selected (the value is finite) and must fail exactly the same sets."""
    (s, _), = _assert_bitwise("neg-nugget", want_lean=True)
    assert s[6] > 0 and s[7] == 603


def test_failure_verdicts_from_a_zero_pivot():
    """A nugget of -sigma^2 exactly: the point's diagonal is +0, so the pivot is +0 in the sets the point leads (its reciprocal
    is no finite number: the sign test alone would pass it, the verdict has to come through v of the last row) and negative
    in the others that hold it.  The lean kernel is selected and must give the general kernel's verdicts and sums."""
    (s, _), = _assert_bitwise("zero-diag", want_lean=True)
    print("zero-diag: failed sets", s[6], "sums", s)
    assert s[6] > 0 and s[7] == 603


def test_two_lean_launches_on_one_plan_agree_bitwise():
    (a, ka), (b, kb) = _assert_bitwise("twice", want_lean=True)
    assert np.array_equal(_bits(a), _bits(b))


if __name__ == "__main__" and "--child" in sys.argv:
    sys.path.insert(0, ROOT)
    res = {name: [([format(int(u), "016x") for u in _bits(s)], kind) for s, kind in _evaluate(name)] for name in CASES}
    print("LEANREF " + json.dumps(res), flush=True)
