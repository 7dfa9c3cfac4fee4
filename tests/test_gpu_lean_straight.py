"""The lean likelihood-only set kernel takes a task the plan knows to be unpadded (its byte of task_pad is 0) down a straight
path: records from the prefetch registers straight to their use, staging addresses from per-wavefront tables, stores of row
slots without a cell into a dump cell instead of under a lane mask, indices of the next task by SGPR base + lane offset, the
failure verdict from one OR per two pivots.  A padded task keeps the masked path.  Both must give the general
likelihood-only kernel's eight sums BIT FOR BIT.

As in tests/test_gpu_lik_lean.py the comparison side is one fresh child process with GPV_NO_LEAN=1, which evaluates every case
of this file once.  The small shapes are the smallest that reach every branch of ONE task: n = 300, m = 30 with ordering
'none' has its first 30 sets padded (8 tasks) and the rest not (67 tasks), and a task inside `rows` gets its indices by SGPR
base, one at or past the end the general way; n = 301 and 303 end in a task with sets beyond `rows`; a hole in one interior
row makes a padded task between unpadded ones; two shards cut the tasks at a row that is no multiple of 4.  Launches that
short give a wavefront one task, so what the kernel carries from task to task -- the indices requested during the task
before, the data-row cell cleared once per wavefront, the address tables across a padded task, the request past the last
task after real work -- is tried by the case "long" (n = 20 002), laid out so that wavefronts run three tasks in a known
order: see _long_problem."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIK, LEAN = 1, 2           # bits of Plan.last_set_kernel()
Z = 2                      # GPV_WANT_LOGLIK_Z
SHAPES = {"300": (300, 30, 2), "301": (301, 30, 2), "303": (303, 30, 2), "m20": (200, 20, 1), "m25": (200, 25, 3),
          "long": (20002, 30, 2)}
HOLE_ROW, HOLE_COL = 150, 14          # the interior set that loses one neighbour, and where in its row
BAD_ROW = 200                          # the set that is made singular


# "long": tasks (of 4 sets, in the plan's stored order) that get a hole, see _long_problem
LONG_HOLE_TASKS = (300, 560, 2141)


def _spec(shape, nu=1.5, nug="s", rows=None, cond_mixed=False, hole=False, dup=None, rg=None):
    return dict(shape=shape, nu=nu, nug=nug, rows=rows, cond_mixed=cond_mixed, hole=hole, dup=dup, rg=rg)


CASES = {
    "n300": _spec("300"),
    "n301": _spec("301"),
    "n303": _spec("303"),
    "shard0": _spec("300", rows=(0, 149)),                   # 149 = 4 * 37 + 1: the first shard ends inside a task of the whole plan
    "shard1": _spec("300", rows=(149, 300)),                 # and the second starts there
    "m20-d1-nu0.5": _spec("m20", nu=0.5),
    "m25-d3-nu2.5": _spec("m25", nu=2.5),
    "cond-mixed": _spec("300", cond_mixed=True),
    "nugget-vector": _spec("300", nug="v"),
    "hole": _spec("300", hole=True),
    # columns (c1, c2) of set BAD_ROW whose points are made one point with nugget 0: the matrix is singular from pivot c2 on
    "singular-even": _spec("300", nug="v", dup=(3, 12)),
    "singular-odd": _spec("300", nug="v", dup=(3, 13)),
    "singular-last": _spec("300", nug="v", dup=(7, 29)),
    # range 0.006: 30 neighbours span a quarter of it, and sqrt(3) / 0.006 * sqrt(2) = 408 <= 500 keeps the lean kernel
    "long": _spec("long", nug="v", hole=True, rg=0.006),
}


def _need_gpu():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


def _long_problem():
    """n = 20 002 points along the diagonal of the unit square, both coordinates strictly increasing with the index (jitter
    below the spacing).  The plan stores the sets in Morton order of their own point (21 bits per coordinate; spacing 5e-5 is
    100 quantisation steps), which for such points IS the index order, so stored set s is row s and task t holds rows 4 t ..
    4 t + 3.  5001 tasks are fewer than 3 per wavefront slot: equal shares, one workgroup per slot, and on a device of 256
    CUs 512 workgroups of 4 wavefronts; XCD x takes tasks [5001 x / 8, 5001 (x + 1) / 8) and wavefront v of its 256 the tasks
    lo + v, lo + v + 256, lo + v + 512.  Then, in ONE wavefront each:
      * tasks 0 .. 7 hold the first 30 rows: wavefronts 0 .. 7 of XCD 0 go padded -> straight -> straight;
      * task 300 (hole): wavefront 44 of XCD 0 runs 44, 300, 556: straight -> padded -> straight;
      * task 560 (hole): wavefront 48 runs 48, 304, 560: its LAST task is padded, then the request past the end;
      * task 2141 = 1875 + 256 + 10 (hole): the same in the middle of XCD 3's range;
      * task 5000 holds rows 20 000, 20 001 and two sets beyond `rows`: third task of wavefront 113 of XCD 7 (lo = 4375),
        asked for by the general loads during a straight task.
    (On a device with another CU count the placement differs and the comparison still holds; nothing here reads the
    placement back.)  Neighbours by the library's own search, ordering 'none'."""
    import gpvecchia_amd as G
    n, m, d = SHAPES["long"]
    rng = np.random.default_rng(20002)
    locs = (np.arange(n)[:, None] + 0.4 * rng.random((n, d))) / n
    z = rng.standard_normal(n)
    tau = 0.05 + rng.random(n)
    va = G.vecchia_specify(locs, m, ordering="none", cond_yz="z")
    return z, tau, va


@functools.lru_cache(maxsize=None)
def _problem(shape):
    if shape == "long":
        return _long_problem()
    from oracle import r_side as R
    n, m, d = SHAPES[shape]
    rng = np.random.default_rng(9100 + 10 * m + d + n)
    locs = rng.random((n, d))
    z = rng.standard_normal(n)
    tau = 0.05 + rng.random(n)
    va = R.vecchia_specify(locs, m, ordering="none", cond_yz="z")
    return z, tau, va


def _inputs(spec):
    """(z, locsord, nn, cond, covparms, nuggets in the plan's order) of a case"""
    z, tau, va = _problem(spec["shape"])
    n, m, d = SHAPES[spec["shape"]]
    prep = va["U_prep"]
    locs = np.array(va["locsord"], dtype=np.float64, copy=True)
    nn = np.nan_to_num(prep["revNNarray"], nan=0.0).astype(np.int32)
    cond = np.nan_to_num(prep["revCond"], nan=-1.0).astype(np.int8)
    cp = [1.3, spec["rg"] if spec["rg"] is not None else (0.2 * np.sqrt(d) if d > 1 else 0.02), spec["nu"]]
    nug = np.array([0.1]) if spec["nug"] == "s" else tau[va["ord"] - 1].copy()
    if spec["cond_mixed"]:
        # every third neighbour (never the point itself, the last column) conditioned on as latent instead of observed
        rng = np.random.default_rng(5)
        flip = (rng.random(cond.shape) < 1.0 / 3.0) & (cond >= 0)
        flip[:, -1] = False
        cond = np.where(flip, 1 - cond, cond).astype(np.int8)
    if spec["hole"]:
        # the plan compacts a row's neighbours and pairs them with the LAST entries of its cond row (as the reference does)
        rows = [HOLE_ROW] if spec["shape"] != "long" else [4 * t + 1 for t in LONG_HOLE_TASKS]
        for r in rows:
            assert nn[r, HOLE_COL] > 0
            nn[r, HOLE_COL] = 0
            cond[r] = np.concatenate(([-1], np.delete(cond[r], HOLE_COL)))
    if spec["dup"] is not None:
        c1, c2 = spec["dup"]
        a, b = nn[BAD_ROW, c1] - 1, nn[BAD_ROW, c2] - 1      # (1-based indices into the ordered locations)
        assert a >= 0 and b >= 0 and a != b
        locs[b] = locs[a]
        nug[a] = nug[b] = 0.0
    return z[va["ord_z"] - 1], locs, nn, cond, cp, nug


def _evaluate(name):
    """(8 sums, last_set_kernel) of the case with the library and environment of THIS process"""
    G = _need_gpu()
    spec = CASES[name]
    zord, locs, nn, cond, cp, nug = _inputs(spec)
    kw = {} if spec["rows"] is None else dict(row_begin=spec["rows"][0], row_end=spec["rows"][1])
    plan = G.Plan(locs, nn, cond, **kw)
    plan.set_data(zord)
    plan.eval("matern", cp, nug, Z)
    return np.array(plan.sums(), dtype=np.float64), plan.last_set_kernel()


@functools.lru_cache(maxsize=None)
def _general_kernel():
    """every case through the general likelihood-only kernel: one child process with GPV_NO_LEAN=1"""
    env = dict(os.environ, GPV_NO_LEAN="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    lines = [l for l in r.stdout.splitlines() if l.startswith("STRAIGHTREF ")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    ref = json.loads(lines[-1][len("STRAIGHTREF "):])
    return {k: (np.array([int(h, 16) for h in bits], dtype=np.uint64), kind) for k, (bits, kind) in ref.items()}


def _bits(s):
    return np.ascontiguousarray(s, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _bitwise(name):
    s, kind = _evaluate(name)
    rbits, rkind = _general_kernel()[name]
    print(f"{name}: kernel {kind} (general side {rkind}) sums {s.tolist()}")
    assert rkind == LIK, (name, rkind)                        # the child never takes the lean kernel
    assert kind == (LIK | LEAN), (name, kind)                 # and this process always does
    assert np.array_equal(_bits(s), rbits), (name, s, rbits.view(np.float64))
    return s


@pytest.mark.parametrize("name", ["n300", "n301", "n303", "m20-d1-nu0.5", "m25-d3-nu2.5", "cond-mixed", "nugget-vector", "hole"])
def test_straight_and_padded_tasks_equal_the_general_kernel_bitwise(name):
    s = _bitwise(name)
    assert s[6] == 0 and s[7] == SHAPES[CASES[name]["shape"]][0]


def test_shards_cut_inside_a_task():
    """Each shard's lean sums equal the general kernel's on the same shard bit for bit; sets failed and sets done add up to the
    whole plan's exactly, the floating-point sums -- other partial sums in another order -- within the rounding of that order
    (1e-12, as tests/test_gpu_lik_lean.py and tests/test_gpu_parity.py ask of shards)."""
    whole, a, b = _bitwise("n300"), _bitwise("shard0"), _bitwise("shard1")
    tot = a + b
    assert tot[6] == whole[6] == 0 and tot[7] == whole[7] == 300 and a[7] == 149
    np.testing.assert_allclose(tot, whole, rtol=1e-12)


def test_wavefronts_that_run_three_tasks_padded_and_straight_in_turn():
    """The case "long" (_long_problem): padded -> straight -> straight, straight -> padded -> straight, a padded last task, a
    ragged last task asked for during a straight one, each inside one wavefront; per-point nuggets.  Bit for bit."""
    s = _bitwise("long")
    assert s[7] == SHAPES["long"][0]


@pytest.mark.parametrize("name", ["singular-even", "singular-odd", "singular-last"])
def test_singular_sets_fail_alike(name):
    """Two columns of one set are the same point with nugget 0: exactly singular from the later column's pivot on (an even
    column, an odd one, and the last pivot, j = 29: the verdict ORs the pivots' reciprocals in pairs).  Whatever the rounding
    makes of that pivot and the ones behind it, failure count and sums are the general kernel's bit for bit.  The column is
    where the matrix BECOMES singular; at which pivot the rounding first turns non-positive cannot be read from outside the
    kernel, so the parity of the failing pivot is intended by these cases and not verified."""
    s = _bitwise(name)
    assert s[6] >= 1 and s[7] == 300                          # (the case does reach the failure path)


if __name__ == "__main__" and "--child" in sys.argv:
    sys.path.insert(0, ROOT)
    res = {}
    for name in CASES:
        s, kind = _evaluate(name)
        res[name] = ([format(int(u), "016x") for u in _bits(s)], kind)
    print("STRAIGHTREF " + json.dumps(res), flush=True)
