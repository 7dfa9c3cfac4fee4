"""The timed-repetition entries of the operators on a resident factor (gpv_plan_debug_{whiten,unwhiten,loo,blockcv,solve_t,selinv}_ms,
developer aids of tools/*_timing.py, not in the public header), on the GPU.  For each entry, on a plan of its own: it refuses
(GPV_ERR_STATE) before its operator has run; after the operator, three repetitions give three finite, positive device times;
and the operator called again afterwards returns the bits it returned before the timing call: the repetitions run on the
columns the operator left on the device and change nothing that a later call reads.

n = 1999 (odd, more than one block of every kernel), 2-D, Matern 1.5, m = 10 and m = 30; 3 columns (padded to 4) and 16 (the
most a call takes).  whiten / unwhiten / loo / block_cv on a cond.yz = 'z' plan; solve_t / selinv on the cond.yz = 'SGV' plan of
a vecchia_prediction, as in test_gpu_selinv.py."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1999
CP = [1.0, 0.15, 1.5]
TAU = 0.1
REPS = 3
GPV_OK, GPV_ERR_STATE = 0, 7
MS = C.POINTER(C.c_double)
ARGTYPES = {                                   # the tools declare them too; gpvecchia_amd/_lib.py declares the public header only
    "gpv_plan_debug_whiten_ms": [C.c_void_p, C.c_int, MS],
    "gpv_plan_debug_unwhiten_ms": [C.c_void_p, C.c_int, MS],
    "gpv_plan_debug_loo_ms": [C.c_void_p, C.c_int, MS],
    "gpv_plan_debug_blockcv_ms": [C.c_void_p, C.c_int, C.c_int, MS],
    "gpv_plan_debug_solve_t_ms": [C.c_void_p, C.c_int, MS],
    "gpv_plan_debug_selinv_ms": [C.c_void_p, C.c_int, MS],
}


def _need_gpu():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    return G


@functools.lru_cache(maxsize=None)
def _case(m, cond_yz):
    """locations, data, columns and the specification, made once per (m, cond.yz); every test makes a plan of its own from it"""
    G = _need_gpu()
    rng = np.random.default_rng(100 + m)
    locs, z, tau = rng.random((N, 2)), rng.standard_normal(N), 0.05 + 0.1 * rng.random(N)
    cols = np.asfortranarray(rng.standard_normal((N, 16)))
    return G.vecchia_specify(locs, m, ordering="maxmin", cond_yz=cond_yz), z, tau, cols


def _z_plan(m):
    """a new 'z' plan whose latest evaluation left its factor"""
    G = _need_gpu()
    va, z, _, cols = _case(m, "z")
    prep = va["U_prep"]
    plan = G.api.Plan(va["locsord"], prep["revNNarray"], prep["revCond"])
    plan.set_data(z[va["ord_z"] - 1])
    plan.eval("matern", CP, np.array([TAU]), G.GPV_WANT_U)
    return plan, cols


def _sgv_plan(m):
    """a new 'SGV' plan with the posterior factor of a prediction"""
    G = _need_gpu()
    va, z, tau, cols = _case(m, "SGV")
    va = {k: v for k, v in va.items() if not isinstance(k, tuple)}          # (without the plan an earlier test made for it)
    preds = G.vecchia_prediction(z, va, CP, tau, return_values="meanmat")
    return preds["factor"]["plan"], cols


def _timed(plan, entry, *parts):
    """(status, ms[REPS]) of one call of the entry; ms keeps its NaN where the entry wrote nothing"""
    from gpvecchia_amd import _lib as L
    f = getattr(L.lib(), entry)
    f.argtypes, f.restype = ARGTYPES[entry], C.c_int
    ms = np.full(REPS, np.nan)
    return f(plan._h, REPS, *parts, L.dptr(ms)), ms


def _bits(out):
    return [None if a is None else np.asarray(a).tobytes() for a in (out if isinstance(out, tuple) else (out,))]


def _check(plan, entry, operator, *parts):
    st, ms = _timed(plan, entry, *parts)
    assert st == GPV_ERR_STATE and np.all(np.isnan(ms)), (entry, "before its operator", st, ms)
    before = operator()
    st, ms = _timed(plan, entry, *parts)
    print(f"{entry}{parts}: status {st}, ms = {ms.tolist()}")
    assert st == GPV_OK, (entry, st)
    assert ms.shape == (REPS,) and np.all(np.isfinite(ms)) and np.all(ms > 0.0), (entry, ms)
    after = operator()
    assert _bits(after) == _bits(before), (entry, "the operator's result changed over the timing call")


@pytest.mark.parametrize("ncols", [3, 16])
@pytest.mark.parametrize("m", [10, 30])
def test_whiten(m, ncols):
    plan, cols = _z_plan(m)
    _check(plan, "gpv_plan_debug_whiten_ms", lambda: plan.whiten(cols[:, :ncols], want_E=True))


@pytest.mark.parametrize("ncols", [3, 16])
@pytest.mark.parametrize("m", [10, 30])
def test_unwhiten(m, ncols):
    plan, cols = _z_plan(m)
    _check(plan, "gpv_plan_debug_unwhiten_ms", lambda: plan.unwhiten(cols[:, :ncols]))


@pytest.mark.parametrize("ncols", [3, 16])
@pytest.mark.parametrize("m", [10, 30])
def test_loo(m, ncols):
    plan, cols = _z_plan(m)
    _check(plan, "gpv_plan_debug_loo_ms", lambda: plan.loo(cols[:, :ncols]))


@pytest.mark.parametrize("ncols", [3, 16])
@pytest.mark.parametrize("m", [10, 30])
def test_blockcv(m, ncols):
    plan, cols = _z_plan(m)
    plan.set_blocks((np.arange(N) // 8).astype(np.int32))                   # 250 blocks of (up to) 8 consecutive ordered rows
    _check(plan, "gpv_plan_debug_blockcv_ms", lambda: plan.block_cv(cols[:, :ncols]), 7)


@pytest.mark.parametrize("ncols", [3, 16])
@pytest.mark.parametrize("m", [10, 30])
def test_solve_t(m, ncols):
    plan, cols = _sgv_plan(m)
    E = np.ascontiguousarray(cols[:, :ncols].T)
    _check(plan, "gpv_plan_debug_solve_t_ms", lambda: plan.solve_t(E))


@pytest.mark.parametrize("m", [10, 30])
def test_selinv(m):
    plan, _ = _sgv_plan(m)
    _check(plan, "gpv_plan_debug_selinv_ms", plan.selinv)
