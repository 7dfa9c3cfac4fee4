"""The set kernels give the bits they gave before the LDS layout of the 2-D kernels changed ("LDS layout of the
2-D set kernels"): where the staged coordinates lie, how wide the covariance rounds read them and which row a row slot
without a row shadows move no bit of any result.

tests/golden/lds_layout_bits.json was recorded by tools/lds_layout_record.py with the library of the commit BEFORE that change
(built from a clean checkout as a tagged library, GPV_LIB pointing at it).  The cases (cases() of the tool) are replayed here
through the library under test and compared with the record: the SHA-256 of the eight sums (mode L through the lean kernel,
and through the general likelihood-only kernel in a child process that sets GPV_NO_LEAN) and of the sums and U rows (mode U).
n = 4099 uniform points (seed 0), ordering 'none': padded first rows, straight tasks, a ragged last task, the four wavefronts
of a workgroup at four struct offsets; 2-D at m = 30, 25, 20, whole and in two row shards cut inside a task; 1-D and 3-D at
m = 30, which the change must not touch; Matern 0.5 / 1.5 / 2.5.

The sums run over the workgroups in workgroup order, so the bits depend on the CU count through the grid size, and they depend
on the compiler; the record holds both, and the replay is skipped only where one of them differs from the record.  A bit that
differs otherwise means the arithmetic or the summation order moved: find it and put it back, do not record again.

  test_record_is_complete_and_not_degenerate   (no GPU) the record holds exactly the cases, every set done, none failed
  test_bits[group]                             modes L (lean) and U of one (dimension, m)
  test_bits_general_likelihood_kernel          mode L with GPV_NO_LEAN=1, every case, one child process"""
import functools
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("lds_layout_record", os.path.join(ROOT, "tools", "lds_layout_record.py"))
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)
with open(os.path.join(ROOT, "tests", "golden", "lds_layout_bits.json")) as _f:
    GOLDEN = json.load(_f)
CASES = REC.cases()


def test_record_is_complete_and_not_degenerate():
    assert set(GOLDEN["cases"]) == {c[1] for c in CASES}
    assert len(CASES) == 11 * 3 * 3
    assert GOLDEN["cu_count"] == 256 and GOLDEN["hipcc_version"]
    REC.check_not_degenerate(CASES, GOLDEN["cases"])


@functools.lru_cache(maxsize=None)
def _environment_differs():
    env = REC.environment()
    for key in ("cu_count", "hipcc_version"):
        if env[key] != GOLDEN[key]:
            return (f"{key} is {env[key]!r}, the record was made with {GOLDEN[key]!r}: build the commit before the layout change "
                    "as a tagged library and record again with GPV_LIB=<that library> python tools/lds_layout_record.py "
                    "tests/golden/lds_layout_bits.json")
    return None


def _compare(todo, got):
    assert set(got) == {c[1] for c in todo}
    REC.check_not_degenerate(todo, got)
    differ = [c[1] for c in todo if got[c[1]] != GOLDEN["cases"][c[1]]]
    print(f"{len(todo)} cases, {len(differ)} differ from the record")
    assert not differ, differ[:10]


def _need_gpu():
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    why = _environment_differs()
    if why:
        pytest.skip(why)


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted({c[0] for c in CASES}))
def test_bits(group):
    _need_gpu()
    todo = [c for c in CASES if c[0] == group and c[4] != REC.NO_LEAN]
    _compare(todo, REC.run(todo))


@pytest.mark.gpu
def test_bits_general_likelihood_kernel():
    _need_gpu()
    _compare([c for c in CASES if c[4] == REC.NO_LEAN], REC.run_no_lean())
