"""gpv_plan_loglik_{grad,fisher,rep}{,_nu} give the bits they gave before their kernels' phases were shared.

tests/golden/grad_family_bits.json was recorded by tools/grad_family_record.py with the library of the commit BEFORE that refactor
(built from a worktree as a tagged library, GPV_LIB pointing at it).  The cases (cases() of the tool) are replayed here through the
library under test and compared with the record byte for byte: loglik, grad, the information, n_failed and the SHA-256 of the
row_terms bytes.  They are the smallest that reach every instantiation and edge: n = 600, every family (matern 0.5 / 1.5 / 2.5,
esqe, matern 0.8 through the _nu entries), rows on both sides of every bucket (m = 3, 15, 16, 31, 32, 63), packed and unpacked
coordinates (d = 2, 5), R = 1, 5, 9 replicates, the general smoothness with and without its tables (the latter in a child
process that sets GPV_NO_MATERN_TABLE), coincident points, a NaN coordinate, and n = 6000 at the grid cap of 1024 workgroups.

The sums run over the workgroups in workgroup order, so the bits depend on the CU count through the grid cap, and they depend on
the compiler; the record holds both, and a group is skipped only where one of them differs from the record.  A bit that differs
otherwise means the arithmetic moved: find it and put it back, do not record again.

  test_record_is_complete_and_not_degenerate   (no GPU) the record holds exactly the cases, finite totals, no failed set
  test_bits[group]                             the replay"""
import functools
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("grad_family_record", os.path.join(ROOT, "tools", "grad_family_record.py"))
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)
with open(os.path.join(ROOT, "tests", "golden", "grad_family_bits.json")) as _f:
    GOLDEN = json.load(_f)
CASES = REC.cases()
FIELDS = ("loglik", "grad", "fisher", "n_failed", "row_terms_sha256")


def test_record_is_complete_and_not_degenerate():
    assert set(GOLDEN["cases"]) == {c[1] for c in CASES}
    assert GOLDEN["cu_count"] == 256 and GOLDEN["hipcc_version"]
    for c in CASES:
        assert ("fisher" in GOLDEN["cases"][c[1]]) == (c[4] != "grad"), c[1]
    REC.check_not_degenerate(CASES, GOLDEN["cases"])


@functools.lru_cache(maxsize=None)
def _environment_differs():
    env = REC.environment()
    for key in ("cu_count", "hipcc_version"):
        if env[key] != GOLDEN[key]:
            return (f"{key} is {env[key]!r}, the record was made with {GOLDEN[key]!r}: build the commit before the refactor as a "
                    "tagged library and record again with GPV_LIB=<that library> python tools/grad_family_record.py "
                    "tests/golden/grad_family_bits.json")
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted({c[0] for c in CASES}))
def test_bits(group):
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    why = _environment_differs()
    if why:
        pytest.skip(why)
    todo = [c for c in CASES if c[0] == group]
    got = REC.run_no_table() if group == REC.NO_TABLE else REC.run(todo)
    assert set(got) == {c[1] for c in todo}
    differ = [(c[1], f) for c in todo for f in FIELDS if got[c[1]].get(f) != GOLDEN["cases"][c[1]].get(f)]
    print(f"{group}: {len(todo)} cases, {len(differ)} fields differ from the record")
    assert not differ, differ[:10]
