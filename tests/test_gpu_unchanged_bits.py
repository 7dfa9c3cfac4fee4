"""'matern' and 'esqe' compute what the commit before 'matern_scaledim' computed, bit for bit.

No committed number: the record is made from the parent's build.  tools/eval_bits_record.py finds the parent commit in the git
history (the newest one whose gpv_api.hip does not know the family), builds its library once with its own build.py -- a tagged
build of the two row lengths the cases use, kept in an ignored folder for the next run -- and this test runs the tool's record()
in two fresh child processes, one of them with GPV_LIB naming that library (the library is chosen when the package is imported).
The records -- SHA-256 of the sums and U entries of evaluations through the general, the likelihood-only and the lean set
kernels, of the posterior pass and its replay, and of gpv_plan_loglik_grad, for Matern 0.5 / 1.5 / 2.5 / 0.8 and esqe, d = 2 and 5,
m = 10 and 30 -- must be equal.  GPV_PARENT_LIB names a parent library built elsewhere.  Where there is neither (a tree without
git history) the comparison cannot be made and the test skips, saying so.

The first run compiles the parent's library (minutes); the runs after it take a few seconds."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "eval_bits_record.py")
_spec = importlib.util.spec_from_file_location("eval_bits_record", TOOL)
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)


def _record(tmp_path, name, lib):
    out = str(tmp_path / (name + ".json"))
    env = {k: v for k, v in os.environ.items() if k != "GPV_LIB"}
    if lib:
        env["GPV_LIB"] = lib
    r = subprocess.run([sys.executable, TOOL, out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(out) as f:
        return json.load(f)


@pytest.mark.gpu
def test_matern_and_esqe_are_bitwise_the_parents(tmp_path):
    import gpvecchia_amd as G
    if G.device_count() < 1:
        pytest.fail("gpu-marked test but libgpvecchia_hip sees no HIP device")
    lib = REC.parent_library()
    if lib is None:
        pytest.skip("no parent build to compare with: no git history here and GPV_PARENT_LIB is not set")
    new, parent = _record(tmp_path, "new", None), _record(tmp_path, "parent", lib)
    assert len(new) == 66 and set(new) == set(parent)
    # the three set kernels were reached (the record's keys name the kernel of the likelihood-only launch)
    assert any("lik kernel 3" in k for k in new) and any("lik kernel 1" in k for k in new) and any("lik kernel 0" in k for k in new)
    differ = sorted(k for k in new if new[k] != parent[k])
    print(f"{len(new)} records, {len(differ)} differ from the parent's build ({lib})")
    assert not differ, differ[:10]
