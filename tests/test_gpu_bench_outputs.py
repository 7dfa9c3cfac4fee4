"""bench.py at one GPU without --full: the result line carries the headline and nothing that needs runs of its own, and
--dump-outputs writes what the last timed step computed, the same arrays from run to run.  Fresh child processes only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 200_000


def _bench(out_dir, steps):
    e = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", str(N), "--mode", "U",
                        "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    return json.loads(lines[-1])


def test_plain_run_is_lean_and_dumps_the_same_outputs_every_run(tmp_path):
    j = _bench(tmp_path / "a", 3)
    assert j["metric"] == "vecchia_loglik_evals_per_sec" and j["unit"] == "evals/s" and j["higher_is_better"] is True
    assert j["dtype"] == "f64" and j["steps"] == 3 and j["value"] > 0
    assert abs(j["ms_per_step"] - 1e3 / j["value"]) <= 1e-9 * j["ms_per_step"]
    assert j["roofline"]["kernel_ms"] > 0
    assert not {"cpu_baseline", "secondary", "parity_in_run", "self_check"} & set(j) and "from_idle" not in j["config"]
    a = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(a) == ["Lentries_sample.npy", "Lentries_sample_rows.npy", "loglik.npy", "sums.npy"]
    assert a["loglik.npy"][0] == j["config"]["loglik"] and a["sums.npy"][7] == N
    rows = a["Lentries_sample_rows.npy"].astype(np.int64)
    assert rows.size == N and np.array_equal(rows, np.arange(N))          # 200 000 x 31 doubles fit the 48 MB sample whole
    L = a["Lentries_sample.npy"]
    assert L.shape == (N, 31) and np.all(L[rows, np.minimum(rows, 30)] > 0)   # the diagonal entry of every row
    j2 = _bench(tmp_path / "b", 5)
    assert j2["steps"] == 5
    for f, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / f)), f
