"""GPU tier: a plain bench.py run (the timed steps and the line, nothing
else) and its --dump-outputs: the dumped array is the last timed step's
output, bit for bit the oracle's sum of the same generator -- whole below the
dump limit, the fixed seeded sample (bench.dump_indices) above it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("log2count", [16, 24])  # the whole output; a sample (2^24 > bench.DUMP_MAX_ELEMS)
def test_plain_run_line_and_dump(oracle, tmp_path, log2count):
    import bench
    n, count, steps = 3, 1 << log2count, 3
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--n", str(n), "--log2count", str(log2count), "--dump-outputs", str(tmp_path / "dump")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert (r["metric"], r["unit"], r["higher_is_better"], r["dtype"]) == (bench.METRIC, "GB/s", True, "f32")
    assert r["steps"] == steps and r["warmup"] == 1 and r["full"] is False
    assert r["ms_per_step"] > 0
    # value = bytes per step / the time of one step (one rank); the line rounds
    # ms_per_step to 1e-4 ms and value to 0.01 GB/s
    rel = 5e-5 / r["ms_per_step"] + 0.005 / r["value"] + 1e-6
    assert r["value"] == pytest.approx((n + 1) * count * 4 / (r["ms_per_step"] * 1e-3) / 1e9, rel=rel)
    # a plain run measures nothing but its steps
    assert r["cpu_baseline"] is None and r["parity_full"] is None and r["parity_sample_ok"] is None
    assert r["roofline"]["mix_ceiling_GBps"] is None and r["roofline"]["copy_ceiling_GBps"] is None
    assert "c2_misaligned" not in r and "c2_layout_ab" not in r and "c5" not in r
    assert os.listdir(tmp_path / "dump") == ["out.npy"]
    got = np.load(tmp_path / "dump" / "out.npy")
    idx = bench.dump_indices(count)
    assert (idx is None) == (count <= bench.DUMP_MAX_ELEMS)
    if idx is None:
        exp = oracle.reduce(list(oracle.fill(n, count, bench.SEED)))
    else:
        exp = oracle.sample_sum(idx, bench.SEED, n)
    assert got.dtype == np.float32 and got.shape == exp.shape
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
