"""A plain bench.py run (no --full) on a small table set: it times exactly
--steps steps, prints one result line whose extra legs are null, and with
--dump-outputs writes the last timed step's output -- checked here against
the tables' regenerable rows (synth(1000 + t, key, :)) for the batch that
step read.  6 steps = one 4-step hipGraph replay + 2 eager steps, so the
last timed step is an eager one on batch 1; 8 steps = two replays, the last
step the graph's fourth."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, R, D, B, STEPS = 4, 200_000, 128, 4096, 6


@pytest.mark.parametrize("steps", [STEPS, 8])
def test_plain_run_dumps_last_step(tmp_path, steps):
    import bench
    out_dir = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
           "--warmup", "2", "--tables", str(T), "--rows", str(R), "--dim", str(D),
           "--batch", str(B), "--dump-outputs", out_dir]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    line = lines[0]
    assert line["steps"] == steps and line["full"] is False and line["n_gpus"] == 1
    assert line["unit"] == "lookups/s" and line["higher_is_better"] is True
    assert line["dtype"] == "fp32" and line["ms_per_step"] > 0
    # value and ms_per_step are the same measurement (ms_per_step is printed
    # to 1e-4 ms, a step of this size takes some 0.02 ms or more)
    assert line["value"] == pytest.approx(T * B / (line["ms_per_step"] * 1e-3), rel=1e-2)
    for k in ("train_step", "dlrm_train_step", "din_config", "deepfm_config", "native_engine",
              "criteo_tb_cardinalities", "criteo_tb_hybrid", "dcn_bf16_config", "correctness",
              "roofline", "roofline_row_gather", "cpu_baseline"):
        assert line[k] is None, k
    assert os.listdir(out_dir) == ["embedding_output.npy"]
    got = np.load(os.path.join(out_dir, "embedding_output.npy"))
    assert got.dtype == np.float32 and got.shape == (B, T * D)
    ids = bench.make_batches(4, T, B, R, 0.0, 2021, "cuda:0")[(steps - 1) % 4].cpu().numpy()
    for t in range(T):
        np.testing.assert_array_equal(got[:, t * D:(t + 1) * D],
                                      bench.synth_rows(1000 + t, ids[t], D))
