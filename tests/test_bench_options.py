"""bench.py's --full and --dump-outputs on the host: the options parse, a
plain run is the default, and dump_outputs() writes float32 arrays whose row
sample is fixed and stays under the size bound."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(argv):
    import bench
    old = sys.argv
    sys.argv = ["bench.py"] + argv
    try:
        return bench.parse()
    finally:
        sys.argv = old


def test_plain_run_is_the_default():
    a = _parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    a = _parse(["--full", "--dump-outputs", "somewhere"])
    assert a.full is True and a.dump_outputs == "somewhere"


def test_dump_small_output_whole(tmp_path):
    import bench
    t = torch.arange(37 * 24, dtype=torch.float32).reshape(37, 24)
    bench.dump_outputs(str(tmp_path / "d"), {"embedding_output": t}, 0, 1)
    a = np.load(tmp_path / "d" / "embedding_output.npy")
    assert a.dtype == np.float32
    np.testing.assert_array_equal(a, t.numpy())


def test_dump_large_output_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1000 * 4)   # 1000 floats
    t = torch.randn((301, 16), generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"out": t}, 0, 1)
    a, b = np.load(tmp_path / "a" / "out.npy"), np.load(tmp_path / "b" / "out.npy")
    assert a.dtype == np.float32 and a.shape == (62, 16) and a.nbytes <= 1000 * 4
    np.testing.assert_array_equal(a, b)
    # the sample: distinct rows of the output, in ascending order
    full = t.float().numpy()
    idx = [int(np.flatnonzero((full == r).all(1))[0]) for r in a]
    assert idx == sorted(set(idx))
    # N = 2: each rank its own file, the bound shared
    bench.dump_outputs(str(tmp_path / "c"), {"out": t}, 1, 2)
    c = np.load(tmp_path / "c" / "out.rank1.npy")
    assert c.shape == (31, 16)
