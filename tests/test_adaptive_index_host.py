"""dr_adaptive_bucket / dr_adaptive_row_valid (deeprec-1_amd/csrc/
dr_adaptive.h), the bucket rule every adaptive kernel uses, compiled into a
stand-alone host program (tools/adaptive_index_check.cpp) and checked against
Python's %: floormod(id, bucket_size) with floor semantics for negative ids is
always a row of the hash table, on both division paths (32-bit and 64-bit)."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler (g++, c++ or clang++)"
    path = str(tmp_path_factory.mktemp("adaptive") / "adaptive_index_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "deeprec-1_amd", "csrc"),
                    os.path.join(ROOT, "tools", "adaptive_index_check.cpp"), "-o", path],
                   check=True)
    return path


def _ids(n, seed):
    rng = random.Random(seed)
    ids = [0, 1, n - 1, n, n + 1, -1, -n, -n - 1, -7, (1 << 40) + 3, (1 << 32) - 1, 1 << 32,
           I64_MIN, I64_MAX]
    ids += [rng.randrange(I64_MIN, I64_MAX + 1) for _ in range(1500)]     # anywhere
    ids += [rng.randrange(-2 * n - 2, 2 * n + 2) for _ in range(1500)]    # near the table
    ids += [rng.randrange(-(1 << 33), 1 << 33) for _ in range(1000)]      # both division paths
    return [min(max(i, I64_MIN), I64_MAX) for i in ids]


@pytest.mark.parametrize("n", [5, 1, 100003, (1 << 31) + 1, (1 << 32) + 7])
def test_bucket_rule_matches_python_floor_mod(exe, n):
    ids = _ids(n, 2000 + n % 89)
    r = subprocess.run([exe, str(n)], input="\n".join(map(str, ids)) + "\n", capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(ids)
    for i, line in zip(ids, lines):
        got = tuple(int(x) for x in line.split())
        assert got == (i, i % n, int(0 <= i < n)), (n, i, got)
        assert 0 <= got[1] < n


def test_usage_errors(exe):
    assert subprocess.run([exe], capture_output=True).returncode == 2
    assert subprocess.run([exe, "0"], capture_output=True).returncode == 2
