"""dr::overlay_lower_bound / dr::overlay_find (deeprec-1_amd/csrc/dr_overlay.h),
the search both kernels of the host-tier serving overlay use (DESIGN section
19), against std::lower_bound on the host (g++, tools/overlay_check.cpp): random
sorted int64 ranges, back-to-back ranges of a grouped overlay with an empty
one in between, an empty range, M = 1, the keys -1, 0, INT64_MIN and INT64_MAX,
and probes below, above, between and on the keys."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ absent")
@pytest.mark.parametrize("seed", [1, 7, 2021])
def test_overlay_search_matches_std_lower_bound(tmp_path, seed):
    exe = str(tmp_path / "overlay_check")
    subprocess.run(["g++", "-O2", "-std=c++17",
                    "-I", os.path.join(ROOT, "deeprec-1_amd", "csrc"),
                    os.path.join(ROOT, "tools", "overlay_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "1500", str(seed)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "mismatches 0" in r.stdout
