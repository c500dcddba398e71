"""The flag-word methods of dr::HostTier (count_masked / export_masked /
clear_bits / or_bits / shrink_keys) walked against std::map
under AddressSanitizer and UndefinedBehaviorSanitizer:
tools/host_tier_flags_check.cpp is a stand-alone program (its own main, the
header only), built and run on the host as tests/test_host_tier_sanitized.py
does -- nothing is preloaded and nothing loaded into Python is sanitized."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ absent")
def test_host_tier_flag_walk_is_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "host_tier_flags_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "deeprec-1_amd", "csrc"),
                    os.path.join(ROOT, "tools", "host_tier_flags_check.cpp"), "-o", exe],
                   check=True)
    for seed in ("2", "11"):
        r = subprocess.run([exe, "2500", seed], capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        assert "mismatches 0" in r.stdout
        words = r.stdout.split()
        assert int(words[words.index("buckets") + 1]) >= 8 * 2 ** 4, r.stdout   # it rehashed
        assert int(words[words.index("flagged") + 1]) > 100, r.stdout
        assert int(words[words.index("aged") + 1]) > 100, r.stdout
