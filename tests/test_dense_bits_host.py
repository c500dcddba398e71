"""The update-mark arithmetic every dense checkpoint kernel uses
(deeprec-1_amd/csrc/dr_dense_bits.h: word index, mask, the last word's valid
mask, a set bit's rank inside its word), compiled into a stand-alone host
program (tools/dense_bits_check.cpp) and checked against Python integers at
the word boundaries and past 2^31 rows.  The program is built twice, plainly
and with -fsanitize=address,undefined, and both are run directly."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [1, 31, 32, 33, 64, (1 << 31) + 1]


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def exe(request, tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler (g++, c++ or clang++)"
    path = str(tmp_path_factory.mktemp("dense_bits") / ("dense_bits_check_" + request.param))
    flags = ["-O2"] if request.param == "plain" else \
        ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "deeprec-1_amd", "csrc"),
                    os.path.join(ROOT, "tools", "dense_bits_check.cpp"), "-o", path], check=True)
    return path


def _pairs(rows, seed):
    rng = random.Random(seed)
    last = rows - 1
    picks = {0, last, last // 2, max(last - 1, 0), min(31, last), min(32, last), min(33, last),
             last & ~31, max((last & ~31) - 1, 0)}
    picks |= {rng.randrange(rows) for _ in range(200)}
    words = [0, 0xFFFFFFFF, 0x80000000, 1, 0x55555555, 0xAAAAAAAA]
    out = []
    for r in sorted(picks):
        for w in words + [rng.getrandbits(32) for _ in range(4)]:
            out.append((r, w))
    return out


def _popcount(x):
    return bin(x).count("1")


@pytest.mark.parametrize("rows", ROWS)
def test_bits_match_python_integers(exe, rows):
    pairs = _pairs(rows, 77 + rows % 97)
    r = subprocess.run([exe, str(rows)], input="".join("%d %d\n" % p for p in pairs),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(pairs) + 1
    nw = (rows + 31) // 32
    tail = (1 << (rows % 32)) - 1 if rows % 32 else 0xFFFFFFFF
    assert tuple(int(x) for x in lines[0].split()) == (nw, tail)
    for (row, word), line in zip(pairs, lines[1:]):
        got = tuple(int(x) for x in line.split())
        w, b = row // 32, row % 32
        valid = tail if w == nw - 1 else 0xFFFFFFFF
        assert got == (row, w, 1 << b, _popcount(word & ((1 << b) - 1)), valid), (rows, row, word)
        assert valid & (1 << b), "a row of the table is a valid bit of its word"


def test_usage_errors(exe):
    assert subprocess.run([exe], capture_output=True).returncode == 2
    assert subprocess.run([exe, "0"], capture_output=True).returncode == 2
    assert subprocess.run([exe, "5"], input=b"-1 0\n", capture_output=True).returncode == 2
