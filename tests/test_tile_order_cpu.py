"""The index arithmetic every GEMM (and the strip kernels of norm.hip) rests on -- XCD remap, persistent work-unit ranges, super-tile order,
split-K ranges, the tap decode of the descriptor-addressed implicit GEMMs, the packed pixel word -- is stated once in
unicorn_amd/csrc/tile_index.h and compiles for the host as well.  tools/tile_index_check.cpp checks each function over its stated domain by
exhaustion; csrc/build.sh builds it with g++.  No GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_index_functions_hold_over_their_domains():
    exe = os.path.join(ROOT, "tools", "build", "tile_index_check")
    if not os.path.exists(exe):
        pytest.fail("tools/build/tile_index_check is missing: run __graft_entry__.build() (csrc/build.sh builds it)")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tile_index_check: OK" in r.stdout
    # the bound the launchers use (gemm_h2d_supported / gemm_h2q_supported) is the one the exhaustion proved, and the next value fails
    header = open(os.path.join(ROOT, "unicorn_amd", "csrc", "tile_index.h")).read()
    bound = int(re.search(r"constexpr int TAP_DECODE_MAX_CS = (\d+);", header).group(1))
    assert "proved bound TAP_DECODE_MAX_CS = %d" % bound in r.stdout
    assert "cs = %d, K step" % (bound + 1) in r.stdout
    for unit in ("gemm_h2d.hip", "gemm_h2q.hip"):
        text = open(os.path.join(ROOT, "unicorn_amd", "csrc", unit)).read()
        assert "> TAP_DECODE_MAX_CS" in text and "> 448" not in text, unit
