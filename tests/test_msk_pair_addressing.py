"""The timing recovery's pair-loop address helpers (gr-ais_amd/csrc/aisx_common.h: mmse_row_off, ring_read_off)
against the formulas they replace, on the host: every float mu in [0, 1] through the tap row (rintf(mu * 128)), and
the role-aware ring offset for every ring layout (tests/emul_addr/addr_check.cpp, built with g++)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pair_loop_addresses_match_the_old_formulas(tmp_path):
    exe = str(tmp_path / "addr_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
                    "-I", os.path.join(ROOT, "gr-ais_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "emul_addr", "addr_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ")
