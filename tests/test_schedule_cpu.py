"""The row-block kernel's workgroup -> cell schedule (csrc/lec_schedule.h) on the host: tests/sched/schedule_check.cpp includes the
header the kernel includes, walks every workgroup index of the grids of its sweep (box heights 1..130 and 721, 1..9 and 64 time steps,
1 / 2 / 37 levels, four block shapes, 25 tile requests) and checks that every cell is produced exactly once, none outside the ranges,
no cell in two XCDs' chunks, and the XCDs' row walks within one (cell, time group) unit of their mean.  Built with
-fsanitize=address,undefined as a stand-alone program; no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_every_cell_once_and_the_xcds_balanced(tmp_path):
    exe = tmp_path / "schedule_check"
    r = subprocess.run([CXX, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                        os.path.join(ROOT, "tests", "sched", "schedule_check.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    print(r.stdout.strip())
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.startswith("393000 combinations") and r.stdout.rstrip().endswith(" 0 failures"), r.stdout
