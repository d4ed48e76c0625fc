"""bench.py's options that decide what a run does beyond its headline, checked without a GPU."""
import os
import subprocess
import sys

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_full_is_off_by_default_and_write_digest_needs_it():
    assert bench.parse_args([]).full is False and bench.parse_args(["--full"]).full is True
    # refused before anything touches a GPU: a plain run computes no digest, so it would silently write none
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--write-digest"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode != 0 and "--write-digest needs --full" in r.stderr and not r.stdout.strip()
