"""CPU: the LDS geometry of the round-2 ROC chain kernels (csrc/roc_u2_geom.h) -- the dense encoder's base table, slots, pad and
strip, and the bitmap decoder's u32 rows, natural-order bitmap and strip: no overlap, everything a step addresses in bounds (all
4096 (L1, lane) pairs of the decoder's rows), every launch within the 163 840 bytes a workgroup can have.
tests/roc_u2_geom_test.cpp is built with g++ like tests/roc_rows_geom_test.cpp (no HIP, no GPU)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_u2_geometry_on_the_host(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path / "roc_u2_geom_test")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "roc_u2_geom_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines[-1] == "roc u2 geometry ok", out.stdout[-3000:] + out.stderr
    assert lines[0] == "dense encoder: 147856 bytes"
    assert "decoder UB 20: 147712 bytes" in lines and "decoder UB 18: 49408 bytes" in lines
