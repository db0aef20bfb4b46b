"""CPU: the word-granular LDS geometry of the 20-bit ROC chain decoder (csrc/roc_u2_geom.h, U2DecWord) -- u16 rows and bitmap
disjoint and exactly the 163 840 bytes a workgroup can have; for every id below 2^20 the row element, the bitmap word, the insertion
dword and all 64 lanes' packed-add and zero-OR targets in bounds, lane 0's target no other lane's; a model of the packed add over
one full level-1 block in ascending, descending and shuffled order against plain per-word prefix counts (no carry between fields).
tests/roc_u2_decword_geom_test.cpp is built with g++ like tests/roc_u2_geom_test.cpp (no HIP, no GPU)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_u2_word_row_geometry_on_the_host(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path / "roc_u2_decword_geom_test")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "roc_u2_decword_geom_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines[-1] == "roc u2 word-row geometry ok", out.stdout[-3000:] + out.stderr
    assert lines[0] == "word-row decoder: 163840 bytes"
    assert sum("shuffled" in ln for ln in lines) == 3
