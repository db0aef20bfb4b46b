"""The carry-free 64-bit reciprocal multiply of the ROC chain encoders (U2_DIV in csrc/roc_u2.h, restated in csrc/u2_div_ref.h)
against unsigned __int128, built with g++ (no HIP, no GPU)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_u2_div_flow(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path / "u2_div_test")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "u2_div_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "u2 div ok" in out.stdout, out.stdout + out.stderr
