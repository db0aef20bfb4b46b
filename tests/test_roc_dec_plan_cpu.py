"""The planning half of the ROC decoder's host call (csrc/roc_dec_plan.h): class cascade, by-length against per-list route, promotion
to the chain kernels, scratch / slot layout and stream assignment, built with g++ (no HIP, no GPU)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_roc_decode_plan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path / "roc_dec_plan_test")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "roc_dec_plan_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "roc dec plan ok" in out.stdout, out.stdout + out.stderr
