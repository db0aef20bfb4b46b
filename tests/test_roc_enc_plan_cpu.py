"""The planning half of the ROC encoder's host call (csrc/roc_enc_plan.h): kernel classes, work lists, chain promotion, octaves, perm
items and the schedule grammar, built with g++ (no HIP, no GPU)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_roc_encode_plan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path / "roc_enc_plan_test")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "roc_enc_plan_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "roc enc plan ok" in out.stdout, out.stdout + out.stderr
