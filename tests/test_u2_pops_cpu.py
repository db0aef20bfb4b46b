"""The one-test, one-shift slice pops of the bitmap chain decoder (U2_DEC_TOP_P in csrc/roc_u2.h, restated in csrc/u2_pops_ref.h)
against the two pops of codec.cpp, built with g++ (no HIP, no GPU); and the Python port tests/roc_pops_ref.py against that program."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roc_pops_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    path = str(tmp_path_factory.mktemp("u2_pops") / "u2_pops_test")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-o", path, os.path.join(ROOT, "tests", "u2_pops_test.cpp")])
    return path


def test_u2_pops_forms_agree(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0 and "u2 pops ok" in out.stdout, out.stdout + out.stderr


def test_python_port_equals_the_header(exe):
    rng = np.random.default_rng(5)
    rows = []
    for P in range(1, 21):
        p1, p0 = ref.pop_widths(P)
        t1, t0 = 1 << (31 + p1), 1 << (31 + p1 + p0)
        heads = [ref.L, t1 - 1, t1, t1 + 1, t0 - 1, t0, t0 + 1, (1 << 63) - 1]
        heads += [max(int(h) >> int(s), 0) | ref.L for h, s in zip(rng.integers(0, 1 << 63, 200, dtype=np.uint64) * 2 + 1, rng.integers(0, 33, 200))]
        rows += [(h, int(w), P) for h, w in zip(heads, rng.integers(0, 1 << 32, len(heads), dtype=np.uint64)) if h >= ref.L]
    assert len(rows) > 4000
    text = "".join(f"{h} {w} {P}\n" for h, w, P in rows)
    out = subprocess.run([exe, "eval", str(len(rows))], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")[:len(rows)]
    for (h, w, P), line in zip(rows, lines):
        v = [int(t) for t in line.split()]
        p1, p0 = ref.pop_widths(P)
        words = iter([w, w ^ 0xffffffff])
        assert tuple(v[0:4]) == ref.pops_two(h, p1, p0, lambda: next(words)), (h, w, P)
        assert tuple(v[4:8]) == ref.pops_one(h, w, p1, p0), (h, w, P)
        assert v[0:4] == v[4:8]
