"""CPU: csrc/ef_rank_ref.h -- the arithmetic the rank kernels call -- built with g++ as a stand-alone program (tests/ef_rank_test.cpp, own
main), plain and with -fsanitize=address,undefined, against cases the numpy model (tests/ef_rank_ref.py) writes out: every designed
list and a sample of the lists_ref families, every query of ef_rank_ref.queries."""
import os
import shutil
import subprocess

import pytest

import ef_rank_ref as er
import lists_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp, flags, name):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    path = str(tmp / name)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", *flags, "-o", path,
                           os.path.join(ROOT, "tests", "ef_rank_test.cpp")])
    return path


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ef_rank")
    return {"plain": _build(tmp, [], "ef_rank_test"),
            "sanitized": _build(tmp, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "ef_rank_test_san")}


@pytest.fixture(scope="module")
def cases():
    d = er.designed()
    lists = [d[k] for k in sorted(d)]
    for fam in ("quotient_edges", "low_widths", "batch_seams", "constant_runs"):
        lists += [li for li in lr.family(fam) if li.size <= 4200][::3]
    text = er.case_text(lists)
    nq = sum(er.queries(li).size for li in lists)
    return text, len(lists), nq


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_self_checks(exes, which):
    out = subprocess.run([exes[which]], capture_output=True, text=True)
    assert out.returncode == 0 and "ef rank ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_header_equals_the_numpy_model(exes, cases, which):
    text, nlists, nq = cases
    assert nlists > 40 and nq > 20000
    out = subprocess.run([exes[which], "cases"], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert f"{nlists} lists, {nq} queries" in out.stdout and "ef rank ok" in out.stdout, out.stdout[-2000:]
