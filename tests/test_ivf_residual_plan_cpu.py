"""CPU: csrc/ivf_residual_ref.h and csrc/ivf_residual_plan.h as a stand-alone program (tests/ivf_residual_test.cpp), built with g++ and
once more with -fsanitize=address,undefined: the serial scan, count and fill against cases the numpy model writes out (S of 1 and 4),
the plan against a written-out table, and the one-CU batches of the GPU test."""
import os
import shutil
import subprocess

import pytest

import ivf_residual_ref as rs
import ivf_scan_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ivf_residual_test.cpp")


@pytest.fixture(scope="module", params=("plain", "sanitized"))
def exe(request, tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    path = str(tmp_path_factory.mktemp("ivf_residual_" + request.param) / "ivf_residual_test")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", *extra, "-o", path, SRC])
    return path


def test_self_checks(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ivf residual ok" in out.stdout, out.stdout + out.stderr


def test_serial_form_against_the_model(exe):
    cases = []
    for d, M in rs.FORMS:
        o = rs.obj(d, M)
        xq = rs.queries(d, len(rs.EDGE_ROWS))
        cases.append((o, xq, rs.EDGE_ROWS, 64, rs.radii(d, M)[1]))
        cases.append((o, rs.queries(d, 4), ir.probe_rows(4, 7), 10, float("inf")))
    s = rs.shape("ties")
    cases.append((s, s["xq"][:8], s["probes"][:8], s["k"], 6.0))
    out = subprocess.run([exe, "cases"], input=rs.cases_text(cases), capture_output=True, text=True)
    assert out.returncode == 0 and "ivf residual ok" in out.stdout and f"{len(cases)} cases, {2 * len(cases)} runs" in out.stdout, \
        out.stdout[-2000:] + out.stderr[-2000:]


def plan(exe, nq, num_cu, d, M, nprobe, k):
    out = subprocess.run([exe, "plan", *map(str, (nq, num_cu, d, M, nprobe, k))], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    names = ("lds", "resident", "S", "items", "nslots", "scratch", "lo", "hi", "W", "merge_lds")
    scan, rng = (dict(zip(names, map(int, line.split()))) for line in out.stdout.strip().splitlines())
    return scan, rng


# nq, num_cu, d, M, nprobe, k -> scan (lds, resident, S, nslots, scratch), range (lds, resident, S, nslots, scratch)
PLAN_TABLE = [
    ((10, 256, 128, 16, 16, 20), (18560, 2048, 16, 160, 10 * 16 * 21 * 8), (17472, 2304, 16, 160, 640)),     # the reference shape
    ((1000, 256, 128, 16, 16, 20), (18560, 2048, 4, 2048, 1000 * 4 * 21 * 8), (17472, 2304, 4, 2304, 64000)),
    ((10000, 256, 128, 16, 16, 20), (18560, 2048, 1, 2048, 0), (17472, 2304, 1, 2304, 640000)),
    ((10, 256, 128, 16, 1, 20), (18512, 2048, 1, 10, 0), (17424, 2304, 1, 10, 40)),                           # S <= nprobe
    ((1, 256, 2048, 64, 1024, 256), (90880, 256, 16, 16, 16 * 257 * 8), (86016, 256, 16, 16, 4096)),         # the limits: one per CU
    ((3, 1, 128, 16, 16, 20), (18560, 8, 4, 8, 3 * 4 * 21 * 8), (17472, 9, 4, 9, 192)),                        # one compute unit
    ((3, 1, 4, 4, 3, 10), (5072, 32, 2, 6, 3 * 2 * 11 * 8), (4144, 32, 2, 6, 36)),
]


@pytest.mark.parametrize("args,want_scan,want_range", PLAN_TABLE)
def test_the_plan_against_written_out_tables(exe, args, want_scan, want_range):
    nq, num_cu, d, M, nprobe, k = args
    for p, want, kk in zip(plan(exe, *args), (want_scan, want_range), (k, 0)):
        assert (p["lds"], p["resident"], p["S"], p["nslots"], p["scratch"]) == want, p
        assert p["lds"] == rs.plan_lds(kk, nprobe, d, M) and p["resident"] == rs.plan_resident(num_cu, p["lds"])
        assert p["S"] == rs.plan_pieces(nq, nprobe, p["resident"]) and p["items"] == nq * p["S"]
        assert p["lds"] * (p["resident"] // num_cu) <= 160 * 1024
        assert p["W"] == max(w for w in (1, 2, 4, 8, 16) if M % w == 0) and p["merge_lds"] == (p["S"] * k * 8 if kk else 0)


def test_the_one_cu_batches_go_round_the_grid_stride_loop(exe):
    b = rs.ONE_CU
    args = (1, b["d"], b["M"], b["nprobe"], b["k"])
    for i, resident in enumerate((8, 9)):  # scan, range
        whole, cut = plan(exe, b["nq_whole"], *args)[i], plan(exe, b["nq_cut"], *args)[i]
        assert whole["resident"] == cut["resident"] == resident
        assert whole["S"] == 1 and whole["nslots"] == resident
        assert whole["lo"] >= 3 and whole["hi"] == whole["lo"] + 1  # every slot takes three items, some a fourth: a ragged last trip
        assert cut["S"] == 4 and cut["nslots"] == resident and (cut["lo"], cut["hi"]) == (1, 2)  # some slots go round, some do not
    assert plan(exe, b["nq_whole"], *args)[0]["scratch"] == 0 and plan(exe, b["nq_cut"], *args)[0]["scratch"] == b["nq_cut"] * 4 * (b["k"] + 1) * 8
