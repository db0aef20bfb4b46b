"""CPU: the numpy model of the IVF list scan (tests/ivf_scan_ref.py) against a brute-force double loop written from include/vidc.h, on
the shared shapes and the designed objects, whole and cut into S pieces; the shapes hold what they are named for;
csrc/ivf_scan_ref.h + ivf_scan_plan.h built with g++ as a stand-alone program (tests/ivf_scan_test.cpp), plain and with
-fsanitize=address,undefined, against cases the model writes out, every case as one piece and as S pieces merged."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ivf_scan_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PQ_FORMS = ((1, 4), (4, 1), (16, 8), (64, 2))  # (M, dsub)
DIMS = (1, 3, 4, 20, 128)
KS = (1, 64, 65, 256)
NPROBES = (1, 3, 16, 17, 1024)


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("D", "labels", "stats")):
        assert np.array_equal(np.asarray(g), np.asarray(w)), f"{what}: {name} differs"


@pytest.mark.parametrize("name", sorted(ir.SHAPES))
def test_model_equals_the_brute_force_on_the_shapes(name):
    s = ir.shape(name)
    nq = 12
    want = ir.brute_force(s["offsets"], s["vecs"], s["xq"][:nq], s["probes"][:nq], s["k"])
    assert_same([a[:nq] for a in ir.expected(name)], want, name)


def test_model_equals_the_brute_force_on_the_designed_objects():
    for d, M in [(d, 0) for d in DIMS] + [(M * dsub, M) for M, dsub in PQ_FORMS]:
        o = ir.obj(d, M)
        xq = ir.queries(d, len(ir.EDGE_ROWS))
        for k in (1, 64, 65):
            assert_same(ir.model(o["offsets"], o["vecs"], xq, ir.EDGE_ROWS, k), ir.brute_force(o["offsets"], o["vecs"], xq, ir.EDGE_ROWS, k), (d, M, k))
    o = ir.obj(4)
    for nprobe in NPROBES:
        rows = ir.probe_rows(6, nprobe)
        assert_same(ir.model(o["offsets"], o["vecs"], ir.queries(4, 6), rows, 256), ir.brute_force(o["offsets"], o["vecs"], ir.queries(4, 6), rows, 256), nprobe)


def test_the_result_does_not_depend_on_the_cut():
    o = ir.obj(4)
    for nprobe in (3, 16, 17):
        rows, xq = ir.probe_rows(8, nprobe), ir.queries(4, 8)
        whole = ir.model(o["offsets"], o["vecs"], xq, rows, 20)
        for S in (2, 4, 8, 16):
            assert_same(ir.model(o["offsets"], o["vecs"], xq, rows, 20, S=S), whole, (nprobe, S))
    s = ir.shape("ties")
    assert_same(ir.model(s["offsets"], s["vecs"], s["xq"], s["probes"], s["k"], S=4), ir.expected("ties"), "ties S=4")


def test_model_rules():
    off = np.array([0, 2, 2, 5], np.uint64)  # lists of 2, 0 and 3 entries
    vecs = np.array([[0], [3], [1], [3], [0]], np.float32)
    probes = np.array([[2, 0, 2, -1], [1, 3, 2 ** 40, -7], [0, 0, 0, 0]], np.int64)
    D, L, st = ir.model(off, vecs, np.zeros((3, 1), np.float32), probes, 4)
    assert D[0].tolist() == [0, 0, 1, 9] and L[0].tolist() == [0, (2 << 32) | 2, 2 << 32, 1]  # ties by label; list 2 scanned once
    assert st.tolist() == [[2, 5], [1, 0], [1, 2]]
    assert np.isinf(D[1]).all() and (L[1] == -1).all()
    assert D[2].tolist()[:2] == [0, 9] and np.isinf(D[2, 2:]).all() and L[2].tolist() == [0, 1, -1, -1]


def test_the_shapes_hold_what_they_are_named_for():
    for name in ir.SHAPES:
        s = ir.shape(name)
        assert s["d"] * (2 * s["R"]) ** 2 < 2 ** 24 and np.array_equal(s["vecs"], np.round(s["vecs"])) and np.abs(s["vecs"]).max() <= s["R"]
        assert all(len(set(r.tolist())) == s["nprobe"] for r in s["probes"])
        D, L, st = ir.expected(name)
        assert np.isfinite(D).all() and (st[:, 0] == s["nprobe"]).all() and (st[:, 1] > 64).all()  # more than one trip per query
    s = ir.shape("distinct")
    free = ir.tie_free(s["offsets"], s["vecs"], s["xq"], s["probes"], s["k"])
    assert free.sum() * 4 >= 3 * s["nq"], int(free.sum())
    s = ir.shape("ties")
    D = ir.model(s["offsets"], s["vecs"], s["xq"], s["probes"], s["k"] + 1)[0]
    inside = [(np.diff(row[: s["k"]]) == 0).any() for row in D]
    across = [row[s["k"] - 1] == row[s["k"]] for row in D]
    assert all(inside) and sum(across) * 2 >= s["nq"], (sum(inside), sum(across))


def test_the_designed_objects_hold_what_they_are_named_for():
    sizes = list(ir.EDGE_SIZES)
    assert {0, 1, 63, 64, 65, 129} <= set(sizes) and max(sizes) > 256
    rows, nlist = ir.EDGE_ROWS, len(sizes)
    k = 64
    alone = [sizes[int(r[0])] for r in rows[:3]]
    assert alone == [k - 1, k, k + 1] and all((r[1:] == -1).all() for r in rows[:3])
    flat = rows.reshape(-1).tolist()
    assert -1 in flat and nlist in flat and 2 ** 40 in flat
    counts = [max(np.bincount(r[(r >= 0) & (r < nlist)], minlength=1)) for r in rows]
    assert 2 in counts and 3 in counts
    assert any(not ir.valid_lists(r, nlist) for r in rows)  # a row of only invalid probes
    for M, dsub in PQ_FORMS:
        o = ir.obj(M * dsub, M)
        assert np.array_equal(o["codebooks"], np.round(o["codebooks"])) and o["codes"].shape == (o["ntotal"], M)
    wide = ir.probe_rows(6, 1024)
    assert (wide == -1).any() and (wide == nlist).any() and all(len(ir.valid_lists(r, nlist)) == nlist for r in wide)


def _build(tmp, flags, name):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    path = str(tmp / name)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", *flags, "-o", path, os.path.join(ROOT, "tests", "ivf_scan_test.cpp")])
    return path


@pytest.fixture(scope="session")
def ivf_scan_exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ivf_scan")
    return {"plain": _build(tmp, [], "ivf_scan_test"),
            "sanitized": _build(tmp, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "ivf_scan_test_san")}


@pytest.fixture(scope="module")
def cases():
    out = []
    for name in sorted(ir.SHAPES):
        s = ir.shape(name)
        out.append((s, s["xq"][:6], s["probes"][:6], s["k"]))
    for d, M in [(d, 0) for d in DIMS] + [(M * dsub, M) for M, dsub in PQ_FORMS]:
        out.append((ir.obj(d, M), ir.queries(d, len(ir.EDGE_ROWS)), ir.EDGE_ROWS, 64))
    o = ir.obj(4)
    for k in KS:
        out.append((o, ir.queries(4, len(ir.EDGE_ROWS)), ir.EDGE_ROWS, k))
    for nprobe in NPROBES:
        out.append((o, ir.queries(4, 4), ir.probe_rows(4, nprobe), 20))
    return ir.cases_text(out), len(out), sum(c[1].shape[0] for c in out)


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_self_checks(ivf_scan_exes, which):
    out = subprocess.run([ivf_scan_exes[which]], capture_output=True, text=True)
    assert out.returncode == 0 and "ivf scan ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_headers_equal_the_numpy_model_whole_and_cut(ivf_scan_exes, cases, which):
    text, ncases, nq = cases
    assert ncases >= 20
    out = subprocess.run([ivf_scan_exes[which], "cases"], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert f"{ncases} cases, {nq} queries, {5 * nq} runs" in out.stdout and "ivf scan ok" in out.stdout, out.stdout[-2000:]
