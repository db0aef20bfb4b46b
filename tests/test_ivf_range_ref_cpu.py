"""CPU: the numpy model of the IVF range search (tests/ivf_range_ref.py) against a brute-force loop written from include/vidc.h, on
the designed objects of the scan tests, for every radius of the list (a candidate's distance, that +- 0.5, 0, -1, +inf, NaN); the
cases hold what they are named for; csrc/ivf_range_ref.h + ivf_range_plan.h built with g++ as a stand-alone program
(tests/ivf_range_test.cpp), plain and with -fsanitize=address,undefined, against cases the model writes out: count and fill as one
piece and as S pieces, and the write bound under short capacities and the slot limits of another radius."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ivf_range_ref as rr
import ivf_scan_ref as ir
from test_ivf_scan_ref_cpu import DIMS, PQ_FORMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = [(d, 0) for d in DIMS] + [(M * dsub, M) for M, dsub in PQ_FORMS]
NPROBES = (1, 2, 3, 16, 64, 65, 1024)


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("slot_lims", "D", "labels")):
        assert rr.same_bits(g, w), f"{what}: {name} differs"


@pytest.mark.parametrize("d,M", FORMS)
def test_model_equals_the_brute_force_on_the_designed_objects(d, M):
    o, xq = ir.obj(d, M), ir.queries(d, len(ir.EDGE_ROWS))
    for radius in rr.radii(d, M):
        assert_same(rr.model(o["offsets"], o["vecs"], xq, ir.EDGE_ROWS, radius), rr.brute_force(o["offsets"], o["vecs"], xq, ir.EDGE_ROWS, radius),
                    (d, M, radius))


def test_model_equals_the_brute_force_on_wide_rows():
    o = ir.obj(4)
    for nprobe in NPROBES:
        rows, xq = ir.probe_rows(3, nprobe), ir.queries(4, 3)
        for radius in (rr.equal_radius(4), float("inf")):
            assert_same(rr.model(o["offsets"], o["vecs"], xq, rows, radius), rr.brute_force(o["offsets"], o["vecs"], xq, rows, radius), (nprobe, radius))


def test_model_rules():
    off = np.array([0, 2, 2, 5], np.uint64)  # lists of 2, 0 and 3 entries
    vecs = np.array([[0], [3], [1], [3], [0]], np.float32)
    probes = np.array([[2, 0, 2, -1], [1, 3, 2 ** 40, -7], [0, 0, 0, 0]], np.int64)
    xq = np.zeros((3, 1), np.float32)
    lims, D, L = rr.model(off, vecs, xq, probes, 9.0)  # 9 itself is excluded
    assert lims.tolist() == [0, 2, 3, 3, 3, 3, 3, 3, 3, 4, 4, 4, 4]
    assert D.tolist() == [1, 0, 0, 0] and L.tolist() == [2 << 32, (2 << 32) | 2, 0, 0]  # probe-row order, then offset: not sorted
    lims, D, L = rr.model(off, vecs, xq, probes, 9.5)
    assert lims[::4].tolist() == [0, 5, 5, 7] and D.tolist() == [1, 9, 0, 0, 9, 0, 9]
    for radius in (0.0, -1.0, float("nan")):
        lims, D, L = rr.model(off, vecs, xq, probes, radius)
        assert not lims.any() and lims.size == 13 and D.size == 0 and L.size == 0
    assert rr.model(off, vecs, xq, probes, np.inf)[0][-1] == 5 + 0 + 2
    # the fill model under other slot limits: a short capacity cuts, smaller limits keep each slot's first hits
    big = rr.model(off, vecs, xq, probes, 9.5)
    small = rr.model(off, vecs, xq, probes, 9.0)
    fD, fL = rr.fill_model(off, vecs, xq, probes, 9.5, small[0], 4)
    assert fD.tolist() == [1, 9, 0, 0] and fL.tolist() == [2 << 32, (2 << 32) | 1, 0, 0]
    fD, fL = rr.fill_model(off, vecs, xq, probes, 9.0, big[0], 7)
    assert rr.same_bits(fD[[0, 1, 3, 5]], small[1]) and all(rr.same_bits(fD[i], rr.POISON_D) for i in (2, 4, 6)) and fL[2] == rr.POISON_L


@pytest.mark.parametrize("d,M", FORMS)
def test_the_cases_hold_what_they_are_named_for(d, M):
    o, xq, rows = ir.obj(d, M), ir.queries(d, len(ir.EDGE_ROWS)), ir.EDGE_ROWS
    nprobe = rows.shape[1]
    eq, lo, hi, zero, neg, inf, nan = rr.radii(d, M)
    assert eq > 0 and (lo, hi) == (eq - 0.5, eq + 0.5) and (zero, neg) == (0, -1) and np.isinf(inf) and np.isnan(nan)
    every = rr.model(o["offsets"], o["vecs"], xq, rows, inf)
    at, below, above = (rr.model(o["offsets"], o["vecs"], xq, rows, r) for r in (eq, lo, hi))
    # a candidate with distance == radius exists, and it is excluded: eq and eq - 0.5 agree, eq + 0.5 adds exactly those candidates
    n_equal = int((every[1] == np.float32(eq)).sum())
    assert n_equal > 0 and not (at[1] == np.float32(eq)).any() and (at[1] < np.float32(eq)).all()
    assert_same(at, below, "eq against eq - 0.5")
    assert int(above[0][-1]) == int(at[0][-1]) + n_equal and 0 < int(at[0][-1]) < int(every[0][-1])
    # distances are exact integers: every comparison is exact
    assert np.array_equal(every[1], np.round(every[1])) and every[1].max() < 2 ** 24
    per_slot = np.diff(every[0].astype(np.int64))
    assert (per_slot > 128).any() and ((per_slot > 64) & (per_slot <= 128)).any()  # slots of several trips
    lists = [rr.slot_lists(r, o["nlist"]) for r in rows]
    assert per_slot.tolist() == [ir.EDGE_SIZES[l] if l >= 0 else 0 for row in lists for l in row]
    # an empty slot between two non-empty ones (a repeated list), invalid probes, an empty list that is probed
    q = [r.tolist() for r in rows].index([5, 5, 6, -1])
    assert per_slot[q * nprobe: q * nprobe + 3].tolist() == [129, 0, 300]
    flat = rows.reshape(-1).tolist()
    assert -1 in flat and o["nlist"] in flat and 2 ** 40 in flat
    valid = [[p for p in r.tolist() if 0 <= p < o["nlist"]] for r in rows]
    assert any(len(v) - len(set(v)) == 1 for v in valid) and any(len(v) - len(set(v)) >= 2 for v in valid)  # named twice, three times
    assert ir.EDGE_SIZES[0] == 0 and any(row[0] == 0 for row in lists)
    # a query with no result at +inf (only invalid probes, or the empty list alone), and calls whose total is 0
    per_query = np.diff(every[0][::nprobe].astype(np.int64))
    assert (per_query == 0).sum() >= 2 and (per_query > 0).any()
    for r in (zero, neg, nan):
        lims, D, L = rr.model(o["offsets"], o["vecs"], xq, rows, r)
        assert lims.size == rows.size + 1 and not lims.any() and D.size == 0 and L.size == 0
    # at the candidate's radius some queries have results and, where d leaves room, the hits end inside a trip
    assert (np.diff(at[0][::nprobe].astype(np.int64)) > 0).any()


def test_wide_rows_name_lists_again_and_again():
    o = ir.obj(4)
    for nprobe in (64, 65, 1024):
        rows = ir.probe_rows(3, nprobe)
        lims = rr.model(o["offsets"], o["vecs"], ir.queries(4, 3), rows, np.inf)[0]
        per_slot = np.diff(lims.astype(np.int64)).reshape(3, nprobe)
        assert (per_slot.sum(1) == o["ntotal"]).all()  # every list once per query, however often it is named
        assert ((per_slot > 0).sum(1) == sum(s > 0 for s in ir.EDGE_SIZES)).all()


def _build(tmp, flags, name):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    path = str(tmp / name)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", *flags, "-o", path, os.path.join(ROOT, "tests", "ivf_range_test.cpp")])
    return path


@pytest.fixture(scope="session")
def ivf_range_exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ivf_range")
    return {"plain": _build(tmp, [], "ivf_range_test"),
            "sanitized": _build(tmp, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "ivf_range_test_san")}


@pytest.fixture(scope="module")
def cases():
    out = []
    for d, M in FORMS:
        o, xq = ir.obj(d, M), ir.queries(d, len(ir.EDGE_ROWS))
        for radius in rr.radii(d, M) if d in (4, 128) else (rr.equal_radius(d, M), float("inf")):
            out.append((o, xq, ir.EDGE_ROWS, radius))
    o = ir.obj(4)
    for nprobe in NPROBES:
        out.append((o, ir.queries(4, 3), ir.probe_rows(3, nprobe), rr.equal_radius(4) + 0.5))
    return rr.cases_text(out), len(out)


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_self_checks(ivf_range_exes, which):
    out = subprocess.run([ivf_range_exes[which]], capture_output=True, text=True)
    assert out.returncode == 0 and "ivf range ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_headers_equal_the_numpy_model_whole_and_cut(ivf_range_exes, cases, which):
    text, ncases = cases
    assert ncases >= 30
    out = subprocess.run([ivf_range_exes[which], "cases"], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert f"{ncases} cases, {5 * ncases} runs, {4 * ncases} bounded fills" in out.stdout and "ivf range ok" in out.stdout, out.stdout[-2000:]
