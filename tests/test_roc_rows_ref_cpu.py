"""tests/roc_rows_ref.py (the member-row geometry of the ROC decoders in numpy, the id families on the capacity edge) against the C++
headers and the oracle: no GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import roc_rows_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = rr.gpu_cases()


def test_geometry_equals_the_headers(tmp_path):
    """geometry and b2l_buckets against roc_sizing.h / roc_dec_plan.h, built with g++ like tests/test_roc_dec_plan_cpu.py builds its
    program, on every (n, P, umax, align) of the GPU cases and on the class boundaries."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path / "roc_rows_geom_test")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "roc_rows_geom_test.cpp")])
    table = rr.geometry_table()
    out = subprocess.run([exe], input="".join("%d %d %d %d\n" % row for row in table), capture_output=True, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines[-1] == "roc rows geometry ok %d" % len(table), out.stdout[-2000:] + out.stderr
    for row, line in zip(table, lines):
        n, P, umax, align = row
        got = tuple(int(v) for v in line.split())
        assert got[:4] == row
        want = (rr.geometry("lane64", n, P, align)[1], rr.geometry("lane128", n, P, align)[1], rr.geometry("lane256", n, P, align)[1],
                *rr.geometry("grp", n, P), *rr.geometry("gen", n, P), rr.b2l_buckets(n, P, umax))
        assert got[4:] == want, (row, got[4:], want)
    assert [rr.geometry(k, 700, 20)[0] for k in rr.KINDS] == [6, 7, 8, 8, 12, 5, 6, 7, 8, 7]
    # the caps the lane cases rely on: n = 700 tells the two alignments apart
    assert [(rr.lane_cap(64, n, 16), rr.lane_cap(64, n, 4)) for n in (65, 513, 700, 1024)] == [(32, 20), (32, 32), (48, 36), (48, 48)]


def test_bucket_counts_of_imported_streams():
    """without maxima the planner assumes half of the buckets: the sizes that keep each bucket count are 30 * (bk / 2 + 1)"""
    for P in (20, 31):
        assert [rr.b2l_buckets(n, P, (1 << P) - 1) for n in (960, 1920, 3840, 4096)] == [32, 64, 128, 256]
        assert [rr.b2l_buckets(n, P, 0) for n in (510, 990, 1950, 3870)] == [32, 64, 128, 256]
        assert [rr.b2l_buckets(n, P, 0) for n in (511, 991, 1951, 3871)] == [64, 128, 256, 0]
    assert rr.b2l_buckets(256, 20, 0) == 0 and rr.b2l_buckets(4097, 20, (1 << 20) - 1) == 0 and rr.b2l_buckets(960, 32, 0) == 0


def _check_family(oracle, ids, n, P, roundtrip=True):
    assert ids.dtype == np.uint64 and ids.size == n
    assert np.all(ids[1:] > ids[:-1])  # ascending, distinct
    assert int(ids[-1]) == (1 << P) - 1 and oracle.list_precision(ids) == P
    if roundtrip:
        e = oracle.roc_encode(ids, P)
        dec = oracle.roc_decode(e["head"], e["words"], n, P, e["mt_draws"])[0]
        assert np.array_equal(np.sort(dec), ids)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_families_of_the_gpu_cases(oracle, case):
    """size, distinct ids, reference precision P, loads.max() == cap (packed) / cap + 1 in the bucket `where` names (one_over), and
    the oracle round-trips every family as a set; three lists of every group of six go one over."""
    lists, tags, geo = rr.case_lists(case)
    lossless = not case.get("beyond_reference")
    for li, tag, (kind, n, P, align) in zip(lists, tags, geo):
        bits, cap = rr.geometry(kind, n, P, align)
        assert (1 << (P - bits)) >= cap + 2  # a bucket is wide enough for cap + 1 members and another id
        _check_family(oracle, li, n, P, roundtrip=lossless)
        ld = rr.loads(li, P, bits)
        assert ld.sum() == n and ld[-1] >= 1
        if tag == "packed":
            assert ld.max() == cap and not rr.handed_back(li, P, bits, cap)
            k = -(-n // cap)
            assert np.count_nonzero(ld) == k and np.count_nonzero(ld == cap) >= k - 1
            assert ld[0] == cap and (k < 3 or ld[-1] == cap) and np.all(ld[1:k - 1] > 0)  # bucket 0, the top bucket, a run from 1 upward
        elif tag == "random":  # (the general decoder's rows of 16 spill on random ids too: nothing is handed back there)
            assert kind == "gen" or not rr.handed_back(li, P, bits, cap)
        else:
            b = rr.over_bucket(tag, bits)
            assert ld.max() == cap + 1 and ld[b] == cap + 1 and np.count_nonzero(ld > cap) == 1 and rr.handed_back(li, P, bits, cap)
            if tag == "middle" and rr.middle_is_flanked(n, cap):
                assert ld[b - 1] == cap and ld[b + 1] == cap
    if case["hands_back"]:
        back = rr.model_handed_back(lists, geo)
        assert sum(back) == 3 * len(case["groups"]) and [t in ("top", "middle", "first") for t in tags] == back


def test_the_reference_does_not_round_trip_the_65537_id_families(oracle):
    """Beyond 65 536 ids the reference's codec is lossy: what the decoder sees is not the encoded list, so a `packed` list (fullest
    bucket at cap = 96) decodes to ids of which 97 fall into one bucket.  The GPU test of that size asks the model about the decoded
    ids for this reason."""
    (case,) = [c for c in CASES if c.get("beyond_reference")]
    lists, tags, geo = rr.case_lists(case)
    seen_max = []
    for li, (kind, n, P, align) in zip(lists, geo):
        bits, cap = rr.geometry(kind, n, P, align)
        e = oracle.roc_encode(li, P)
        dec = oracle.roc_decode(e["head"], e["words"], n, P, e["mt_draws"])[0]
        assert not np.array_equal(np.sort(dec), li)
        seen_max.append(int(rr.loads(dec, P, bits).max()))
    assert [int(rr.loads(li, 24, 12).max()) for li in lists[:5]] == [97, 96, 97, 96, 97] and seen_max[:5] == [97] * 5 and seen_max[5] < 96


def test_single_bucket_family(oracle):
    rng = np.random.default_rng(5)
    for n, P in ((300, 24), (300, 31), (4097, 24), (4097, 31)):
        bits, cap = rr.geometry("gen", n, P)
        li = rr.single_bucket(rng, n, P, bits)
        _check_family(oracle, li, n, P)
        ld = rr.loads(li, P, bits)
        assert ld[0] == n - 1 and ld[-1] == 1 and n - 1 - cap > 64  # an overflow list longer than a 64-step block


def test_families_refuse_what_does_not_fit():
    rng = np.random.default_rng(6)
    with pytest.raises(ValueError):
        rr.packed(rng, 64 * 20 + 1, 20, 6, 20)       # more ids than 64 rows of 20 hold
    with pytest.raises(ValueError):
        rr.one_over(rng, 30, 20, 6, 32, "first")      # too few ids to fill a row
    with pytest.raises(ValueError):
        rr.one_over(rng, 4097, 16, 12, 64, "top")     # a bucket of 16 ids cannot take 65 members
    assert rr.loads(rr.packed(rng, 64 * 20, 20, 6, 20), 20, 6).tolist() == [20] * 64  # every row exactly full


def test_packed_lists_collide_inside_decode_blocks(oracle):
    """What the families are for: most steps of a 64-step block of the decoders with members in flight hit a nearly full row, against
    about one collision per block on random ids."""
    rng = np.random.default_rng(7)
    for kind, n, P in (("b2", 4097, 24), ("gen", 4096, 24)):
        bits, cap = rr.geometry(kind, n, P)
        pk = rr.packed(rng, n, P, bits, cap)
        rnd = np.sort(rng.choice(1 << P, size=n, replace=False)).astype(np.uint64)
        pairs = [rr.same_bucket_pairs(oracle.roc_encode(li, P)["order"], P, bits) for li in (pk, rnd)]
        assert pairs[0] > (8 if kind == "b2" else 1.5) * pairs[1], (kind, pairs)
