"""CPU: csrc/roc_seg_plan.h -- k / shift / segment counts, the multisplit's chunk table and count-table layout, the expansion of a
decode_lists request, the fix-up chunks and the checks of an imported map -- built with g++ as a stand-alone program
(tests/roc_seg_plan_test.cpp) and compared with the numpy model (tests/roc_seg_ref.py) on random cases and on the edges: n = T, T + 1,
k capped at B, S = 1024 and 1025 (refused).  Once more under -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import roc_seg_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fix_chunks(starts_counts_bases):
    out = []
    for start, count, base in starts_counts_bases:
        if base:
            out += [(start + c, min(sr.CHUNK, count - c), base) for c in range(0, count, sr.CHUNK)]
    return out


def plan_case(T, B, sizes):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    head = ["PLAN", T, B, len(sizes), *sizes]
    try:
        k, shift, seg_first = sr.plan(off, T, B)
    except ValueError:
        return head + [1]
    chunks, tbl = sr.chunk_table(off, T, B)
    nseg = 1 << k
    return head + [0, *k, *shift, *seg_first, *tbl, int(nseg[nseg > 1].sum()), len(chunks), *[v for c in chunks for v in c]]


def req_case(rng, T, B, sizes, req):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    k, shift, seg_first = sr.plan(off, T, B)
    inner_sizes = np.concatenate([rng.multinomial(n, np.full(1 << kk, 1.0 / (1 << kk))) for n, kk in zip(sizes, k)] + [np.zeros(0, np.int64)])
    inner_off = np.concatenate([[0], np.cumsum(inner_sizes)])
    model = dict(seg_first=seg_first)
    inner, _ = sr.expand_request(model, req)
    out_off, fix, at = [0], [], 0
    for l in req:
        for i in range(int(seg_first[l]), int(seg_first[l + 1])):
            fix.append((at, int(inner_sizes[i]), (i - int(seg_first[l])) << int(shift[l])))
            at += int(inner_sizes[i])
        out_off.append(at)
    fix = fix_chunks(fix)
    fix_all = fix_chunks([(int(inner_off[i]), int(inner_sizes[i]), (i - int(seg_first[l])) << int(shift[l]))
                          for l in range(len(sizes)) for i in range(int(seg_first[l]), int(seg_first[l + 1]))])
    flat = lambda rows: [v for r in rows for v in r]
    return ["REQ", T, B, len(sizes), *sizes, *inner_sizes, len(req), *req, inner.size, *inner, *out_off, len(fix), *flat(fix),
            len(fix_all), *flat(fix_all)]


def map_case(seg_first, shift, B, prec, want):
    return ["MAP", len(shift), *seg_first, *shift, B, len(prec), *prec, want]


@pytest.fixture(scope="module")
def cases_file(tmp_path_factory):
    rng = np.random.default_rng(33)
    cases = []
    # the edges: n = T, T + 1; k capped at B; S = 1024 (taken) and 1025 -> 2048 (refused); empty lists; no list at all
    for T in (16, 64, 1024):
        cases.append(plan_case(T, 20, [T, T + 1, 2 * T, 2 * T + 1, 0, 1]))
    cases.append(plan_case(16, 3, [1000, 16, 17]))
    cases.append(plan_case(16, 20, [16 * 1024]))
    cases.append(plan_case(16, 20, [5, 16 * 1024 + 1]))
    cases.append(plan_case(16, 10, [16 * 1024 + 1]))  # (k capped at B = 10: S = 1024 is taken)
    cases.append(plan_case(2048, 20, []))
    cases.append(plan_case(1024, 20, [1023, 1024, 1025, 2049, 20000]))
    for _ in range(40):
        T = int(2 ** rng.integers(4, 12))
        B = int(rng.integers(1, 25))
        sizes = [int(v) for v in rng.integers(0, 40 * T, int(rng.integers(0, 9)))]
        sizes = [n if n <= T * 1024 else T for n in sizes]
        cases.append(plan_case(T, B, sizes))
        if sizes and plan_case(T, B, sizes)[4 + len(sizes)] == 0:
            cases.append(req_case(rng, T, B, sizes, [int(v) for v in rng.integers(0, len(sizes), int(rng.integers(0, 7)))]))
    cases.append(req_case(rng, 1024, 20, [3000, 0, 20000, 5], [2, 2, 0, 1, 3]))
    # maps: a good one, then every check
    good = ([0, 1, 5, 6], [10, 8, 10], 10, [10, 8, 0, 7, 8, 3])
    cases.append(map_case(*good, 0))
    cases.append(map_case([0, 1, 5, 7], good[1], 10, good[3], 4))          # does not end at the inner list count
    cases.append(map_case([1, 1, 5, 6], good[1], 10, good[3], 4))          # does not start at 0
    cases.append(map_case([0, 1, 1, 6], good[1], 10, good[3], 2))          # not increasing (a list without a segment)
    cases.append(map_case([0, 1, 4, 6], [10, 8, 9], 10, good[3], 2))       # 3 segments
    cases.append(map_case(good[0], [10, 7, 10], 10, good[3], 2))           # 4 segments but shift says 8
    cases.append(map_case(good[0], [10, 11, 10], 10, good[3], 2))          # shift > B
    cases.append(map_case(good[0], good[1], 10, [10, 8, 9, 7, 8, 3], 2))   # an inner precision above its shift
    cases.append(map_case([0, 2048], [0], 11, [0] * 2048, 1))              # 2048 segments
    cases.append(map_case([0, 9, 5, 6], good[1], 10, good[3], 1))          # past the inner object
    cases.append(map_case([0], [], 10, [], 0))
    path = tmp_path_factory.mktemp("rocseg") / "cases.txt"
    path.write_text("\n".join(" ".join(str(int(v)) if not isinstance(v, str) else v for v in c) for c in cases) + "\n")
    return str(path), len(cases)


def test_the_edges_are_what_they_claim():
    assert plan_case(16, 20, [16 * 1024])[4 + 1] == 0 and plan_case(16, 20, [5, 16 * 1024 + 1])[4 + 2] == 1
    assert plan_case(16, 10, [16 * 1024 + 1])[4 + 1] == 0
    k, shift, seg_first = sr.plan(np.array([0, 16, 33], np.uint64), 16, 20)
    assert k.tolist() == [0, 1] and shift.tolist() == [20, 19] and seg_first.tolist() == [0, 1, 3]
    k, shift, _ = sr.plan(np.array([0, 1000], np.uint64), 16, 3)
    assert k.tolist() == [3] and shift.tolist() == [0]


@pytest.mark.parametrize("sanitize", [False, True])
def test_roc_seg_plan_program(tmp_path, cases_file, sanitize):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    path, ncases = cases_file
    exe = str(tmp_path / "roc_seg_plan_test")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    if sanitize:  # a stand-alone host program: the sanitizer runtimes are linked into it
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([gxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "roc_seg_plan_test.cpp")])
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0 and f"roc seg plan ok: {ncases} cases" in out.stdout, out.stdout + out.stderr
