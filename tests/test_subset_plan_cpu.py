"""CPU: the host-side decisions of a subset (csrc/subset_plan.h: the refusals, the [i1, i2) formulas, the ROC list classes, the ID_MOD
arithmetic, the read-back sizes) built with g++ into a stand-alone program with its own main and held to the numpy model
(subset_ref.py) on generated cases, plain and under -fsanitize=address,undefined.  The header is never loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import subset_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 2 ** 64 - 1


def _cases():
    rng = np.random.default_rng(91)
    cases = []
    # refusals
    for any_null in (0, 1):
        for t in (-1, 0, 1, 2, 3, 4, 5, 77):
            for a1, a2, T in ((0, 0, 0), (1, 0, 10), (3, 3, 10), (3, 2, 10), (0, 10, 10), (4, 3, 10), (3, 11, 10), (2 ** 32, 0, 10),
                              (2 ** 32 - 1, 2 ** 32 - 2, 10), (BIG, BIG - 1, 0), (BIG, BIG, 2 ** 32 - 2), (0, 1, 0), (7, 2, 10)):
                cases.append(["REFUSE", any_null, t, a1, a2, T, sr.refusal(bool(any_null), t, a1, a2, T)])
    # bounds: the i1 > i2 example, then random offsets at every list, also at the largest T
    objs = [np.array([0, 3, 4, 10], np.uint64)]
    for _ in range(30):
        nlist = int(rng.integers(1, 7))
        objs.append(np.concatenate([[0], np.cumsum(rng.integers(0, 2000, nlist) * (rng.random(nlist) < 0.8))]).astype(np.uint64))
    objs.append(np.array([0, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 2], np.uint64))
    for off in objs:
        T = int(off[-1])
        if not T:
            continue
        picks = [(3, 4), (0, T), (T, T), (0, 0)] + [tuple(sorted(int(x) for x in rng.integers(0, T + 1, 2))) for _ in range(4)]
        for a1, a2 in picks:
            i1, i2 = sr.bounds(sr.ELEMENT_RANGE, a1, a2, off)
            for l in range(off.size - 1):
                cases.append(["BOUNDS", 2, a1, a2, T, l, int(off[l]), int(off[l + 1]), int(i1[l]), int(i2[l])])
        for a1 in (1, 2, 3, 7, 2000, 2 ** 32 - 1):
            for a2 in {0, a1 - 1, a1 // 2}:
                i1, i2 = sr.bounds(sr.INVLIST_FRACTION, a1, a2, off)
                for l in range(off.size - 1):
                    cases.append(["BOUNDS", 3, a1, a2, T, l, int(off[l]), int(off[l + 1]), int(i1[l]), int(i2[l])])
        for a1, a2 in ((0, 2), (1, 1), (2, 0), (0, BIG), (off.size - 2, off.size + 5)):
            i1, i2 = sr.bounds(sr.INVLIST, a1, a2, off)
            for l in range(off.size - 1):
                cases.append(["BOUNDS", 4, a1, a2, T, l, int(off[l]), int(off[l + 1]), int(i1[l]), int(i2[l])])
    # classes
    for n, n_new in ((0, 0), (1, 1), (1, 0), (5, 5), (5, 0), (5, 4), (2 ** 32 - 2, 1)):
        cases.append(["CLASS", n, n_new, sr.roc_class(n, n_new)])
    # ID_MOD
    mods = [1, 2, 3, 5, 8, 1000, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 10 ** 12 + 39, 2 ** 63, 2 ** 63 + 1, BIG]
    ids = [0, 1, 7, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 40 + 3, 2 ** 63, 2 ** 63 + 7, BIG] + [int(x) for x in rng.integers(0, 2 ** 63, 20)] \
        + [int(x) << 1 | 1 for x in rng.integers(2 ** 62, 2 ** 63, 10)]
    for a1 in mods + [int(x) for x in rng.integers(1, 2 ** 32, 10)]:
        cases.append(["MODKIND", a1, sr.mod_kind(a1)])
        for x in ids:
            cases.append(["MOD", x, a1, x % a1])
            cases.append(["TAKES", 1, a1, x % a1, x, 1])
            cases.append(["TAKES", 1, a1, (x + 1) % a1, x, int(a1 == 1)])
    for a1, a2 in ((0, 0), (0, 1), (5, 2 ** 32), (2 ** 32, 2 ** 63), (2 ** 63, BIG), (0, BIG), (9, 3)):
        for x in ids:
            cases.append(["TAKES", 0, a1, a2, x, int(a1 <= x < a2)])
    # read-back sizes
    for roc in (0, 1):
        for t in range(5):
            for nlist, T, cand, re in ((0, 0, 0, 0), (5, 0, 0, 0), (5, 100, 4, 0), (5, 100, 4, 3), (9000, 10 ** 6, 8000, 8000)):
                cases.append(["BACK", roc, t, nlist, T, cand, re, sr.readback_bytes(bool(roc), t, nlist, T, cand, re)])
    return cases


@pytest.mark.parametrize("sanitize", [False, True])
def test_subset_plan_program(tmp_path, sanitize):
    """the refusals, the range formulas, the classes and the ID_MOD arithmetic the library runs (csrc/subset_plan.h) are the model's"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    cases = _cases()
    kinds = {(c[0], c[-1]) for c in cases}
    assert {("REFUSE", r) for r in (sr.OK, sr.ERR_NULL, sr.ERR_TYPE, sr.ERR_ARGS)} <= kinds
    assert {("CLASS", c) for c in (sr.KEEP, sr.EMPTY, sr.PARTIAL)} <= kinds
    assert {("MODKIND", k) for k in (sr.MOD_MASK, sr.MOD_U32, sr.MOD_U64)} <= kinds
    assert ["BOUNDS", 2, 3, 4, 10, 1, 3, 4, 1, 1] in cases  # the i1 > i2 example, clamped to the empty range
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(" ".join(str(v) for v in c) for c in cases) + "\n")
    exe = str(tmp_path / "subset_plan_test")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    if sanitize:  # a stand-alone host program: the sanitizer runtimes are linked into it
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([gxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "subset_plan_test.cpp")])
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0 and f"subset plan ok: {len(cases)} cases" in out.stdout, out.stdout + out.stderr
