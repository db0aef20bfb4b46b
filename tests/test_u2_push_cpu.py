"""The classified id push of the dense chain encoder step (U2_ENC_PUSH in csrc/roc_u2.h, restated in csrc/u2_push_ref.h) against the
two slices of codec.cpp, built with g++ (no HIP, no GPU); the Python port tests/roc_push_ref.py against that program; and the
oracle's encode of the headline workload's longest list stepped through the port, which gives the class frequencies of
profiles/r48_roc_encode_push_class.txt."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roc_push_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    path = str(tmp_path_factory.mktemp("u2_push") / "u2_push_test")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-o", path, os.path.join(ROOT, "tests", "u2_push_test.cpp")])
    return path


def test_u2_push_forms_agree(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0 and "u2 push ok" in out.stdout, out.stdout + out.stderr


def test_python_port_equals_the_header(exe):
    rng = np.random.default_rng(6)
    rows = []
    for P in range(1, 21):
        p0, p1 = ref.push_widths(P)
        tA, tB = 1 << (63 - p0), 1 << (63 - p0 - p1)
        qs = [1, ref.L, tB - 1, tB, tB + 1, tA - 1, tA, tA + 1, (1 << 63) - 1]
        qs += [max(int(h) >> int(s), 1) for h, s in zip(rng.integers(0, 1 << 63, 200, dtype=np.uint64), rng.integers(0, 63, 200))]
        rows += [(q, int(x), P) for q, x in zip(qs, rng.integers(0, 1 << P, len(qs), dtype=np.uint64))]
    assert len(rows) > 4000
    text = "".join(f"{q} {x} {P}\n" for q, x, P in rows)
    out = subprocess.run([exe, "eval", str(len(rows))], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")[:len(rows)]
    for (q, x, P), line in zip(rows, lines):
        v = [int(t) for t in line.split()]
        p0, p1 = ref.push_widths(P)
        head2, words2, cls2 = ref.push_two(q, x, p0, p1)
        head1, Bv, mul, words1, cls1 = ref.push_one(q, x, p0, p1)
        assert v[0:4] == [head2, words2[0] if words2 else 0, len(words2), cls2], (q, x, P)
        assert v[4:10] == [head1, Bv, mul, words1[0] if words1 else 0, len(words1), cls1], (q, x, P)
        assert (head1, words1, cls1) == (head2, words2, cls2)


def test_classes_of_the_headline_list(oracle):
    """S1's longest list (52 114 ids, precision 20) through the model: it ends in the oracle's head and words, and the class
    frequencies are the ones DESIGN section 5 quotes."""
    from vector_db_id_compression_amd import synth

    off, ids = synth.make_lists_numpy(1_000_000, 1024, 0.75, seed=42)
    sizes = (off[1:] - off[:-1]).astype(np.int64)
    l = int(np.argmax(sizes))
    li = ids[int(off[l]):int(off[l + 1])]
    P = oracle.list_precision(li)
    assert (li.size, P) == (52114, 20)
    e = oracle.roc_encode(li, P)
    m = ref.classify_encode(e["order"], P, oracle.mt_table(1024))
    assert m["head"] == e["head"] and np.array_equal(m["words"], e["words"]) and m["mt_draws"] == e["mt_draws"]
    n = li.size
    print("classes C / A / B of the %d steps: %s = %s %%; steps in the unrolled loop %d, per copy and class %s; ring spills behind a "
          "class C / A / B step %s; divisor block changes %d"
          % (n, m["classes"], [round(100.0 * c / n, 1) for c in m["classes"]], int((m["copy"] >= 0).sum()), m["by_copy"].tolist(),
             [m["spill_after"].count(k) for k in (0, 1, 2)], m["blocks"]))
    assert sum(m["classes"]) == n
    assert m["classes"][0] > 3 * (m["classes"][1] + m["classes"][2])  # the common path is class C: more than three steps in four
