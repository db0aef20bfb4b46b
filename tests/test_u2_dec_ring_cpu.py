"""The classified ring traffic of the bitmap chain decoder's step (U2_DEC_STEP bit 2 in csrc/roc_u2.h, restated in
csrc/u2_dec_ring_ref.h) against the pops followed by the index push of codec.cpp, built with g++ (no HIP, no GPU); and the Python
port tests/roc_dec_ring_ref.py against that program."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roc_dec_ring_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    path = str(tmp_path_factory.mktemp("u2_dec_ring") / "u2_dec_ring_test")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-o", path, os.path.join(ROOT, "tests", "u2_dec_ring_test.cpp")])
    return path


def test_u2_dec_ring_forms_agree(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0 and "u2 dec ring ok" in out.stdout, out.stdout + out.stderr


def test_python_port_equals_the_header(exe):
    rng = np.random.default_rng(9)
    rows = []
    for P in range(1, 21):
        p1, p0 = ref.pop_widths(P)
        sh = p1 + p0
        for nmax in (1, 2, 3, 255, 256, 4100, 65535, 65536, int(rng.integers(1, 65537))):
            lq = ref.ring_lq(nmax)
            thr = [ref.L, 1 << (31 + p1), 1 << (31 + sh), lq << sh, (lq << 32) << sh]
            heads = [t + d for t in thr for d in (-1, 0, 1)] + [(1 << 63) - 1, (1 << 64) - 1]
            heads += [max(int(h) >> int(s), 0) | ref.L for h, s in zip(rng.integers(0, 1 << 63, 40, dtype=np.uint64) * 2 + 1, rng.integers(0, 33, 40))]
            for h in heads:
                if ref.L <= h < 1 << 64:
                    rows.append((h, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)), nmax, P))
    assert len(rows) > 9000
    text = "".join("%d %d %d %d %d\n" % r for r in rows)
    out = subprocess.run([exe, "eval", str(len(rows))], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")[:len(rows)]
    seen = set()
    for (h, w, w2, nmax, P), line in zip(rows, lines):
        v = [int(t) for t in line.split()]
        p1, p0 = ref.pop_widths(P)
        lq = ref.ring_lq(nmax)
        ra, rb = [0] * 64, [0] * 64
        ra[39] = rb[39] = w
        ra[38] = rb[38] = w2
        assert tuple(v[0:8]) == ref.dec_ring_ref(h, 40, ra, lq, p1, p0), (h, w, w2, nmax, P)
        assert tuple(v[8:16]) == ref.dec_ring_cls(h, 40, rb, w, lq, p1, p0), (h, w, w2, nmax, P)
        assert v[0:5] == v[8:13]
        seen.add(v[8])
    assert seen == {ref.QUIET, ref.REFILL, ref.SPILL, ref.SIDE}


def test_classes_of_the_headline_list(oracle):
    """S1's longest list (52 114 ids, precision 20) through the model: every step's id is the oracle's, the decode ends in the
    initial state, and the class counts are the ones DESIGN section 5 quotes."""
    from vector_db_id_compression_amd import synth

    off, ids = synth.make_lists_numpy(1_000_000, 1024, 0.75, seed=42)
    sizes = (off[1:] - off[:-1]).astype(np.int64)
    l = int(np.argmax(sizes))
    li = ids[int(off[l]):int(off[l + 1])]
    P = oracle.list_precision(li)
    assert (li.size, P) == (52114, 20)
    e = oracle.roc_encode(li, P)
    want = oracle.roc_decode(e["head"], e["words"], li.size, P, e["mt_draws"])[0]
    m = ref.classify_decode(e["head"], e["words"], li.size, P, want_ids=want, mt_draws=e["mt_draws"], mt_table=oracle.mt_table(1024))
    print("quiet / refill only / spill only / side of the %d steps: %s; exits through head < 2^31: %d"
          % (li.size, m["counts"], int(m["generic_after"].sum())))
    assert m["end_head"] == ref.L and m["end_words"] == m["mt_draws"] - e["mt_draws"]  # (what a pop drew below the empty stack and a spill put back: the kernel's end test)
    assert m["counts"] == [19533 + 23180, 2903, 0, 6498]


@pytest.mark.parametrize("bits", [6, 7, 8, 9, 10])  # (4161 ids are far enough above 2^bits for the ring to regrow)
def test_the_first_step_behind_a_generic_step_is_quiet(oracle, bits):
    """Multiset streams (4161 ids below 2^bits) stepped with the rank the kernel's counters and bitmap give, and the kernel's way
    through them (kernel_walk: ring glue, generic steps, the control of the eight-copy loop).  The loop is entered again right behind
    generic steps -- the ring regrows to 18 words, or a stretch of generic steps at 54 .. 56 words ends in a ring spill -- and the
    first step there is never loud: "refill only" needs nmax < 2^P and "spill only" nmax > 2^P, so a ring only shrinks up to step
    2^P and only grows behind it; a generic stretch inside the list therefore ends with a "spill only" step, and behind one
    H >= lq makes the next step quiet.  tests/test_gpu_roc_dec_ring_class.py says the same of the lists it decodes."""
    rng = np.random.default_rng(bits)
    li = np.sort(np.concatenate([rng.integers(0, 1 << bits, 4160), [(1 << bits) - 1]])).astype(np.uint64)
    P = oracle.list_precision(li)
    e = oracle.roc_encode(li, P)
    mt = oracle.mt_table(1024)
    for rank in ("set", "bitmap"):
        m = ref.classify_decode(e["head"], e["words"], li.size, P, mt_draws=e["mt_draws"], mt_table=mt, rank=rank)
        w = ref.kernel_walk(m, li.size, e["words"].size)
        cls = m["cls"]
        refill, spill = np.flatnonzero((cls == ref.REFILL) | (cls == ref.SIDE)), np.flatnonzero(cls == ref.SPILL)
        assert refill.size and spill.size and refill.max() < (1 << P) <= spill.min()  # nmax = step + 1
        bg = np.flatnonzero(w["behind_generic"])
        print(f"bits {bits}, rank '{rank}': classes {m['counts']}, {int((w['path'] == 1).sum())} steps in the loop, entries behind generic steps at {bg.tolist()}")
        assert bg.size >= 1
        assert (cls[bg] == ref.QUIET).all() and (cls[bg - 1] == ref.SPILL).all()
