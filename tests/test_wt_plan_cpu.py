"""The deciding half of the wavelet tree's host calls (csrc/wt_plan.h): geometry, shape verdict, build / decode / import plans, sizes
and the host checks of an image, built with g++ (no HIP, no GPU); and the tie between that header, which the library runs, and the
numpy models the GPU files compare the library with (wt_ref.py, image_ref.py): the same level count, image word counts, RRR
geometry and sizes on a grid of shapes, and the models' images through wt_image_check, clean and after one-bit corruptions."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import image_ref as ir
import wt_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLISTS = (1, 2, 3, 4, 5, 255, 256, 257, 65537)
NTOTALS = (0, 1, 63, 64, 65, 511, 512, 513, 2015, 2016, 2017, 16383, 16384, 16385)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    path = str(tmp_path_factory.mktemp("wt_plan") / "wt_plan_test")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-o", path, os.path.join(ROOT, "tests", "wt_plan_test.cpp")])
    return path


@pytest.fixture(scope="module")
def shapes():
    """(nlist, ntotal) -> (offsets, level bit vectors, plain image, class words, off_bits) of random symbols, computed once"""
    rng = np.random.default_rng(20260)
    out = {}
    for nlist in NLISTS:
        for nt in NTOTALS:
            sym = rng.integers(0, nlist, nt)
            lv = wr.levels(sym, nlist)
            cls, off_bits = ir.wt_rrr_classes(lv, nlist)
            out[(nlist, nt)] = (wr.lists(sym, nlist)[0], lv, ir.wt_plain_image(lv, nlist), cls, off_bits)
    return out


def test_wt_plan(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "wt plan ok" in out.stdout, out.stdout + out.stderr


def test_geometry_and_sizes_are_the_models(exe, shapes):
    """the header's L, image word counts, nblk / nsamp and both sizes are wt_ref.n_levels, image_ref.words_per_level,
    image_ref.rrr_geometry, the sizes of image_ref's images (off_bits fed in) and wt_ref.plain_size / rrr_size"""
    lines, want = [], []
    for (nlist, nt), (_, lv, plain, cls, off_bits) in shapes.items():
        L = wr.n_levels(nlist)
        assert len(lv) == L and off_bits.size == L
        nblk, nsamp = ir.rrr_geometry(nt)
        lines.append(f"{nlist} {nt} {L} " + " ".join(str(int(b)) for b in off_bits))
        want.append((L, ir.words_per_level(nt), nblk, nsamp, plain.size, cls.size, sum((int(b) + 63) // 64 for b in off_bits),
                     wr.plain_size(lv, nlist), wr.rrr_size(lv, nlist)))
    out = subprocess.run([exe, "query"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = [tuple(int(x) for x in ln.split()) for ln in out.stdout.splitlines()]
    assert len(got) == len(want) == len(NLISTS) * len(NTOTALS)
    for key, g, w in zip(shapes, got, want):
        assert g == w, (key, g, w)


def _record(wt_type, offsets, bits=(), cls=(), offs=(), off_bits=()):
    def arr(a):
        return f"{len(a)} " + " ".join(str(int(x)) for x in a)
    return f"{wt_type} {len(offsets) - 1} " + " ".join(str(int(x)) for x in offsets) + f" {arr(bits)} {arr(cls)} {arr(offs)} {arr(off_bits)}"


def _set_bit(a, word, bit):
    a = np.array(a, copy=True)
    a[word] |= a.dtype.type(1) << a.dtype.type(bit)
    return a


def test_models_pass_the_image_check(exe, shapes):
    """image_ref's images are accepted by wt_image_check as they are (the offset streams, which image_ref does not model, as zero
    words of the length off_bits demands), and refused with the right kind after the smallest corruption of each rule"""
    recs, want = [], []

    def case(key, expect, rec):
        recs.append(rec)
        want.append((key, expect))

    for (nlist, nt), (off, _, plain, cls, off_bits) in shapes.items():
        L, W = wr.n_levels(nlist), ir.words_per_level(nt)
        nblk, nsamp = ir.rrr_geometry(nt)
        ow = [(int(b) + 63) // 64 for b in off_bits]
        offs = np.zeros(sum(ow), dtype=np.uint64)
        key = (nlist, nt)
        case(key, "ok 0 0 0", _record(0, off, bits=plain))
        case(key, "ok 0 0 0", _record(1, off, cls=cls, offs=offs, off_bits=off_bits))
        if nlist > 257:
            continue  # (the corruptions below do not depend on the list count: not on the 65 538-entry records)
        # offsets
        bad = np.array(off, copy=True)
        if nlist >= 2:
            bad[nlist - 1] = bad[nlist] + np.uint64(1)
            case(key, f"offsets_order 0 {nlist - 1} 0", _record(0, bad, bits=plain))
        else:
            bad[0] = 1
            case(key, "offsets_start 0 1 0", _record(0, bad, bits=plain))
        # wt_type 0: sizes off by one, one bit behind ntotal
        case(key, f"n_bits 0 {plain.size + 1} {L * W}", _record(0, off, bits=np.append(plain, np.uint64(0))))
        if plain.size:
            case(key, f"n_bits 0 {plain.size - 1} {L * W}", _record(0, off, bits=plain[:-1]))
        if nt % 64:
            case(key, f"bits_stray {L - 1} 0 0", _record(0, off, bits=_set_bit(plain, L * W - 1, nt % 64)))
        # wt_type 1
        case(key, f"n_cls 0 {cls.size + 1} {L * 6 * nsamp}", _record(1, off, cls=np.append(cls, np.uint32(0)), offs=offs, off_bits=off_bits))
        if cls.size:
            case(key, f"n_cls 0 {cls.size - 1} {L * 6 * nsamp}", _record(1, off, cls=cls[:-1], offs=offs, off_bits=off_bits))
        case(key, f"n_offs 0 {offs.size + 1} {offs.size}", _record(1, off, cls=cls, offs=np.append(offs, np.uint64(0)), off_bits=off_bits))
        if offs.size:
            case(key, f"n_offs 0 {offs.size - 1} {offs.size}", _record(1, off, cls=cls, offs=offs[:-1], off_bits=off_bits))
        over = np.array(off_bits, copy=True)
        over[L - 1] = 61 * nblk + 1
        case(key, f"off_bits_max {L - 1} {61 * nblk + 1} {61 * nblk}", _record(1, off, cls=cls, offs=offs, off_bits=over))
        if nblk < 32 * nsamp:  # the field of block nblk of the last level
            bp = 6 * nblk
            case(key, f"cls_stray {L - 1} {nblk} 0", _record(1, off, cls=_set_bit(cls, (L - 1) * 6 * nsamp + bp // 32, bp % 32), offs=offs, off_bits=off_bits))
        partial = [l for l in range(L) if int(off_bits[l]) % 64]
        if partial:  # the first bit behind off_bits of the last level that has one
            l = partial[-1]
            case(key, f"offs_stray {l} 0 0", _record(1, off, cls=cls, offs=_set_bit(offs, sum(ow[: l + 1]) - 1, int(off_bits[l]) % 64), off_bits=off_bits))
    out = subprocess.run([exe, "check"], input="\n".join(recs) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(want)
    for (key, expect), line in zip(want, got):
        assert line == expect, (key, line, expect)
    kinds = {w.split()[0] for _, w in want}
    assert kinds == {"ok", "offsets_start", "offsets_order", "n_bits", "bits_stray", "n_cls", "n_offs", "off_bits_max", "cls_stray", "offs_stray"}
