"""GPU: packed-bits IVF lists of explicit widths on value patterns that show a stray bit across a field boundary -- every byte of every
list against the numpy model tests/lists_ref.py (packed_list; equal to the CPU oracle, tests/test_lists_ref_cpu.py), every position
through every random-access entry point, from host and from device offsets, before and after save -> load.

An object of width `bits` holds, for every pattern of lists_ref.PACKED_PATTERNS (all-ones fields next to all-zero fields, alternating
0x55.. / 0xAA.., a single one walking through the field) and for uniform values, one list of every size in lists_ref.PACKED_SIZES
(0, one id, 63 / 64 / 65, one 512-id chunk and its neighbours, 1025, 4097).  At 64 bits the all-ones field is the id 2^64 - 1, which the
encoder's domain check used to refuse."""
import numpy as np
import pytest

import lists_ref as lr

pytestmark = pytest.mark.gpu

BITS = (1, 13, 31, 32, 33, 63, 64)
CASES = [(b, r) for b in BITS for r in ("host", "dev")]
_DATA, _OBJ = {}, {}  # filled on demand (any test order), emptied when the file is done


@pytest.fixture(scope="module", autouse=True)
def _release_objects():
    yield
    _OBJ.clear()
    _DATA.clear()


class Data:
    def __init__(self, bits):
        rng = np.random.default_rng(bits)
        mask = np.uint64((1 << bits) - 1)
        self.bits = bits
        self.lists = [lr.packed_patterns(n, bits, kind) for kind in lr.PACKED_PATTERNS for n in lr.PACKED_SIZES]
        self.lists += [rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1) & mask for n in lr.PACKED_SIZES]
        self.sizes = np.array([li.size for li in self.lists], dtype=np.int64)
        self.off = lr.offsets_of(self.lists)
        self.flat = lr.concat(self.lists)
        self.images = [lr.packed_list(li, bits) for li in self.lists]
        self.ql = np.repeat(np.arange(len(self.lists), dtype=np.uint64), self.sizes)
        self.qo = np.arange(self.flat.size, dtype=np.uint64) - np.repeat(self.off[:-1], self.sizes)


def data(bits):
    if bits not in _DATA:
        _DATA[bits] = Data(bits)
    return _DATA[bits]


def obj(bits, route):
    import torch
    from vector_db_id_compression_amd.codecs import PackedLists

    if (bits, route) not in _OBJ:
        d = data(bits)
        ids = torch.from_numpy(d.flat.view(np.int64)).cuda()
        off = torch.from_numpy(d.off.view(np.int64)).cuda() if route == "dev" else d.off
        _OBJ[bits, route] = PackedLists.encode(off, ids, bits=bits)
    return _OBJ[bits, route]


def check_images_and_decode(pk, d, tag):
    assert pk.bits == d.bits and np.array_equal(pk.offsets, d.off), tag
    assert pk.compressed_bytes == sum(img.size for img in d.images), tag
    for l, img in enumerate(d.images):
        assert np.array_equal(pk.export_bytes(l), img), (tag, l)
    assert np.array_equal(pk.decode_all().cpu().numpy().view(np.uint64), d.flat), tag


def check_every_position(pk, d, tag):
    import torch

    want = d.flat.view(np.int64)
    got = pk.get(d.ql, d.qo)
    assert np.array_equal(got, want), (tag, "get", np.flatnonzero(got != want)[:8])
    lab = lr.all_labels(d.sizes, np.random.default_rng(7))
    exp, n_invalid = lr.expect_labels(lab, d.sizes, d.flat)
    invalid = torch.zeros(1, dtype=torch.int64, device="cuda")
    got = pk.translate_labels(torch.from_numpy(lab).cuda(), invalid=invalid).cpu().numpy()
    assert np.array_equal(got, exp), (tag, "translate_labels", np.flatnonzero(got != exp)[:8])
    assert int(invalid.item()) == n_invalid, tag
    ne = np.flatnonzero(d.sizes)
    slot_of = np.zeros(len(d.lists), dtype=np.int64)
    slot_of[ne] = np.arange(ne.size)
    p = np.random.default_rng(8).permutation(want.size)
    got = pk.decode_gather(ne, slot_of[d.ql.astype(np.int64)][p], d.qo[p])
    assert np.array_equal(got, want[p]), (tag, "decode_gather")


@pytest.mark.parametrize("bits,route", CASES)
def test_byte_images_and_decode_all(bits, route):
    check_images_and_decode(obj(bits, route), data(bits), (bits, route))


@pytest.mark.parametrize("bits,route", CASES)
def test_get_translate_labels_and_decode_gather_at_every_position(bits, route):
    check_every_position(obj(bits, route), data(bits), (bits, route))


@pytest.mark.parametrize("bits,route", CASES)
def test_loaded_object_answers_like_the_model(bits, route, tmp_path):
    from vector_db_id_compression_amd.codecs import PackedLists

    obj(bits, route).save(tmp_path / "pk.npz")
    pk = PackedLists.load(tmp_path / "pk.npz")
    check_images_and_decode(pk, data(bits), (bits, route, "loaded"))
    check_every_position(pk, data(bits), (bits, route, "loaded"))
