"""GPU: the level-2 counter rows of the bitmap chain decoder k_roc_decode_u2<18> / <20>, which live in LDS in front of the bitmap
(csrc/roc_u2.h: u32 row[64][64], read by a broadcast ds_read_b32 and updated by a ds_add_u32 of all lanes; U2Geom::DEC_ROWS_BYTES).

The method is that of test_gpu_roc_u2_decode.py (its _check): the library's streams equal the oracle's, decode_all equals the
oracle's decode of those streams element by element, and both also hold under VIDC_FORCE_GENERAL=1.  Every case is one list with a
100-id list beside it, run in the three id ranges of that file (P20 / P19: four words per entry, 256 ids; G1: one word, 64 ids),
anchored at the top id of the range where the list does not reach it by itself.

What the lists aim at (an entry is dword L1 * 64 + L2 of the counters in REVERSED order: the lowest ids are row 63, element 63):
* full_l1_row: every id of one level-1 row (16 384 ids, 4096 with one word per entry and a random fill from other rows), one id in
  the row above and one in the row below.  Element 0 of that row counts up to 63 entries' worth of ids (63 x 256): a counter
  narrower than that wraps, and an add that leaks into the neighbouring row changes the rank of the two outside ids.
* corners: ids in the first and the last entry of the first and the last level-1 row of the range, i.e. row[63][63], row[63][0],
  row[0][63] and row[0][0] in the ranges that reach the top (row[63][63] at byte 16 380 is the last dword before the bitmap, whose
  first word holds the ids of row[0][0]'s entry): an address that is off by one corrupts the bitmap and shows as a wrong rank or as a
  list handed to the round-1 body.
* same_row_steps: two adjacent entries filled completely among random ids: runs of steps that add to and read from one row.
* multiset: one id twice, so the kernel decodes the list again with the round-1 body over LDS whose front holds counters.
* n4161: random, 65 blocks and one step: the generic step and the asm step alternate on the same rows."""
import numpy as np
import pytest

from test_gpu_roc_u2_decode import RANGES, _anchored, _check, _duplicate, _rand

pytestmark = pytest.mark.gpu


def _fill(li, seed, n, hi):
    """li topped up with random ids below hi to n ids at least"""
    li = np.unique(np.asarray(li, dtype=np.uint64))
    return np.union1d(li, _rand(seed, max(n - li.size, 1) + 64, hi)) if li.size < n else li


def _list(kind, rng_name):
    hi, need, epe = RANGES[rng_name]
    row = 64 * epe  # ids of a level-1 row
    nrows = hi // row
    if kind == "full_l1_row":
        r = nrows * 3 // 4
        li = np.concatenate([[(r - 1) * row + 5], np.arange(r * row, (r + 1) * row), [(r + 1) * row + row - 7]]).astype(np.uint64)
        li = _fill(li, 51, 4200, hi)
        assert np.count_nonzero((li >= r * row) & (li < (r + 1) * row)) == row
    elif kind == "corners":
        ent = [0, 63, (nrows - 1) * 64, nrows * 64 - 1]  # first / last entry of the first / last level-1 row, in id order
        li = np.concatenate([[e * epe, e * epe + 1, e * epe + epe // 2, (e + 1) * epe - 1] for e in ent]).astype(np.uint64)
        li = _fill(li, 52, 4097, hi)
        assert li[0] == 0 and li[-1] == hi - 1
    elif kind == "same_row_steps":
        e0 = (hi * 5 // 8) // epe
        li = _fill(np.arange(e0 * epe, (e0 + 2) * epe, dtype=np.uint64), 53, 4200, hi)
    elif kind == "n4161":
        li = _rand(54, 4161, hi)
    else:
        raise KeyError(kind)
    return _anchored(li, rng_name)


KINDS = ("full_l1_row", "corners", "same_row_steps", "n4161")


@pytest.mark.parametrize("rng_name", list(RANGES))
@pytest.mark.parametrize("kind", KINDS)
def test_lds_counter_rows_decode_equals_oracle_and_general_kernels(roc, oracle, monkeypatch, kind, rng_name):
    hi, need, _ = RANGES[rng_name]
    li = _list(kind, rng_name)
    assert li.size <= 17000
    P = {"P20": 20, "P19": 19}.get(rng_name)
    if P is None:
        assert int(li.max()) < 1 << 18
    _check(roc, oracle, monkeypatch, [li, _rand(7, 100, hi)], P)


@pytest.mark.parametrize("rng_name", list(RANGES))
def test_multiset_falls_back_over_lds_that_holds_counters(roc, oracle, monkeypatch, rng_name):
    hi, need, _ = RANGES[rng_name]
    li = _duplicate(55, 4100, hi)
    assert np.unique(li).size == li.size - 1 and need <= int(li.max()) < hi
    _check(roc, oracle, monkeypatch, [li, _rand(7, 100, hi)])


@pytest.fixture(scope="module")
def roc():
    from vector_db_id_compression_amd.codecs import RocLists

    return RocLists
