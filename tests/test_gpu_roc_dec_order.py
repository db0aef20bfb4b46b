"""GPU: the natural entry order of the bitmap chain decoder k_roc_decode_u2<18> / <20> (csrc/roc_u2.h: entry = x >> 8 or x >> 6,
bitmap dword x >> 5, E1 and the level-2 row elements count the ids in blocks and entries BELOW; the encoders keep the reversed order
their search needs, the decoder builds its own structures from empty LDS and nothing else reads them).

Checked the way test_gpu_roc_enc_step.py and test_gpu_roc_u2_decode.py check (check_modes below): the default kernels,
VIDC_U2_DENSE=0 and VIDC_FORCE_GENERAL=1 must be identical to each other and to the oracle in heads, words, nwords, mt_draws,
precision, perm and the decoded ids.  Every case is one
list with a 100-id list beside it, in the three id ranges of test_gpu_roc_u2_decode.RANGES (P20 / P19: four words per entry, 256 ids;
G1: one word, 64 ids), anchored at the top id of the range where the list does not reach it by itself.

What the lists aim at:
* ends: ids 0 .. 63 and the top 64 ids of the range: the first and the last dword of the bitmap, which sit next to the last dword of
  the counter rows and next to the strip; row[0][0] and the last row element of the range.
* full_l1_row: every id of one level-1 row, one id in the row above and one in the row below (test_gpu_roc_dec_rows.py's list): the
  prefix of a row now grows in the lanes ABOVE the entry, and a row that is updated in the wrong direction changes every rank.
* low_dense_high_sparse and its mirror image: 4000 ids in the lowest eighth of the range and 200 in the upper half.  Reversal
  (x -> top - x) is not a symmetry of either list, so a step that is converted in one place only (entry without rank, E1 without
  the rows, insertion without the read) gives a wrong rank on at least one of the two.
* multiset: one id twice: the kernel sees fewer bits than ids and decodes the list again with the round-1 body, over LDS that holds
  natural-order structures.
* n4161: random, 65 blocks and one step: the generic step and the asm step alternate on the same structures."""
import numpy as np
import pytest

from test_gpu_roc_dec_rows import _fill
from test_gpu_roc_dec_rows import _list as _rows_list
from test_gpu_roc_enc_step import MODES, _encode
from test_gpu_roc_u2_decode import RANGES, _anchored, _duplicate, _rand

pytestmark = pytest.mark.gpu

KINDS = ("ends", "full_l1_row", "low_dense_high_sparse", "high_dense_low_sparse", "multiset", "n4161")


def _list(kind, rng_name):
    hi, need, epe = RANGES[rng_name]
    if kind == "ends":
        li = _fill(np.concatenate([np.arange(64), np.arange(hi - 64, hi)]).astype(np.uint64), 61, 4097, hi)
        assert np.array_equal(li[:64], np.arange(64)) and np.array_equal(li[-64:], np.arange(hi - 64, hi))
    elif kind == "full_l1_row":
        return _rows_list(kind, rng_name)
    elif kind in ("low_dense_high_sparse", "high_dense_low_sparse"):
        li = np.concatenate([_rand(62, 4000, hi // 8), _rand(63, 200, hi, hi // 2)])
        if kind == "high_dense_low_sparse":
            li = np.sort(np.uint64(hi - 1) - li)
        assert not np.array_equal(np.sort(np.uint64(hi - 1) - li), li)
    elif kind == "multiset":
        li = _duplicate(64, 4100, hi)
        assert np.unique(li).size == li.size - 1 and need <= int(li.max()) < hi
        return li
    elif kind == "n4161":
        li = _rand(65, 4161, hi)
    else:
        raise KeyError(kind)
    return _anchored(li, rng_name)


def check_modes(roc, oracle, monkeypatch, lists, name, want_perms=(True, False)):
    """default == bitmap body == general kernels == oracle, for every stream field, perm and the decoded ids"""
    off = np.concatenate([[0], np.cumsum([li.size for li in lists])]).astype(np.uint64)
    ids = np.concatenate(lists)
    ref = []  # oracle results, computed once for every setting of want_perm
    for li in lists:
        P = oracle.list_precision(li)
        e = oracle.roc_encode(li, P)
        e["decoded"] = oracle.roc_decode(e["head"], e["words"], li.size, P, e["mt_draws"])[0]
        ref.append((P, e))
    try:
        for want_perm in want_perms:
            got = _encode(roc, monkeypatch, "default", off, ids, want_perm)
            assert not isinstance(got, str), f"{name}: {got}"
            for other in ("bitmap", "general"):
                base = _encode(roc, monkeypatch, other, off, ids, want_perm)
                assert not isinstance(base, str), f"{name} ({other}): {base}"
                for k in base:
                    assert np.array_equal(got[k], base[k]), f"{name} want_perm={want_perm}: '{k}' differs from the {other} kernels"
            woff = np.concatenate([[0], np.cumsum(got["nwords"].astype(np.int64))])
            for l, li in enumerate(lists):
                P, e = ref[l]
                a, b = int(off[l]), int(off[l + 1])
                assert int(got["precision"][l]) == P, f"{name} list {l}: precision"
                assert int(got["heads"][l]) == e["head"], f"{name} list {l}: head"
                assert int(got["nwords"][l]) == e["words"].size, f"{name} list {l}: nwords"
                assert np.array_equal(got["words"][woff[l]:woff[l + 1]], e["words"]), f"{name} list {l}: words"
                assert int(got["mt_draws"][l]) == e["mt_draws"], f"{name} list {l}: mt_draws"
                assert np.array_equal(got["dec"][a:b], e["decoded"]), f"{name} list {l}: decoded ids"
                if np.unique(li).size == li.size:  # (a multiset is checked against the reference's own decode, above)
                    assert np.array_equal(np.sort(got["dec"][a:b]), li), f"{name} list {l}: the decoded ids are not the list"
                if want_perm:
                    assert np.array_equal(got["perm"][a:b], e["perm"]), f"{name} list {l}: perm"
    finally:
        for k in MODES["default"]:
            monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def roc():
    from vector_db_id_compression_amd.codecs import RocLists

    return RocLists


@pytest.mark.parametrize("rng_name", list(RANGES))
@pytest.mark.parametrize("kind", KINDS)
def test_natural_order_decode_equals_other_modes_and_oracle(roc, oracle, monkeypatch, kind, rng_name):
    hi, need, _ = RANGES[rng_name]
    li = _list(kind, rng_name)
    assert 4097 <= li.size <= 17000 and need <= int(li.max()) < hi
    check_modes(roc, oracle, monkeypatch, [li, _rand(7, 100, hi)], f"{kind}-{rng_name}", want_perms=(True,))
