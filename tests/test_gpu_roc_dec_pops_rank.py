"""GPU: the two changes to the step of the bitmap chain decoders k_roc_decode_u2<20, true> / <18, false> (csrc/roc_u2.h):

* the rank inside the one bitmap word is taken from lane b = x & 63 of v_mbcnt_lo / v_mbcnt_hi of the broadcast word, read out with
  v_readlane at x itself (U2_DEC_RANK_1W): the instruction must take six bits of x, whatever the bits above them hold;
* the two slice pops are one classified shift (U2_DEC_TOP_P, csrc/u2_pops_ref.h): one test of the head, at most one refill, with the
  stack word carried from the previous step in a scalar register, so every way into the loop has to load that word.

Method and helpers of tests/test_gpu_roc_u2_decode.py: every case is one list of 4097 .. about 4300 ids with a list of 100 ids beside
it; the library's streams must equal the oracle's, decode_all the oracle's decode element by element in sampling order, and both must
be the same under VIDC_FORCE_GENERAL=1.  The pop cases first classify the oracle's decode of the list's stream with the Python port of
the header (tests/roc_pops_ref.py) and assert that the stream really reaches the classes the case is there for."""
import numpy as np
import pytest

import roc_pops_ref as pr
from test_gpu_roc_u2_decode import RANGES, _anchored, _check, _duplicate, _rand

pytestmark = pytest.mark.gpu

# (name, bits of the word that are set)
PATTERNS = (("all64", range(64)), ("bit0", (0,)), ("bit31", (31,)), ("bit32", (32,)), ("bit63", (63,)), ("bits31_32", (31, 32)),
            ("low_half", range(32)), ("high_half", range(32, 64)))


def _bit_position_list(rng_name):
    """the eight patterns in eight words spread over the range (every one of them far above word 0, so x >> 6 has high bits set),
    the other words filled with 4100 random ids"""
    hi, need, _ = RANGES[rng_name]
    nwords = hi // 64
    words = [nwords * (k + 1) // 9 + 3 * k + 1 for k in range(len(PATTERNS))]
    words[-1] = nwords - 1  # the last word of the range: the top id anchors the precision
    assert len(set(words)) == len(words) and min(words) >= 256
    core = np.concatenate([np.asarray([64 * w + b for b in bits], dtype=np.uint64) for w, (_, bits) in zip(words, PATTERNS)])
    fill = _rand(61, 4100, hi)
    fill = fill[~np.isin(fill >> np.uint64(6), np.asarray(words, dtype=np.uint64))]
    li = _anchored(np.union1d(core, fill), rng_name)
    for w, (name, bits) in zip(words, PATTERNS):  # the words hold exactly their pattern
        inside = li[(li >> np.uint64(6)) == np.uint64(w)]
        assert np.array_equal(inside, np.asarray([64 * w + b for b in bits], dtype=np.uint64)), name
    assert 4097 <= li.size <= 4300
    return li


@pytest.mark.parametrize("rng_name", list(RANGES))
def test_rank_at_every_bit_position_of_a_word(roc, oracle, monkeypatch, rng_name):
    li = _bit_position_list(rng_name)
    hi = RANGES[rng_name][0]
    _check(roc, oracle, monkeypatch, [li, _rand(7, 100, hi)], {"P20": 20, "P19": 19}.get(rng_name))


def _list_of_precision(P):
    """4100 random ids below 2^P whose maximum has bit P - 1 set (the precision follows the maximum id)"""
    li = _rand(70 + P, 4100, 1 << P)
    if int(li.max()) < 1 << (P - 1):
        li = np.append(li, np.uint64((1 << P) - 1))
    return li


@pytest.mark.parametrize("P", [20, 19, 18, 17, 16, 13])
def test_every_refill_class_of_the_slice_pops(roc, oracle, monkeypatch, P):
    li = _list_of_precision(P)
    assert oracle.list_precision(li) == P
    e = oracle.roc_encode(li, P)
    want = oracle.roc_decode(e["head"], e["words"], li.size, P, e["mt_draws"])[0]
    c = pr.classify_decode(e["head"], e["words"], li.size, P, want, e["mt_draws"], oracle.mt_table(64))
    print(f"P {P}: steps per class none / slice 0 / slice 1 / both {c['classes']}, slice-0 refills undone by the index push {c['undone']}")
    assert c["classes"][pr.NONE] >= 1 and c["classes"][pr.SLICE0] >= 1
    if P >= 17:
        assert c["classes"][pr.SLICE1] >= 1
    else:
        assert c["classes"][pr.SLICE1] == 0
    assert c["classes"][pr.BOTH] == 0 and c["max_popped"] <= 1, "a step refilled twice"
    _check(roc, oracle, monkeypatch, [li, _rand(7, 100, 1 << P)], P)


@pytest.mark.parametrize("rng_name", ["P20", "G1"])
def test_reentry_after_generic_steps_and_block_changes(roc, oracle, monkeypatch, rng_name):
    """4161 ids = 65 blocks of 64 steps and one step: the loop is left and entered again at every block change and around every
    generic step, and each entry loads the carried stack word again"""
    hi = RANGES[rng_name][0]
    li = _anchored(_rand(81, 4161, hi), rng_name)
    assert li.size == 4161
    _check(roc, oracle, monkeypatch, [li, _rand(7, 100, hi)], {"P20": 20}.get(rng_name))


@pytest.mark.parametrize("rng_name", ["P20", "G1"])
def test_reentry_multiset_goes_to_the_round1_body(roc, oracle, monkeypatch, rng_name):
    hi, need, _ = RANGES[rng_name]
    li = _duplicate(82, 4161, hi)
    assert np.unique(li).size == li.size - 1 and int(li.max()) >= need
    _check(roc, oracle, monkeypatch, [li, _rand(7, 100, hi)])


@pytest.fixture(scope="module")
def roc():
    from vector_db_id_compression_amd.codecs import RocLists

    return RocLists
