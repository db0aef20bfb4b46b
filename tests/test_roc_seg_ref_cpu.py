"""CPU: the numpy statement of the segmented ROC container (tests/roc_seg_ref.py) against a brute-force loop and the CPU oracle.

The model is what the GPU tests compare the library with, so it is pinned here first: the segment of every id, the stable order inside
a segment, the inner offsets, the permutation compose; every model segment round-trips through the oracle, and adding the base back
gives the list as a set and the stated decode order.  The size condition: 52 114 uniform distinct ids in [0, 10^6) from default_rng(1) at
T = 1024 / 2048 / 4096 take at most 1.02 x the bytes of the oracle's plain bit_width(max) stream (measured 1.0035 / 0.998 / 0.995; T =
256, measured 1.048, is recorded in DESIGN 9c and not bounded).
"""
import numpy as np
import pytest

import roc_seg_ref as sr


def random_case(rng, T, B, sizes, shuffled=True):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    lists = []
    for n in sizes:
        li = rng.choice(1 << B, n, replace=False).astype(np.uint64) if n <= 1 << B else rng.integers(0, 1 << B, n).astype(np.uint64)
        lists.append(li if shuffled else np.sort(li))
    return off, np.concatenate(lists + [np.zeros(0, np.uint64)])


CASES = [(16, 10, [0, 1, 16, 17, 32, 33, 100]), (64, 12, [64, 65, 129, 0, 1000]), (16, 4, [5, 16]), (16, 3, [100, 3]),
         (1024, 20, [2049, 7, 1025])]


@pytest.mark.parametrize("T,B,sizes", CASES)
@pytest.mark.parametrize("shuffled", [False, True])
def test_model_against_the_brute_force_loop(T, B, sizes, shuffled):
    rng = np.random.default_rng(T * 131 + B + shuffled)
    off, ids = random_case(rng, T, B, sizes, shuffled)
    m = sr.split(off, ids, T, B)
    inner, pos = sr.split_brute(off, ids, T, B)
    assert int(m["seg_first"][-1]) == len(inner)
    for l, n in enumerate(sizes):
        k = sr.seg_k(n, T, B)
        assert int(m["k"][l]) == k and int(m["shift"][l]) == B - k and int(m["seg_first"][l + 1] - m["seg_first"][l]) == 1 << k
        assert k == 0 or n > T
        # the segments of a list are consecutive: inner and outer offsets address the same positions
        assert int(m["inner_offsets"][int(m["seg_first"][l])]) == int(off[l])
    for i, (seg, p) in enumerate(zip(inner, pos)):
        a, b = int(m["inner_offsets"][i]), int(m["inner_offsets"][i + 1])
        assert m["rebased"][a:b].tolist() == seg, i
        assert m["src_pos"][a:b].tolist() == p, i
        assert p == sorted(p), "stable: input order inside a segment"
    # perm composition: with an arbitrary inner permutation, ids[perm] = base + rebased taken through it
    ip = np.concatenate([rng.permutation(len(s)) for s in inner] + [np.zeros(0, np.int64)]).astype(np.uint32)
    perm = sr.compose_perm(m, ip)
    base = np.repeat(sr.bases(m), np.diff(m["inner_offsets"].astype(np.int64)))
    start = np.repeat(m["inner_offsets"][:-1].astype(np.int64), np.diff(m["inner_offsets"].astype(np.int64)))
    lstart = np.repeat(off[:-1].astype(np.int64), np.diff(off.astype(np.int64)))
    assert np.array_equal(ids[lstart + perm], m["rebased"][start + ip] + base)


def test_k_is_capped_and_too_many_segments_are_refused():
    assert sr.seg_k(16, 16, 10) == 0 and sr.seg_k(17, 16, 10) == 1 and sr.seg_k(33, 16, 10) == 2
    assert sr.seg_k(1000, 16, 3) == 3, "k capped at B"
    assert sr.seg_k(16 * 1024, 16, 20) == 10
    off = np.array([0, 16 * 1024 + 1], np.uint64)
    with pytest.raises(ValueError):
        sr.plan(off, 16, 20)
    with pytest.raises(ValueError):
        sr.split(np.array([0, 2], np.uint64), np.array([3, 1 << 10], np.uint64), 16, 10)
    assert sr.universe_bits([]) == 1 and sr.universe_bits([0]) == 1 and sr.universe_bits([1023]) == 10 and sr.universe_bits([1024]) == 11


@pytest.mark.parametrize("T,B,sizes", CASES)
def test_every_segment_round_trips_through_the_oracle(oracle, T, B, sizes):
    rng = np.random.default_rng(T + B)
    off, ids = random_case(rng, T, B, sizes)
    m = sr.split(off, ids, T, B)
    encs = sr.encode_segments(m, oracle)
    base = sr.bases(m)
    want = sr.decode_order(m, encs)
    for i, e in enumerate(encs):
        seg = sr.segment(m, i)
        if e is None:
            assert seg.size == 0
            continue
        assert e["precision"] == sr.bit_width(seg.max()) <= int(m["shift"][np.searchsorted(m["seg_first"], i, side="right") - 1])
        dec = oracle.roc_decode(e["head"], e["words"], seg.size, e["precision"], e["mt_draws"])[0]
        assert np.array_equal(dec, e["order"]) and np.array_equal(seg[e["perm"]], e["order"])
        a, b = int(m["inner_offsets"][i]), int(m["inner_offsets"][i + 1])
        assert np.array_equal(dec + base[i], want[a:b])
    perm = sr.compose_perm(m, sr.inner_perm(m, encs))
    for l in range(len(sizes)):
        a, b = int(off[l]), int(off[l + 1])
        assert np.array_equal(np.sort(want[a:b]), np.sort(ids[a:b])), "the list as a set"
        assert np.array_equal(ids[a:b][perm[a:b]], want[a:b]), "the stated decode order"
    assert sr.compressed_bytes(m, encs) == sr.inner_bytes(encs) + 4 * sum(1 << sr.seg_k(n, T, B) for n in sizes if n > T)


@pytest.mark.parametrize("T", [1024, 2048, 4096])
def test_size_against_the_plain_stream(oracle, T):
    ids = np.sort(np.random.default_rng(1).choice(10 ** 6, 52114, replace=False).astype(np.uint64))
    off = np.array([0, ids.size], np.uint64)
    plain = oracle.roc_encode(ids, sr.bit_width(ids.max()))
    plain_bytes = 8 + 4 * plain["words"].size
    m = sr.split(off, ids, T, sr.universe_bits(ids))
    ratio = sr.compressed_bytes(m, sr.encode_segments(m, oracle)) / plain_bytes
    print(f"T = {T}: {1 << int(m['k'][0])} segments, size ratio {ratio:.4f}")
    assert ratio <= 1.02
