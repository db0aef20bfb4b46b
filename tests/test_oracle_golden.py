"""CPU: the clean-room oracle (oracle/vidc_oracle.c) against the reference-generated golden vectors,
and against the compiled reference itself when oracle/_ref is available."""
import json
import os

import numpy as np
import pytest

from golden_cases import CASES, fnv_stream, fnv_u64, make_ids, ref_random_inputs

CASE_BY_NAME = {c["name"]: c for c in CASES}


def test_mt19937_table(oracle):
    # codec.h:16-18: mt19937(1234); first outputs per SURVEY 8a-Q5
    t = oracle.mt_table(8)
    assert list(t) == [822569775, 2137449171, 2671936806, 3512589365, 1880026316, 2629000564, 3373089432, 3312965625]


def test_precision_rule(oracle):
    # custom_invlists_impl.cpp:163-164
    assert oracle.precision(0) == 0
    assert oracle.precision(1) == 0
    assert oracle.precision(2) == 1
    assert oracle.precision(3) == 2
    assert oracle.precision(1024) == 10  # pow-2 quirk: one bit short
    assert oracle.precision(1025) == 11
    assert oracle.precision(999999) == 20
    assert oracle.precision(2**31 - 1) == 31
    for m in [2, 3, 4, 5, 7, 8, 9, 1000, 65535, 65536, 65537, 2**30, 2**30 + 1, 2**31 - 1]:
        assert oracle.precision(m) == (m - 1).bit_length()


def test_kat_values(golden):
    g = {c["name"]: c for c in golden}
    k1 = g["kat1_test_codec_main_xx"]
    assert k1["head"] == 22906489391 and k1["words"] == [2873710996, 612831110, 2733404530]
    assert k1["decoded"] == [12351235, 17781778, 49024902, 36663666]
    k2 = g["kat2_tiny_p4"]
    assert k2["head"] == 50039995826800 and k2["words"] == [] and k2["decoded"] == [3, 9, 1, 5, 7, 0]
    # SURVEY KAT3 heads (its FNV digests used an unstated byte convention and are not reproduced here;
    # the digests in the fixture are FNV-1a-64 over head LE8 || words LE4, see golden_cases.fnv_stream)
    assert g["kat3_test_codec_seed0"]["head"] == 539341665706
    assert g["kat3_test_codec_seed1"]["head"] == 538759805253
    assert g["kat3_test_codec_seed2"]["head"] == 539484581657
    for s in (0, 1, 2):
        c = g[f"kat3_test_codec_seed{s}"]
        assert 8 + 4 * c["nwords"] == 44324  # test_codec.cpp:91 size for every seed


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_oracle_matches_golden(oracle, golden, name):
    g = {c["name"]: c for c in golden}[name]
    ids = make_ids(CASE_BY_NAME[name])
    n, prec = g["n"], g["precision"]
    assert ids.size == n
    if "ids" in g:
        assert [int(x) for x in ids] == g["ids"]
    if CASE_BY_NAME[name].get("precision") is None and n:
        assert oracle.list_precision(ids) == prec
    enc = oracle.roc_encode(ids, prec)
    assert enc["head"] == g["head"]
    assert enc["words"].size == g["nwords"]
    assert fnv_stream(enc["head"], enc["words"]) == g["stream_fnv"]
    assert fnv_u64(enc["order"]) == g["order_fnv"]
    assert fnv_u64(enc["perm"].astype(np.uint64)) == g["perm_fnv"]
    dec, end_head, end_words, _ = oracle.roc_decode(enc["head"], enc["words"], n, prec, enc["mt_draws"])
    assert fnv_u64(dec) == g["decoded_fnv"]
    if "decoded" in g:
        assert [int(x) for x in dec] == g["decoded"]
        assert [int(x) for x in enc["words"]] == g["words"]
        assert [int(x) for x in enc["perm"]] == g["perm"]
    if g["roundtrip_is_order"]:
        assert np.array_equal(dec, enc["order"])
    if g["roundtrip_set_ok"]:
        # SURVEY appendix A self-check invariant: valid streams decode back to the initial state
        assert end_head == 1 << 31
        assert np.array_equal(np.sort(dec), np.sort(ids))


def test_oracle_vs_compiled_reference_random():
    """120 random lists: the oracle's stream, order, permutation and decode against the reference's, as recorded in
    tests/golden/roc_ref_random.json (make_golden.py), and against the compiled reference itself when oracle/_ref is built."""
    from oracle.pyoracle import Oracle, Ref

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roc_ref_random.json")) as f:
        recorded = json.load(f)["cases"]
    o = Oracle()
    r = Ref() if Ref.available() else None
    assert len(recorded) == 120
    for (t, ids), g in zip(ref_random_inputs(), recorded):
        n = ids.size
        assert g["t"] == t and g["n"] == n and fnv_u64(ids) == g["ids_fnv"]  # the inputs the fixture was recorded for
        prec = o.list_precision(ids)
        assert prec == g["precision"]
        a = o.roc_encode(ids, prec)
        assert a["head"] == g["head"] and a["words"].size == g["nwords"] and fnv_stream(a["head"], a["words"]) == g["stream_fnv"]
        assert fnv_u64(a["order"]) == g["order_fnv"] and fnv_u64(a["perm"].astype(np.uint64)) == g["perm_fnv"]
        d = o.roc_decode(a["head"], a["words"], n, prec, a["mt_draws"])
        assert fnv_u64(d[0]) == g["decoded_fnv"] and d[1] == g["end_head"] and fnv_stream(d[1], d[2]) == g["end_stream_fnv"]
        if r is None:
            continue
        c = r.container_encode(ids, prec, shuffle_seed=t)
        assert a["head"] == c["head"] and np.array_equal(a["words"], c["words"])
        assert np.array_equal(a["order"], c["order"]) and np.array_equal(a["perm"], c["perm"])
        d = o.roc_decode(a["head"], a["words"], n, prec, a["mt_draws"])
        d2 = r.decompress(a["head"], a["words"], n, prec)
        assert np.array_equal(d[0], d2[0]) and d[1] == d2[1] and np.array_equal(d[2], d2[2])


def test_packed_bits_layout(oracle):
    # custom_invlists_impl.cpp:68-70 and the in-tree LSB-first reader :35-58
    assert oracle.packed_bits_for(0) == 0
    assert oracle.packed_bits_for(1) == 1
    assert oracle.packed_bits_for(1000000) == 20
    assert oracle.packed_bits_for(1023) == 10 and oracle.packed_bits_for(1024) == 11
    code = oracle.packed_encode([5, 2, 7], 3)  # 101 010 111 -> bits LSB first: 1,0,1, 0,1,0, 1,1,1
    assert list(code) == [0b11010101, 0b00000001]
    ids = np.array([0, 999999, 123456, 1, 524288], dtype=np.uint64)
    code = oracle.packed_encode(ids, 20)
    assert code.size == (5 * 20 + 7) // 8
    assert np.array_equal(oracle.packed_decode(code, 5, 20), ids)


def test_elias_fano_formulas(oracle):
    # elias_fano.hpp:28-29
    ids = np.array([3, 4, 7, 13, 14, 15, 21, 43], dtype=np.uint64)
    ef = oracle.ef_build(ids)
    assert ef["l"] == 2  # msb(43 / 8) = msb(5) = 2
    assert ef["low_nbits"] == 16 and ef["high_nbits"] == (8 + 1) + (43 >> 2) + 1
    assert np.array_equal(ef["decoded"], ids)
    assert np.array_equal(ef["select_head"], ids)
    one = oracle.ef_build(np.array([0], dtype=np.uint64))
    assert one["l"] == 0 and one["high_nbits"] == 3 and list(one["decoded"]) == [0]
    rng = np.random.default_rng(5)
    for _ in range(20):
        n = int(rng.integers(1, 400))
        ids = np.sort(rng.choice(1 << 20, size=n, replace=False).astype(np.uint64))
        ef = oracle.ef_build(ids)
        assert np.array_equal(ef["decoded"], ids)
        assert np.array_equal(ef["select_head"], ids[:64])


def test_wavelet_select_semantics(oracle):
    ln = np.array([2, 0, 1, 0, 2, 2, 1, 0], dtype=np.uint32)
    assert oracle.wt_select(ln, 0, 0) == 1 and oracle.wt_select(ln, 0, 2) == 7
    assert oracle.wt_select(ln, 2, 1) == 4 and oracle.wt_select(ln, 1, 5) == -1
