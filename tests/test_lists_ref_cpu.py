"""tests/lists_ref.py against the CPU oracle, and every id family against the boundary it is named after (no GPU).

The GPU tests (tests/test_gpu_ef_lists.py, tests/test_gpu_packed_lists.py) compare the kernels with the numpy model on these
families; they prove something about a case distinction of csrc/ef.hip only if the family reaches it.  The property tests below
assert that from ef_chunk_stats / ef_directory, for the families as committed: none is sampled."""
import time

import numpy as np
import pytest

import lists_ref as lr


@pytest.fixture(scope="module")
def fam():
    return {name: lr.family(name, 0) for name in lr.FAMILIES}


@pytest.mark.parametrize("name", lr.FAMILIES)
def test_model_equals_the_oracle_on_every_list(oracle, fam, name):
    for i, li in enumerate(fam[name]):
        assert li.dtype == np.uint64 and li.size and np.all(li[1:] >= li[:-1]), (name, i)
        mdl, e = lr.ef_list(li), oracle.ef_build(li)
        assert (mdl.l, mdl.low_nbits, mdl.high_nbits) == (e["l"], e["low_nbits"], e["high_nbits"]), (name, i)
        assert np.array_equal(mdl.low, e["low"]), (name, i, "low words")
        assert np.array_equal(mdl.high, e["high"]), (name, i, "high words")
        assert np.array_equal(e["decoded"], li), (name, i)
    s = lr.ef_sizes(fam[name] + [np.zeros(0, np.uint64)])
    assert s["total_bits"] == sum(lr.ef_list(li).low_nbits + lr.ef_list(li).high_nbits for li in fam[name])
    assert s["compressed_bytes"] == s["total_bits"] // 8


def test_model_is_fast_enough_for_every_position_tests():
    ids = np.sort(np.random.default_rng(0).integers(0, 1 << 31, 100_000, dtype=np.uint64))
    t = time.perf_counter()
    lr.ef_list(ids), lr.ef_chunk_stats(ids), lr.ef_directory(ids)
    assert time.perf_counter() - t < 1.0


def test_list_and_object_sizes_stay_small(fam):
    for name, lists in fam.items():
        big = [li.size for li in lists if li.size > 24000]  # (only the list with a chunk of more than 64 batches needs more)
        assert sum(big) <= 135_000 and len(big) <= 1, (name, big)
        assert sum(li.size for li in lists) <= 300_000, name


@pytest.mark.parametrize("name", lr.FAMILIES)
def test_family_is_deterministic_in_name_and_seed(name):
    a, b, c = lr.family(name, 3), lr.family(name, 3), lr.family(name, 4)
    assert len(a) == len(b) == len(c) and all(np.array_equal(x, y) for x, y in zip(a, b))
    if name in ("quotient_edges", "low_widths", "uniform", "owned_batches", "window_spans"):  # (the others are closed forms)
        assert any(not np.array_equal(x, y) for x, y in zip(a, c))


@pytest.mark.parametrize("bits", [1, 5, 13, 31, 32, 33, 47, 63, 64])
def test_packed_model_equals_the_oracle(oracle, bits):
    rng = np.random.default_rng(bits)
    mask = np.uint64((1 << bits) - 1)
    for n in (0, 1, 63, 64, 65, 513):
        cases = [rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1) & mask]
        cases += [lr.packed_patterns(n, bits, kind) for kind in lr.PACKED_PATTERNS]
        for ids in cases:
            assert np.all(ids <= mask)
            img = lr.packed_list(ids, bits)
            assert img.size == (n * bits + 7) // 8
            assert np.array_equal(img, oracle.packed_encode(ids, bits)), (bits, n)


def test_packed_patterns_are_what_they_say():
    for bits in (1, 13, 31, 32, 33, 63, 64):
        full = (1 << bits) - 1
        oz = lr.packed_patterns(8, bits, "ones_zeros")
        assert [int(x) for x in oz[:4]] == [full, 0, full, 0]
        alt = lr.packed_patterns(8, bits, "alternating")
        assert int(alt[0]) == 0x5555555555555555 & full and int(alt[1]) == 0xAAAAAAAAAAAAAAAA & full
        w = lr.packed_patterns(3 * bits, bits, "walking")
        assert [int(x) for x in w] == [1 << (i % bits) for i in range(3 * bits)]


def test_labels_cover_every_position_and_every_invalid_kind():
    sizes = np.array([3, 0, 5, 1, 0], dtype=np.int64)
    flat = np.arange(100, 109, dtype=np.uint64)
    lab = lr.all_labels(sizes, np.random.default_rng(0))
    want, invalid = lr.expect_labels(lab, sizes, flat)
    assert sorted(want[want >= 0].tolist()) == list(range(100, 109))  # every position once
    assert np.any(lab == -1) and np.any(lab < -1) and np.any((lab >> 32) >= sizes.size)
    l = lab >> 32
    inside = (lab >= 0) & (l < sizes.size)
    assert np.any(inside & (sizes[np.where(inside, l, 0)] == 0))  # aimed at an empty list
    assert invalid == int(((lab >= 0) & (want < 0)).sum()) and invalid > 0


# ------------------------------------------------------------------------------------------- each family reaches its boundary
def test_quotient_edges_put_u_on_both_sides_of_every_step_of_l(fam):
    seen = {}
    for li in fam["quotient_edges"]:
        seen.setdefault(li.size, set()).add((int(li[-1]), lr.ef_list(li).l))
    assert set(seen) == set(lr.QUOTIENT_M)
    for m in lr.QUOTIENT_M:
        ks = lr.quotient_ks(m)
        assert {0, 1, 5}.issubset(ks) and (20 in ks or max(ks) < 20)
        assert ((m << max(ks)) + 1 < 1 << 32) and ((m << (max(ks) + 1)) + 1 >= 1 << 32)
        for k in ks:
            below = 0 if k == 0 else k - 1  # (k = 0: u = m - 1 < m, the zero-quotient branch)
            above = 1 if (m, k) == (1, 0) else k  # (one id, u = 2: the next step already)
            assert {((m << k) - 1, below), (m << k, k), ((m << k) + 1, above)}.issubset(seen[m]), (m, k)
        assert (m // 2, 0) in seen[m]  # u < m: a multiset


def test_low_widths_hold_every_l_in_both_id_widths(fam):
    narrow, wide = {}, {}
    for li in fam["low_widths"]:
        (narrow if int(li[-1]) < 1 << 32 else wide).setdefault(lr.ef_list(li).l, set()).add(li.size)
    assert sorted(narrow) == list(range(32)) and sorted(wide) == list(range(32, 62))
    assert any(li.size == 1 and int(li[0]) == (1 << 32) - 1 for li in fam["low_widths"])
    for l in range(62):
        sizes = (narrow if l < 32 else wide)[l]
        want = {n for n in lr.LOW_WIDTH_SIZES if ((n + 1) << l) - 1 < (1 << 32 if l < 32 else 1 << 63)}
        assert sizes == want and 1 in sizes, l
    for n in lr.LOW_WIDTH_SIZES:  # every list size occurs with fields that straddle 32- and 64-bit word boundaries
        ls = {l for d in (narrow, wide) for l, s in d.items() if n in s and n > 1}
        assert n == 1 or any(l % 32 for l in ls)
    assert all(np.all(li < np.uint64(1 << 63)) for li in fam["low_widths"])


def test_constant_runs_fill_a_batch_and_leave_one_empty(fam):
    full = empty = False
    for li in fam["constant_runs"]:
        assert np.all(li == li[0])
        d = np.append(lr.ef_directory(li), li.size)
        cnt = np.diff(d)
        full |= bool(np.any(cnt == lr.BATCH_BITS))
        empty |= bool(cnt[-1] == 0)  # the last batch holds only the terminator
    assert full and empty
    assert {(li.size, int(li[0])) for li in fam["constant_runs"]} == {(n, v) for n in (1, 63, 64, 65, 4095, 4096, 4097, 8192, 8193)
                                                                      for v in (0, 7)}
    z = next(li for li in fam["constant_runs"] if li.size == 4096 and li[0] == 0)
    assert lr.ef_directory(z).tolist() == [0, 4096]


def test_consecutive_lists(fam):
    got = {(li.size, int(li[0])) for li in fam["consecutive"]}
    assert got == {(n, b) for n in (512, 513, 3000) for b in (0, 1, 1 << 20, (1 << 32) - n, 1 << 40)}
    assert all(np.all(np.diff(li.astype(np.int64)) == 1) for li in fam["consecutive"])


def test_head_and_outlier_ties_the_directory(fam):
    ties = 0
    tops = set()
    for li in fam["head_and_outlier"]:
        d = lr.ef_directory(li)
        ties += int(np.any((d[1:] == d[:-1]) & (d[1:] > lr.BATCH_BITS)))  # equal entries behind a head of more than 4096 ids
        tops.add((li.size, int(li[-1])))
    assert ties >= 3
    assert tops == {(n, t) for n in (2, 513, 2000, 6001) for t in ((1 << 31) - 1, (1 << 32) - 1, 1 << 40)}
    assert sum(1 for li in fam["head_and_outlier"] if li.size > 2 and int(li[1]) - int(li[0]) > 1 << 20) >= 9  # the mirror images


def test_chunk_seams_end_chunks_on_bit_0_and_bit_63_with_0_1_63_followers(fam):
    seen = set()
    for li in fam["chunk_seams"]:
        assert lr.ef_list(li).l == 0
        st = lr.ef_chunk_stats(li)
        for c in range(st["n"].size):
            if st["n"][c] == lr.CHUNK:
                seen.add((c, int(st["last_bit"][c]), int(st["followers"][c])))
    for c in range(len(lr.SEAM_IDS)):
        for bit, f in lr.SEAM_KINDS:
            assert (c, bit, f) in seen, (c, bit, f)
    assert {512, 1024}.issubset({li.size for li in fam["chunk_seams"]})


def test_batch_seams(fam):
    both = only95 = only96 = False
    hbs = set()
    for li in fam["batch_seams"]:
        m = lr.ef_list(li)
        a, b = 4095 in m.pos, 4096 in m.pos
        both |= a and b
        only95 |= a and not b
        only96 |= b and not a
        hbs.add(m.high_nbits)
    assert both and only95 and only96
    assert {4096, 4097, 8192, 8193}.issubset(hbs)  # exactly 64, 65, 128, 129 high words; 1 | 2 and 2 | 3 batches
    assert {(hb + 63) // 64 for hb in (4096, 4097, 8192, 8193)} == {64, 65, 128, 129}


def test_owned_batches(fam):
    owned = np.concatenate([lr.ef_chunk_stats(li)["owned_batches"] for li in fam["owned_batches"]])
    for k in lr.OWNED_BATCHES:
        assert np.any(owned == k), k
    assert np.any(owned > 64)
    # the four-or-fewer (ballot) form and the lane-per-batch form both meet chunks whose ids are spread over their batches
    spread = lr.ef_chunk_stats(fam["owned_batches"][1])["owned_batches"]
    assert {4, 5}.issubset(set(spread.tolist()))


def test_window_spans(fam):
    for li in fam["window_spans"]:
        owned = set(lr.ef_chunk_stats(li)["owned_words"].tolist())
        assert set(lr.WINDOW_SPANS).issubset(owned), owned


def test_objects_take_every_encoder_form_and_hold_every_list(fam):
    want = {"short": "short", "half": "half"}
    seen = set()
    for name in lr.OBJECTS:
        for route in lr.ROUTES:
            lists, nbase = lr.object_lists(name, route)
            form = lr.encoder_form(lists)
            assert form == {"wide": "wide", "unsorted": "general"}.get(route, want.get(name, "full")), (name, route)
            assert sum(li.size for li in lists) <= 300_000 and sum(1 for li in lists[:nbase] if not li.size) >= 2
            assert lists[0].size == 0 and lists[nbase - 1].size == 0
            assert (len(lists) > nbase) == (route in ("wide", "unsorted"))
            if route == "wide":
                assert all(int(li.max()) >= lr.NARROW for li in lists[nbase:])
            seen |= {li.tobytes() for li in lists}
    for name, lists in fam.items():
        for i, li in enumerate(lists):
            assert li.tobytes() in seen, (name, i)
    sizes = {n: [li.size for li in lr.base_lists(n)] for n in lr.OBJECTS}
    assert max(sizes["short"]) == 256 and 256 in sizes["half"] and 768 in sizes["half"]  # chunks of exactly 256 ids in both SMALL forms
    assert {511, 512, 513}.issubset(sizes["half"]) and max(sizes["half"]) == 1024
    # lists of more than 8 chunks leave their chunk records to k_ef_big_recs: 4096 ids is the last size that does not
    assert {4096, 4097}.issubset(sizes["full_q"]) and {4096, 4097}.issubset(sizes["full_runs"])
    # decode_lists shares a list of 4096 ids or more between workgroups
    assert all(max(sizes[n]) >= 4096 for n in lr.OBJECTS if n.startswith("full"))


def test_uniform_control(fam):
    assert [li.size for li in fam["uniform"]] == [1, 2, 5, 63, 64, 65, 300, 5000, 20000]
