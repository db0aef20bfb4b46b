"""GPU: the classified ring traffic of the bitmap chain decoder's step (U2_DEC_STEP bit 2 in csrc/roc_u2.h; csrc/u2_dec_ring_ref.h and
tests/roc_dec_ring_ref.py are the same on the host) on the smallest lists that reach all of it.  Method and helpers are those of
tests/test_gpu_roc_u2_decode.py: one list of 4101 .. 4300 ids with a 100-id list beside it; streams equal to the oracle's, decode_all
equal to the oracle's decode element by element, both the same under VIDC_FORCE_GENERAL=1.

  * precisions 20 and 19 (the 20-bit launch: word-granular rows, and the four-word step under VIDC_U2_DEC_WORD=0 at 20) and 18, 17, 16,
    13 (the 18-bit launch; p1 = 2, 1, 0, 0).  Before decoding, each case steps the oracle's decode through the Python port and
    asserts that the stream reaches the classes it is there for: quiet, refill only and, where p1 > 0, the slice-1 side path.
  * class x copy: roc_dec_ring_ref.kernel_walk follows the kernel's while loop with its ring glue (refill below 22 words, spill above
    56, a generic step outside 18 .. 53) and the control of the eight-copy loop (copy 0 at every entry and every block change, the
    ring test behind copy 7 alone, blocks of 64 steps counted from the entry), and the test asserts that every class occurs in every
    copy, so every side body, both ways into its push and the quiet path behind each of them have run.
  * re-entry: 4161 ids, so that the list runs through dozens of block changes inside the asm (the re-entry of U2_DEC_OUTER_U) and
    dozens of exits through the ring test with a ring refill and a new U2_DEC_ENTRY_U behind each; both reload both carried
    scalars.  The case asserts a loud step as the first step behind a block change and as the first step behind a new entry.
  * multiset: 4161 ids below 2^10 and below 2^6 go to the 18-bit launch, run the fast loop, fail the recount and are decoded again
    by the round-1 body; the result is the oracle's.  The model steps the stream with the rank the kernel's counters and bitmap give
    (classify_decode(rank="bitmap"): what the first pass really sees once an id has come twice).  It shows that the stream reaches
    "spill only" (h_hi >= lq, nmax > 2^P) inside the fast loop, the class no set reaches, and that the loop is entered again right
    behind generic steps, on both ways there are: the ring regrows to 18 words from below, and a stretch of generic steps at
    54 .. 56 words ends in a ring spill.  The test asserts all of that.
  * a LOUD step right behind a GENERIC step: no stream reaches it, and the multiset cases assert what they find instead (every
    first step behind a generic step is quiet and that generic step was "spill only").  The reason: "refill only" and the side path
    need head' < 2^(31 + P) / nmax, so nmax < 2^P; "spill only" needs head' >= 2^(63 + P) / nmax (about), so nmax > 2^P; nmax only
    grows.  The ring therefore only shrinks up to step 2^P and only grows behind it.  A stretch of generic steps inside the list is
    left only upwards: fewer than 18 words with nothing below the ring regrow to 18, or 54 .. 56 words grow past 56 and the glue
    spills 32; either way the last generic step was "spill only".  Behind such a step H = h_hi >= lq, so the next
    h = (H nmax + r) >> P is at least (2^31 - nmax) >> P >= lq' and far below lq' 2^32: quiet.  (A ring of fewer than 22 words with
    words below it is refilled, not stepped generically; an exit through head' < 2^31 runs the second half of the push in C++ and
    enters again without a generic step.)  The entry's reload is the same code on every way in and its first step is loud in the
    re-entry case above; the host test (tests/u2_dec_ring_test.cpp) carries a loud step behind an exit."""
import numpy as np
import pytest

import roc_dec_ring_ref as ref

pytestmark = pytest.mark.gpu

def _ids(seed, n, lo, hi):
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(hi - lo, size=n, replace=False) + lo).astype(np.uint64)


def _list(P, n, seed=0):
    """n distinct ids whose maximum has exactly P bits (the list's precision, and with it the launch, follow from the maximum)"""
    top = np.array([(1 << P) - 1], np.uint64)
    return np.concatenate([_ids(100 * P + seed, n - 1, 0, (1 << P) - 1), top])


def _multiset(bits, n, seed):
    rng = np.random.default_rng(seed)
    return np.sort(np.concatenate([rng.integers(0, 1 << bits, n - 1), [(1 << bits) - 1]])).astype(np.uint64)


_cache = {}


def _model(oracle, key, li, multiset=False):
    """oracle encode and decode of the list; the model's classes by step (a set: every step's id checked against the oracle's; a
    multiset: stepped with the kernel's bitmap rank) and the kernel's way through them (computed once per list)"""
    if key not in _cache:
        P = oracle.list_precision(li)
        e = oracle.roc_encode(li, P)
        want = oracle.roc_decode(e["head"], e["words"], li.size, P, e["mt_draws"])[0]
        m = ref.classify_decode(e["head"], e["words"], li.size, P, want_ids=None if multiset else want, mt_draws=e["mt_draws"],
                                mt_table=oracle.mt_table(1024), rank="bitmap" if multiset else "set")
        w = ref.kernel_walk(m, li.size, e["words"].size)
        by_copy = np.zeros((8, 4), np.int64)
        for i in np.flatnonzero(w["path"] == 1):
            by_copy[w["copy"][i], m["cls"][i]] += 1
        _cache[key] = dict(P=P, e=e, want=want, m=m, w=w, by_copy=by_copy)
    return _cache[key]


@pytest.fixture(scope="module")
def roc():
    from vector_db_id_compression_amd.codecs import RocLists

    return RocLists


def _run(roc, off, ids):
    r = roc.encode(off, ids)
    info = r.info()
    dec = r.decode_all().cpu().numpy().view(np.uint64).copy()
    return dict(heads=info["heads"], nwords=info["nwords"], precision=info["precision"], mt_draws=info["mt_draws"],
                words=r.all_words(), dec=dec)


def _check(roc, oracle, monkeypatch, li, mod, beside):
    lists = [li, beside]
    off = np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.uint64)
    ids = np.concatenate(lists)
    monkeypatch.delenv("VIDC_FORCE_GENERAL", raising=False)
    got = _run(roc, off, ids)
    woff = np.concatenate([[0], np.cumsum(got["nwords"].astype(np.int64))])
    for l, x in enumerate(lists):
        if l == 0:
            P, e, want = mod["P"], mod["e"], mod["want"]
        else:
            P = oracle.list_precision(x)
            e = oracle.roc_encode(x, P)
            want = oracle.roc_decode(e["head"], e["words"], x.size, P, e["mt_draws"])[0]
        a, b = int(off[l]), int(off[l + 1])
        assert int(got["precision"][l]) == P, f"list {l}: precision"
        assert int(got["heads"][l]) == e["head"], f"list {l}: head"
        assert int(got["nwords"][l]) == e["words"].size, f"list {l}: nwords"
        assert np.array_equal(got["words"][woff[l]:woff[l + 1]], e["words"]), f"list {l}: words"
        assert int(got["mt_draws"][l]) == e["mt_draws"], f"list {l}: mt_draws"
        bad = np.flatnonzero(got["dec"][a:b] != want)
        assert bad.size == 0, f"list {l}: decoded ids differ from the oracle's at {bad[:5]} of {x.size}"
    monkeypatch.setenv("VIDC_FORCE_GENERAL", "1")
    gen = _run(roc, off, ids)
    for k in got:
        assert np.array_equal(got[k], gen[k]), f"'{k}' differs under VIDC_FORCE_GENERAL=1"


def _want_classes(P):
    p1, _ = ref.pop_widths(P)
    return (ref.QUIET, ref.REFILL, ref.SIDE) if p1 else (ref.QUIET, ref.REFILL)


CASES = [(20, 4101, True), (20, 4101, False), (19, 4101, True), (18, 4101, True), (17, 4101, True), (16, 4101, True), (13, 4101, True)]


@pytest.mark.parametrize("P,n,word", CASES)
def test_every_class_in_every_copy(roc, oracle, monkeypatch, P, n, word):
    li = _list(P, n)
    mod = _model(oracle, (P, n, 0), li)
    assert mod["P"] == P
    counts, by = mod["m"]["counts"], mod["by_copy"]
    print(f"P {P} n {n}: quiet / refill only / spill only / side = {counts}; by copy {by.tolist()}")
    assert counts[ref.SPILL] == 0                      # a set: nmax <= 2^P
    for c in _want_classes(P):
        assert counts[c] >= 100, f"class {ref.NAMES[c]}: {counts}"
        for copy in range(8):
            assert by[copy, c] > 0, f"class {ref.NAMES[c]} never runs in copy {copy}: {by.tolist()}"
    if ref.SIDE not in _want_classes(P):
        assert counts[ref.SIDE] == 0
    monkeypatch.setenv("VIDC_U2_DEC_WORD", "1" if word else "0")
    _check(roc, oracle, monkeypatch, li, mod, _ids(7, 100, 0, 1 << P))


@pytest.mark.parametrize("P", [20, 18])
def test_reentry_reloads_both_carried_scalars(roc, oracle, monkeypatch, P):
    """4161 ids: a loud step is the first step behind a block change inside the asm and the first step behind a new entry"""
    li = _list(P, 4161, 1)
    mod = _model(oracle, (P, 4161, 1), li)
    cls, w = mod["m"]["cls"], mod["w"]
    entries = w["entry_first"].copy()
    entries[0] = False
    print(f"P {P}: {int(entries.sum())} entries behind the first ({int((cls[entries] != ref.QUIET).sum())} with a loud first step), "
          f"{int(w['block_first'].sum())} block changes inside the asm ({int((cls[w['block_first']] != ref.QUIET).sum())} loud), "
          f"{w['ring_exits']} exits through the ring test, {int((w['path'] == 0).sum())} generic steps")
    # about 1200 words leave the ring 32 at a time: dozens of ring exits, each with an entry behind it; 4161 steps in blocks of at most 64
    assert w["ring_exits"] >= 20 and entries.sum() >= 20 and w["block_first"].sum() >= 20
    assert entries.sum() + w["block_first"].sum() + 1 >= 4161 // 64
    assert (cls[w["block_first"]] != ref.QUIET).any(), "no loud step at the head of a block"
    assert (cls[entries] != ref.QUIET).any(), "no loud step behind a new entry"
    assert not w["behind_generic"].any()               # (a set leaves the loop for generic steps only at its tail: the module's docstring)
    _check(roc, oracle, monkeypatch, li, mod, _ids(7, 100, 0, 1 << P))


@pytest.mark.parametrize("bits", [10, 6])
def test_multiset_reaches_spill_only_and_goes_to_the_round1_body(roc, oracle, monkeypatch, bits):
    li = _multiset(bits, 4161, 10)
    assert li.size == 4161 and np.unique(li).size <= 1 << bits
    mod = _model(oracle, ("multiset", bits, 10), li, multiset=True)
    assert mod["P"] == bits
    m, w, by = mod["m"], mod["w"], mod["by_copy"]
    cls = m["cls"]
    assert m["distinct"] < li.size                      # the first pass sets fewer bits than it decoded ids: the recount fails
    bg = np.flatnonzero(w["behind_generic"])
    ring = m["sp_before"][bg - 1] >= ref.RING_LO        # the generic step in front ran on a ring above 53 words, not below 18
    print(f"multiset P {bits} n 4161: quiet / refill only / spill only / side = {m['counts']}; in the loop by copy {by.tolist()}; "
          f"entries behind generic steps at {bg.tolist()} ({int(ring.sum())} of them behind a stretch above 53 words), classes there "
          f"{cls[bg].tolist()}, of the generic steps in front {cls[bg - 1].tolist()}")
    assert by[:, ref.SPILL].sum() > 0, "the stream does not reach 'spill only' inside the fast loop"
    assert bg.size >= 3, "the loop is not entered behind generic steps"
    assert (~ring).any(), "no entry behind a regrowth to 18 words"
    if bits == 6:
        assert ring.any(), "no entry behind a stretch of generic steps at 54 .. 56 words"
    assert (cls[bg] == ref.QUIET).all() and (cls[bg - 1] == ref.SPILL).all()  # (never loud: the module's docstring says why)
    _check(roc, oracle, monkeypatch, li, mod, _ids(7, 100, 0, 1 << 10))
