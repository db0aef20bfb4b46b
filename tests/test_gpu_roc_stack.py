"""The ANS word stacks of the ROC kernels at underflow, regrowth and the edge of the 1024-word mt19937 table.

Every kernel family carries its own stack -- the register ring of the wave-per-list kernels with its spill / refill / re-spill scratch
(csrc/wave.h; the general kernels, the bitmap chains of roc_u.h and roc_u2.h, r2 / b2), the LDS rings and the 8-deep stacks of pushed
words of the lane-per-list (roc_lane.h) and row-per-list kernels (roc_grp.h), the tiny kernel's strip -- and every one restates "a pop
from the empty stack draws the next table word; the 1025th draw is an error".  The lists of tests/roc_stack_ref.py (searched on the CPU
oracle, pinned by tests/test_roc_stack_ref_cpu.py) reach those paths; what the library must produce is the oracle's, list by list.

One case = one call.  A case runs under every kernel-family mode that can take it -- the mode table of tools/fuzz_families.py, the
automatic policy, VIDC_OLD_U=1 and VIDC_NO_R2=1 --, with and without the permutation, and every mode must give the same streams, the
same decode and the same refusal.  Per mode: info() and all_words() equal the model; decode_all equals the oracle's decode of that
stream element by element; decode_lists of a subset in another order gives the same; the permutation equals the oracle's; the same
streams imported (RocLists.from_streams with mt_draws) decode to the same; last_decode_nonclean is the number of lists whose decode
does not end in the initial state.  Where a decode is a chain of ten thousand steps and more over a multiset (about 10 us per step)
the work is cut to what differs: lists beyond 4096 ids run under the five modes that treat them differently (LONG_MODES), the
34 000-id class with the permutation only, the second precision of the 8192 / 16 384 bounds and the regrowth calls outside the
automatic mode without it.

Found on the way and outside the contract (ids are below 2^31): an imported stream that decodes to ids of 2^31 and more -- P = 32
and table words instead of stream words -- comes out differently from the tiny lane decoder, whose register rank compares ids as
signed numbers, than from the wave-per-list kernels and the reference.  No case here decodes to such ids.

Hand-overs between families (the test checks the result, and the hand-back count where the library tells it):
  * the universe-bitmap encoders (k_roc_encode_u2, lists of 4097 or more ids below 2^20 in the automatic mode) return a list whose
    ids do not fit its precision -- every C2 / G3 / C3 edge list and the long partial lists -- to the general encoder;
  * lane- and row-per-list decoders hand a list back (VIDC_ST_RETRY) once it holds more than 8 pushed words: the depth-9 lists
    exactly, and nearly every list of the partial / edge / regrowth families under VIDC_FORCE_LANE / VIDC_FORCE_GRP;
  * k_roc_decode_b2<32 .. 256> hands back the low-precision lists of small calls whose few distinct values fill a member row;
  * the multisets go to the general encoder wherever a kernel needs strictly ascending input.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import append_ref as ar
import roc_stack_ref as rs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("VIDC_FORCE_GENERAL", "VIDC_FORCE_LANE", "VIDC_NO_LANE", "VIDC_FORCE_GRP", "VIDC_NO_GRP", "VIDC_NO_LANE_REG", "VIDC_NO_LANE_PAIR",
         "VIDC_LANE_QUAD", "VIDC_PAIR_MIN", "VIDC_NO_LANE128", "VIDC_LANE_ALIGN", "VIDC_LANE_LOOP", "VIDC_NO_R2", "VIDC_OLD_U", "VIDC_B2_MASK",
         "VIDC_NO_LENGTH_CLASSES")
OVERFLOW, INVALID = "vidc status -5:", "vidc status -1:"   # VIDC_ERR_OVERFLOW, VIDC_ERR_INVALID (include/vidc.h)
TABLE = rs.limits()["VIDC_MT_TABLE"]


def _modes():
    """name -> environment: tools/fuzz_families.py's table, the automatic policy, the round-1 bitmap kernels, no r2 / b2 chains"""
    spec = importlib.util.spec_from_file_location("fuzz_families", os.path.join(ROOT, "tools", "fuzz_families.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    modes = {"auto": {}}
    modes.update({k: {n: v for n, v in env.items() if v != "0"} for k, env in mod.MODES.items()})
    modes["old_u"] = {"VIDC_OLD_U": "1"}
    modes["no_r2"] = {"VIDC_NO_R2": "1"}
    assert set(mod.MODES) == {"lane", "wave", "general", "row", "lane_quad", "lane_pair", "lane_old"}
    return modes


@pytest.fixture(scope="module")
def modes():
    return _modes()


@pytest.fixture(scope="module")
def roc():
    from vector_db_id_compression_amd.codecs import RocLists

    return RocLists


@pytest.fixture(scope="module")
def calls(oracle):
    return rs.all_calls(oracle)


@pytest.fixture(scope="module")
def expected(oracle, calls):
    """the model of every list of every call, computed once"""
    return {name: rs.expect(oracle, c) for name, c in calls.items()}


def _pin(monkeypatch, env):
    for name in HOOKS:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        assert name in HOOKS
        monkeypatch.setenv(name, value)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _error():
    from vector_db_id_compression_amd._lib import VidcError

    return VidcError


def _streams_of(want):
    off = np.concatenate([[0], np.cumsum([m["n"] for m in want])]).astype(np.uint64)
    words = np.concatenate([m["words"] for m in want] + [np.zeros(0, np.uint32)])
    return off, [m["precision"] for m in want], [m["head"] for m in want], [m["nwords"] for m in want], words, [m["mt_draws"] for m in want]


def _check_streams(r, want, what):
    """precision, head, nwords, mt_draws and every word of every list equal the model"""
    info = r.info()
    assert [int(v) for v in info["sizes"]] == [m["n"] for m in want], what
    assert [int(v) for v in info["precision"]] == [m["precision"] for m in want], what
    assert [int(v) for v in info["mt_draws"]] == [m["mt_draws"] for m in want], what
    assert [int(v) for v in info["nwords"]] == [m["nwords"] for m in want], what
    assert [int(v) for v in info["heads"]] == [m["head"] for m in want], what
    words = r.all_words()
    assert np.array_equal(words, _streams_of(want)[4]), what
    return info, words


def _check_decode(r, want, what, nonclean=True):
    """decode_all element by element, then decode_lists of [last, first, a middle one, last again]"""
    off = np.concatenate([[0], np.cumsum([m["n"] for m in want])]).astype(np.int64)
    dec = _u64(r.decode_all())
    for l, m in enumerate(want):
        bad = np.flatnonzero(dec[off[l]:off[l + 1]] != m["order"])
        assert bad.size == 0, f"{what}: list {l} (n={m['n']}, P={m['precision']}) differs from the oracle's decode at {bad[:5]}"
    if nonclean:
        assert r.last_decode_nonclean == sum(not m["clean"] for m in want), what
    nl = len(want)
    req = [nl - 1, 0, nl // 2, nl - 1]
    sub, sub_off = r.decode_lists(np.array(req, dtype=np.uint64))
    sub = _u64(sub)
    assert [int(v) for v in sub_off] == [0] + list(np.cumsum([want[l]["n"] for l in req])), what
    for i, l in enumerate(req):
        assert np.array_equal(sub[int(sub_off[i]):int(sub_off[i + 1])], want[l]["order"]), f"{what}: decode_lists item {i} (list {l})"
    return dec


def _check_call(roc, monkeypatch, call, want, env, want_perm, what, imported=True):
    """one call under one mode -> what must be identical in every mode"""
    _pin(monkeypatch, env)
    off, ids = rs.concat(call["lists"])
    r = roc.encode(off, ids, precision_mode=call["precision_mode"], want_perm=want_perm)
    info, words = _check_streams(r, want, what)
    dec = _check_decode(r, want, what)
    perm = r.perm() if want_perm else np.zeros(0, np.uint32)
    if want_perm:
        for l, m in enumerate(want):  # (the permutation is the encoder's sampling order: the oracle's, lossless list or not)
            assert np.array_equal(perm[int(off[l]):int(off[l + 1])], m["perm"]), f"{what}: permutation of list {l}"
    if imported:  # the same streams imported: no maxima, the planner's own assumptions
        r2 = roc.from_streams(off, info["precision"], info["heads"], info["nwords"], words, mt_draws=info["mt_draws"])
        _check_decode(r2, want, what + " (imported)")
    return dict(heads=info["heads"], nwords=info["nwords"], precision=info["precision"], mt_draws=info["mt_draws"], words=words, dec=dec, perm=perm)


# the modes that differ for a list beyond lane_max64 = 4096 ids: the lane-per-list families never see it
LONG_MODES = ("auto", "general", "row", "old_u", "no_r2")


def _every_mode(roc, monkeypatch, modes, call, want, name, perms=(False, True)):
    """(the streams are imported once per mode: an import does not know about the permutation)"""
    first = {}
    for mode, env in modes.items():
        for want_perm in perms:
            got = _check_call(roc, monkeypatch, call, want, env, want_perm, f"{name} [{mode}, perm={want_perm}]", imported=want_perm == perms[0])
            ref = first.setdefault(want_perm, got)
            for k in got:
                assert np.array_equal(got[k], ref[k]), f"{name}: '{k}' under {mode} differs from the first mode"


def _healthy_batch(roc, oracle):
    """the context still encodes and decodes: three natural lists against the oracle"""
    lists = [rs.beside(seed=s, n=n) for s, n in ((11, 40), (12, 300), (13, 5000))]
    want = [rs.model(oracle, li) for li in lists]
    off, ids = rs.concat(lists)
    r = roc.encode(off, ids, want_perm=True)
    _check_streams(r, want, "healthy batch")
    _check_decode(r, want, "healthy batch")
    assert r.last_decode_nonclean == 0


# ----------------------------------------------------------------------------------------------------------------- the table edge
EDGE_CLASSES = ("lane64", "C1", "C2", "r2", "G3", "C3")


# (a decode of the two longest classes is a chain of 10 800 / 34 000 steps over a multiset: one mode per test, and the longest
# class in the three families that differ at its length, with the permutation only)
EDGE_OK = [(c, None) for c in ("lane64", "C1", "C2", "r2")] + [("G3", m) for m in LONG_MODES] + [("C3", m) for m in ("auto", "general", "row")]


@pytest.mark.parametrize("cls,mode", EDGE_OK, ids=[c if m is None else f"{c}-{m}" for c, m in EDGE_OK])
def test_lists_with_1023_and_1024_draws_encode_and_decode_in_every_mode(roc, monkeypatch, modes, calls, expected, cls, mode):
    name = f"edge-{cls}-ok"
    assert [m["mt_draws"] for m in expected[name]][::2] == [TABLE - 1, TABLE]
    use = modes if mode is None else {mode: modes[mode]}
    _every_mode(roc, monkeypatch, use, calls[name], expected[name], name, perms=(True,) if cls == "C3" else (False, True))


@pytest.mark.parametrize("cls", EDGE_CLASSES)
def test_a_list_with_1025_draws_is_refused_in_every_mode(roc, oracle, monkeypatch, modes, calls, expected, cls):
    """alone in its call and between healthy lists: VIDC_ERR_OVERFLOW naming the list, the same message in every mode; the context
    encodes and decodes a healthy batch afterwards"""
    Err = _error()
    for name in (f"edge-{cls}-over", f"edge-{cls}-over+"):
        call, bad = calls[name], calls[name]["fails"]
        assert expected[name][bad]["mt_draws"] == TABLE + 1 and all(m["mt_draws"] <= TABLE for l, m in enumerate(expected[name]) if l != bad)
        off, ids = rs.concat(call["lists"])
        messages = set()
        for mode, env in modes.items():
            _pin(monkeypatch, env)
            for want_perm in (False, True):
                with pytest.raises(Err) as ex:
                    roc.encode(off, ids, precision_mode=call["precision_mode"], want_perm=want_perm)
                messages.add(str(ex.value))
            _pin(monkeypatch, {})
        assert messages == {f"{OVERFLOW} roc encode: list {bad} needed more than {TABLE} mt19937 underflow words"}, (name, messages)
    for mode in ("auto", "lane", "row"):
        _pin(monkeypatch, modes[mode])
        _healthy_batch(roc, oracle)


@pytest.mark.parametrize("cls", rs.DECODE_OVER)
def test_a_decode_that_needs_the_1025th_word_is_refused_in_every_mode(roc, oracle, monkeypatch, modes, calls, expected, cls):
    """a list that encodes with exactly 1024 draws and whose decode ends with one more pop from the empty stack: the stream is the
    oracle's, decode_all and the decode of the imported stream are refused with VIDC_ERR_OVERFLOW naming the list, the healthy list
    beside it still decodes by itself"""
    Err = _error()
    name = f"edge-{cls}-decode-over"
    call, want = calls[name], expected[name]
    assert (want[1]["mt_draws"], want[1]["end_draws"]) == (TABLE, TABLE + 1) and call["decode_fails"] == 1
    off, ids = rs.concat(call["lists"])
    messages = set()
    for mode, env in modes.items():
        if want[1]["n"] > 8192 and mode not in LONG_MODES:
            continue
        _pin(monkeypatch, env)
        r = roc.encode(off, ids, precision_mode=call["precision_mode"])
        info, words = _check_streams(r, want, f"{name} [{mode}]")
        r2 = roc.from_streams(off, info["precision"], info["heads"], info["nwords"], words, mt_draws=info["mt_draws"])
        for obj in (r, r2):
            with pytest.raises(Err) as ex:
                obj.decode_all()
            messages.add(str(ex.value))
            sub, _ = obj.decode_lists(np.array([0], dtype=np.uint64))
            assert np.array_equal(_u64(sub), want[0]["order"])
    assert messages == {f"{OVERFLOW} roc decode: list 1 needed more than {TABLE} mt19937 underflow words"}, messages
    _pin(monkeypatch, {})
    _healthy_batch(roc, oracle)


def test_import_accepts_1024_draws_and_rejects_1025(roc, monkeypatch, expected):
    """vidc_roc_import: mt_draws = 1024 is a valid image (and decodes to the oracle's order); 1025 is VIDC_ERR_INVALID before any
    device work, and *out stays NULL"""
    from vector_db_id_compression_amd import _lib

    _pin(monkeypatch, {})
    want = expected["edge-C2-ok"]
    off, prec, heads, nw, words, draws = _streams_of(want)
    assert draws[2] == TABLE
    r = roc.from_streams(off, prec, heads, nw, words, mt_draws=draws)
    _check_decode(r, want, "imported oracle streams")
    ctx = _lib.default_context()
    arr = [np.ascontiguousarray(a, dtype=t) for a, t in ((off, np.uint64), (prec, np.uint32), (heads, np.uint64), (nw, np.uint32), (words, np.uint32))]
    for d2, status in ((TABLE, 0), (TABLE + 1, -1)):
        dr = np.array([draws[0], draws[1], d2], dtype=np.uint32)
        h = C.c_void_p(0xDEAD0)
        rc = _lib.lib().vidc_roc_import(ctx.h, 3, _lib.ptr(arr[0]), _lib.ptr(arr[1]), _lib.ptr(arr[2]), _lib.ptr(arr[3]), _lib.ptr(dr),
                                        _lib.ptr(arr[4]), C.byref(h))
        assert rc == status
        if status:
            assert not h.value, "*out must be NULL after a rejected import"
            assert _lib.lib().vidc_last_error().decode() == f"roc import: list 2 claims {TABLE + 1} mt19937 draws (table holds {TABLE})"
        else:
            _lib.lib().vidc_roc_destroy(h)
    with pytest.raises(_lib.VidcError, match=INVALID):
        roc.from_streams(off, prec, heads, nw, words, mt_draws=[draws[0], TABLE + 1, draws[2]])


# ------------------------------------------------------------------------------------------------- underflow below the edge, regrowth
def _names(calls, prefix):
    return sorted(k for k in calls if k.startswith(prefix))


@pytest.mark.parametrize("P", [0, 3])
def test_partial_underflow_at_both_ends_of_the_short_classes(roc, monkeypatch, modes, calls, expected, P):
    """1, 63 .. 65, 255 .. 257, 511 .. 513, 1023 .. 1025 and 2047 .. 2049 ids at P = 0 and 3: every encoder class below the edge
    draws (tiny strip, 4- / 16- / 64-word lane strips, C1, r2), every decoder class of that length regrows"""
    name = f"partial-short-P{P}"
    _every_mode(roc, monkeypatch, modes, calls[name], expected[name], name)


@pytest.mark.parametrize("bound", rs.class_bounds()[1])
def test_partial_underflow_at_the_ends_of_the_longer_classes(roc, monkeypatch, modes, calls, expected, bound):
    """bound and bound + 1 ids at the two lowest precisions that stay below the edge.  4096 / 4097 (lane classes, general small class,
    the bitmap kernels' shortest list) in every mode; 8192 / 8193 and 16 384 / 16 385 are bounds of the general and the row-per-list
    kernels only: the lower precision under those and the automatic mode, the higher one on the general kernels"""
    names = _names(calls, f"partial-long-n{bound}-")
    assert len(names) == 2
    for i, name in enumerate(names):
        use = modes if bound <= 4096 else {k: modes[k] for k in (("auto", "general", "row") if i == 0 else ("general",))}
        _every_mode(roc, monkeypatch, use, calls[name], expected[name], name, perms=(i == 0,))


def test_streams_that_grow_while_they_are_decoded(roc, monkeypatch, modes, calls, expected):
    """one ws_spill32 (30 .. 49 words of growth) and several hundred words, in the lengths of k_roc_decode_u2<18> and of the general
    decoder / k_roc_decode_b2<32 .. 256> (the permutation in the automatic mode only)"""
    names = _names(calls, "regrow-")
    assert len(names) >= 2
    for name in names:
        _every_mode(roc, monkeypatch, {"auto": modes["auto"]}, calls[name], expected[name], name)
        _every_mode(roc, monkeypatch, {k: v for k, v in modes.items() if k != "auto"}, calls[name], expected[name], name, perms=(False,))


def _import_and_decode(roc, s):
    off = np.array([0, s["n"]], dtype=np.uint64)
    return roc.from_streams(off, [s["precision"]], [s["head"]], [s["words"].size], s["words"], mt_draws=[s["mt_draws"]])


def test_regrowth_from_every_start_of_the_register_ring(roc, oracle, monkeypatch, modes):
    """the regrowth streams on top of words that are never reached, so that nwords = 0, 1, 31, 32, 33 (mod 64): imported and decoded in
    every mode, equal to the oracle's decode of the padded stream"""
    padded = rs.padded_cases(oracle)
    want = {k: oracle.roc_decode(s["head"], s["words"], s["n"], s["precision"], s["mt_draws"])[0] for k, s in padded.items()}
    for mode, env in modes.items():
        _pin(monkeypatch, env)
        for name, s in padded.items():
            assert s["words"].size % 64 == s["residue"]
            if s["n"] > 4096 and mode not in LONG_MODES:
                continue
            r = _import_and_decode(roc, s)
            dec = _u64(r.decode_all())
            bad = np.flatnonzero(dec != want[name])
            assert bad.size == 0, f"{name} [{mode}]: differs from the oracle's decode at {bad[:5]}"


def test_truncated_streams_take_every_decoder_to_the_table_edge(roc, oracle, monkeypatch, modes):
    """Imports with the bottom of the stream cut off make the DECODER draw, at a pushed depth of one or two: the only way to the
    draw path of k_roc_decode_u2<20> and k_roc_decode_b2 (no list makes them draw), and -- with a claimed mt_draws near the end
    of the table -- the only way for the lane- and row-per-list decoders and the tiny strip to meet the table's end themselves,
    not through the retry pass.  A decode that ends at 1024 draws equals the oracle's in every mode, one at 1025 is refused."""
    Err = _error()
    cases = rs.truncated_cases(oracle)
    want = {k: oracle.roc_decode(s["head"], s["words"], s["n"], s["precision"], s["mt_draws"])[0] for k, s in cases.items()}
    messages, problems = set(), []
    for mode, env in modes.items():
        _pin(monkeypatch, env)
        for name, s in cases.items():
            if s["n"] > 4096 and mode not in LONG_MODES:
                continue
            r = _import_and_decode(roc, s)
            if s["end_draws"] > TABLE:
                try:
                    r.decode_all()
                    problems.append(f"{name} [{mode}]: a decode that needs {s['end_draws']} table words was not refused")
                except Err as ex:
                    messages.add(str(ex))
                continue
            bad = np.flatnonzero(_u64(r.decode_all()) != want[name])
            if bad.size:
                problems.append(f"{name} [{mode}]: differs from the oracle's decode at {bad[:5]}")
            if r.last_decode_handed_back:
                problems.append(f"{name} [{mode}]: handed back")
    assert not problems, problems
    assert messages == {f"{OVERFLOW} roc decode: list 0 needed more than {TABLE} mt19937 underflow words"}, messages


# ------------------------------------------------------------------------------------------------------------------ pushed depth
LANE_MODES = {"lane": {}, "lane_pair": {}, "lane_quad": {}, "lane_old": {}, "lane_rows_only": {"VIDC_FORCE_LANE": "1", "VIDC_NO_LANE_REG": "1", "VIDC_NO_LANE_PAIR": "1"},
              "lane_no128_align4": {"VIDC_FORCE_LANE": "1", "VIDC_NO_LANE128": "1", "VIDC_LANE_ALIGN": "4"}}


def _depth_check(roc, monkeypatch, call, want, env, what):
    """-> (handed back by decode_all, by decode_lists of the depth-9 lists, by decode_lists of the others)"""
    _pin(monkeypatch, env)
    off, ids = rs.concat(call["lists"])
    r = roc.encode(off, ids, precision_mode=call["precision_mode"], want_perm=True)
    _check_streams(r, want, what)
    dec = _u64(r.decode_all())
    back_all, nonclean = r.last_decode_handed_back, r.last_decode_nonclean
    for l, m in enumerate(want):
        a = int(off[l])
        assert np.array_equal(dec[a:a + m["n"]], m["order"]), f"{what}: list {l} ({call['tags'][l]})"
    assert nonclean == sum(not m["clean"] for m in want), what
    deep = [l for l, t in enumerate(call["tags"]) if t.endswith("depth9")]
    rest = [l for l in range(len(want)) if l not in deep]
    out = [back_all]
    for req in (deep[::-1], rest[::-1]):
        sub, sub_off = r.decode_lists(np.array(req, dtype=np.uint64))
        sub = _u64(sub)
        out.append(r.last_decode_handed_back)
        for i, l in enumerate(req):
            assert np.array_equal(sub[int(sub_off[i]):int(sub_off[i + 1])], want[l]["order"]), f"{what}: decode_lists, list {l}"
    return tuple(out)


def test_lane_decoders_hand_back_at_a_pushed_depth_of_9_and_not_at_8(roc, monkeypatch, modes, calls, expected):
    """register / pair / quad / bucket-row decoders (64, 128, 256 buckets, both row alignments): the five lists whose decode holds 9
    pushed words at once come back through the retry pass, the five that hold exactly 8 and the natural list do not; all decode to the
    oracle's order"""
    call, want = calls["depth-lane"], expected["depth-lane"]
    ndeep = sum(t.endswith("depth9") for t in call["tags"])
    assert ndeep == 5 and [m["depth"] for t, m in zip(call["tags"], want) if t != "beside"] == [8, 9] * 5
    for mode, extra in LANE_MODES.items():
        env = dict(modes.get(mode, {}), **extra)
        assert env.get("VIDC_FORCE_LANE") == "1"
        assert _depth_check(roc, monkeypatch, call, want, env, f"depth-lane [{mode}]") == (ndeep, ndeep, 0), mode
    # the wave-per-list kernels have no such limit
    for mode in ("wave", "general", "auto"):
        assert _depth_check(roc, monkeypatch, call, want, modes[mode], f"depth-lane [{mode}]")[0] == 0


def test_row_decoders_hand_back_at_a_pushed_depth_of_9_and_not_at_8(roc, monkeypatch, modes, calls, expected):
    """row-per-list decoder with 2^8 (up to 2048 ids), 2^10 and 2^11 buckets"""
    call, want = calls["depth-grp"], expected["depth-grp"]
    ndeep = sum(t.endswith("depth9") for t in call["tags"])
    assert ndeep == 6
    assert _depth_check(roc, monkeypatch, call, want, modes["row"], "depth-grp [row]") == (ndeep, ndeep, 0)
    assert _depth_check(roc, monkeypatch, call, want, modes["general"], "depth-grp [general]")[0] == 0


# ----------------------------------------------------------------------------------------------- full precision, multisets, graph rows
def test_full_precision(roc, monkeypatch, modes, calls, expected):
    """P = 32: 1, 63 and 64 ids on the tiny strip (64 ids: more words than its window), one list per general class"""
    _every_mode(roc, monkeypatch, modes, calls["full-P32"], expected["full-P32"], "full-P32")


def test_natural_precision_multisets_under_and_over_the_edge(roc, oracle, monkeypatch, modes, calls, expected):
    """thousands of duplicates of the ids 0 .. 3 under the reference precision (2): 731 draws encode and decode everywhere, 1025
    are refused everywhere"""
    Err = _error()
    _every_mode(roc, monkeypatch, modes, calls["multiset-under"], expected["multiset-under"], "multiset-under")
    call = calls["multiset-over"]
    off, ids = rs.concat(call["lists"])
    messages = set()
    for mode, env in modes.items():
        _pin(monkeypatch, env)
        with pytest.raises(Err) as ex:
            roc.encode(off, ids, precision_mode=-1, want_perm=mode == "auto")
        messages.add(str(ex.value))
    assert messages == {f"{OVERFLOW} roc encode: list 1 needed more than {TABLE} mt19937 underflow words"}, messages
    _pin(monkeypatch, {})
    _healthy_batch(roc, oracle)


@pytest.mark.parametrize("P", [32, 0])
def test_graph_rows_at_full_and_at_zero_precision(roc, oracle, monkeypatch, modes, P):
    """96 rows of K = 64 through encode_rows(precision_mode=P): streams and decode_rows equal the oracle's, row by row, on the
    lane-per-row and on the wave-per-row kernels (P = 0: every row of two or more edges draws)"""
    rows = rs.graph_rows()
    N, K = rows.shape
    deg = (rows >= 0).sum(axis=1)
    want = [rs.model(oracle, rows[i, :deg[i]].astype(np.uint64), P) for i in range(N)]
    assert (sum(m["mt_draws"] for m in want) > 0) == (P == 0)
    for mode in ("auto", "lane", "wave", "general"):
        _pin(monkeypatch, modes[mode])
        rg = roc.encode_rows(rows, precision_mode=P)
        _check_streams(rg, want, f"rows P={P} [{mode}]")
        for nodes in (np.arange(N), np.array([2, 95, 0, 2, 50])):
            out, cnt = rg.decode_rows(nodes)
            out = out.cpu().numpy()
            for j, i in enumerate(nodes):
                d = int(deg[i])
                assert cnt[j] == d and np.array_equal(out[j, :d].astype(np.uint64), want[i]["order"]) and np.all(out[j, d:] == -1), (mode, i)


# ------------------------------------------------------------------------------------------------------------------------ append
def test_append_up_to_the_edge_and_one_id_beyond(roc, oracle, monkeypatch, modes):
    """an object encoded at precision 4 whose list draws 800 words; a batch that makes the merged list draw exactly 1024 gives the
    from-scratch encode of the merged list (the oracle's stream), one more id is VIDC_ERR_OVERFLOW and leaves the old object as it was"""
    from test_gpu_append import dev, dev_i64, roc_image, same
    import torch

    Err = _error()
    a = rs.append_case(oracle)
    P, k = a["P"], a["k_ok"]
    off, ids = rs.concat(a["old"])
    want_old = [rs.model(oracle, li, P) for li in a["old"]]
    for mode in ("auto", "general", "lane", "row"):
        _pin(monkeypatch, modes[mode])
        old = roc.encode(off, dev(ids), precision_mode=P, want_perm=True)
        _check_streams(old, want_old, f"append [{mode}]: old object")
        before = roc_image(old, True)
        old_dec = _u64(old.decode_all())
        ln = np.zeros(k + 1, dtype=np.int64)
        m = ar.merge(old.offsets, old_dec, ln[:k], a["add"][:k])
        want_new = [rs.model(oracle, m.ids[int(m.offsets[l]):int(m.offsets[l + 1])], P) for l in range(2)]
        assert want_new[0]["mt_draws"] == TABLE and want_new[0]["n"] == want_old[0]["n"] + k
        inv = torch.zeros(1, dtype=torch.int64, device="cuda")
        new, lab = old.append(dev_i64(ln[:k]), dev(a["add"][:k]), precision_mode=P, want_perm=True, invalid=inv)
        scratch = roc.encode(m.offsets, dev(m.ids), precision_mode=P, want_perm=True)
        same(roc_image(new, True), roc_image(scratch, True), f"append [{mode}]")
        _check_streams(new, want_new, f"append [{mode}]: new object")
        assert int(inv.item()) == 0
        # labels: batch entry i sits where the sampling order puts position |old| + i of the merged list
        where = np.empty(want_new[0]["n"], np.int64)
        where[want_new[0]["perm"].astype(np.int64)] = np.arange(want_new[0]["n"])
        assert np.array_equal(lab.cpu().numpy(), where[want_old[0]["n"]:])
        if a["new_decode_refused"]:
            with pytest.raises(Err, match=OVERFLOW):
                new.decode_all()
        else:
            _check_decode(new, want_new, f"append [{mode}]: new object")
        with pytest.raises(Err) as ex:
            old.append(dev_i64(ln), dev(a["add"]), precision_mode=P, want_perm=True)
        assert OVERFLOW in str(ex.value) and f"needed more than {TABLE} mt19937 underflow words" in str(ex.value)
        same(roc_image(old, True), before, f"append [{mode}]: the old object changed")
        assert np.array_equal(_u64(old.decode_all()), old_dec)
