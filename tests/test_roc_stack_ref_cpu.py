"""tests/roc_stack_ref.py (the lists that drive the ROC kernels' ANS stacks through underflow, regrowth and the 1024-draw edge) against
the CPU oracle and the headers: no GPU.  Every condition tests/test_gpu_roc_stack.py rests on is asserted here; a search that finds
nothing raises roc_stack_ref.SearchFailed, which fails the test."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import roc_stack_ref as rs

TABLE = rs.limits()["VIDC_MT_TABLE"]


# ---- the oracle's new figures against a decoder written out in Python
def _py_decode(head, words, n, P, draws, mt):
    """codec.cpp:140-152 with the reference's stack (codec.h:20-40) -> (ids, peak, most words above the running minimum, final size, draws)"""
    L = 1 << 31
    stack = [int(w) for w in words]
    peak = low = len(stack)
    depth = 0

    def pop():
        nonlocal draws, low
        if not stack:
            draws += 1
            return int(mt[draws - 1])
        w = stack.pop()
        low = min(low, len(stack))
        return w

    def push(w):
        nonlocal peak, depth
        stack.append(w & 0xFFFFFFFF)
        peak = max(peak, len(stack))
        depth = max(depth, len(stack) - low)

    seen, out = [], []
    for i in range(n):
        x = 0
        for lower in (48, 32, 16, 0):
            p = min(max(P - lower, 0), 16)
            x = (x << 16) | (head & ((1 << p) - 1))
            head >>= p
            if head < L:
                head = (head << 32) | pop()
        rank = sum(1 for y in seen if y < x)
        seen.append(x)
        nmax = i + 1
        if head >= ((L // nmax) << 32):
            push(head)
            head >>= 32
        head = head * nmax + rank
        if head < L:
            head = pop() | (head << 32)
        out.append(x)
    return np.array(out[::-1], dtype=np.uint64), peak, depth, len(stack), draws


@pytest.mark.parametrize("n,P,ubits", [(64, 0, 13), (200, 3, 13), (300, 5, 13), (250, 8, 8), (300, 32, 31), (1, 0, 5)])
def test_stack_figures_of_the_oracle_equal_a_python_decoder(oracle, n, P, ubits):
    """Oracle.roc_decode_stats: peak, pushed depth, final stack and draws equal a step-by-step Python decoder with a Python list as
    its stack; the plain entry points return what they returned before."""
    ids = np.sort(np.random.default_rng([n, P]).choice(1 << ubits, size=n, replace=False)).astype(np.uint64)
    e, e2 = oracle.roc_encode(ids, P, stats=True), oracle.roc_encode(ids, P)
    assert "stack" not in e2 and all(np.array_equal(e[k], e2[k]) for k in e2)
    plain = oracle.roc_decode(e["head"], e["words"], n, P, e["mt_draws"])
    got = oracle.roc_decode_stats(e["head"], e["words"], n, P, e["mt_draws"])
    assert len(plain) == 4 and len(got) == 5
    assert np.array_equal(plain[0], got[0]) and plain[1] == got[1] and np.array_equal(plain[2], got[2]) and plain[3] == got[3]
    ids_py, peak, depth, final, draws = _py_decode(e["head"], e["words"], n, P, e["mt_draws"], oracle.mt_table(4096))
    assert np.array_equal(ids_py, got[0])
    assert (got[4]["peak"], got[4]["depth"], got[2].size, got[3]) == (peak, depth, final, draws)
    # the encoder's figures: the peak is at least the stream, a natural list never pops far past its freshest pushes
    assert e["stack"]["peak"] >= e["words"].size and e["stack"]["pushes"] - e["stack"]["pops"] == e["words"].size


def test_natural_lists_stay_out_of_the_regime(oracle):
    """what the issue starts from: with the natural precision and distinct ids a list draws at most a few words and its decoder
    holds one or two pushed words"""
    rng = np.random.default_rng(1)
    for n, bits in ((100, 20), (1000, 20), (5000, 24), (40000, 31)):
        ids = np.sort(rng.choice(1 << bits, size=n, replace=False)).astype(np.uint64)
        m = rs.model(oracle, ids)
        assert m["mt_draws"] <= 3 and m["depth"] <= 2 and m["lossless"] and m["clean"] and m["growth"] < 0


def test_bounds_come_from_the_headers(tmp_path):
    """limits() reads csrc/; dec_stack_cap restates roc_sizing.h (checked by compiling the header where g++ exists, by its text
    otherwise); the bounds the families assume to coincide do"""
    L = rs.limits()
    assert L["VIDC_MT_TABLE"] == 1024 and L["VIDC_DPST"] == L["VIDC_GRP_DPST"] == 8
    assert L["GEN_SMALL_MAX"] == L["VIDC_LANE_MAX64"] == L["ENC_C1_MAX"] == L["U_MIN_LIST"] - 1
    assert L["VIDC_LANE_QUAD_MAX"] == L["VIDC_LANE_MAX"] and L["DEC_G8K_MAX"] == L["VIDC_GRP_LEV2_MAX"]
    cases = [(n, w) for n in (1, 64, 100, 4097, 34093, 262144) for w in (0, 1, 500, 400000)]
    gxx = shutil.which("g++")
    if gxx is not None:
        src = tmp_path / "cap.cpp"
        src.write_text('#include <cstdio>\n#include "roc_sizing.h"\nint main() { unsigned n, w; while (scanf("%u %u", &n, &w) == 2) '
                       'printf("%u\\n", vidc::dev::roc_dec_stack_cap(n, w)); }\n')
        exe = str(tmp_path / "cap")
        subprocess.check_call([gxx, "-std=c++17", "-I", rs.CSRC, "-o", exe, str(src)])
        out = subprocess.run([exe], input="".join("%d %d\n" % c for c in cases), capture_output=True, text=True, check=True)
        assert [int(v) for v in out.stdout.split()] == [rs.dec_stack_cap(n, w) for n, w in cases]
    else:
        text = open(os.path.join(rs.CSRC, "roc_sizing.h")).read()
        assert "(uint32_t)(((uint64_t)n * 37ull) >> 5) + 8u" in text and "return (a > W ? a : W) + 64u;" in text
    assert "n * 37 / 32 + 8" in open(os.path.join(rs.CSRC, "roc.hip")).read()  # arena_words_for


# ---- the families
@pytest.fixture(scope="module")
def calls(oracle):
    return rs.all_calls(oracle)


@pytest.fixture(scope="module")
def expected(oracle, calls):
    return {name: rs.expect(oracle, c) for name, c in calls.items()}


def test_every_list_stays_inside_its_arena_and_its_decoder_scratch(calls, expected):
    """no case expects the arena-overflow status: every stream is shorter than the encoder's arena, the encoder's stack never
    exceeds it, every decode stack peaks below roc_dec_stack_cap; a list that is not marked as refused stays inside the table
    through its decode"""
    assert len(calls) >= 30
    for name, c in calls.items():
        for l, m in enumerate(expected[name]):
            assert m["nwords"] < rs.arena_words(m["n"]) and m["enc_peak"] < rs.arena_words(m["n"]), (name, l)
            assert m["peak"] < rs.dec_stack_cap(m["n"], m["nwords"]), (name, l)
            assert m["n"] <= 40000
            if c.get("fails") == l:
                assert m["refused"]
            elif c.get("decode_fails") == l:
                assert not m["refused"] and m["decode_refused"]
            else:
                assert not m["refused"] and not m["decode_refused"], (name, l)
        assert len(c["lists"]) <= 24


def test_edge_lists_draw_exactly_1023_1024_and_1025_words(oracle, calls, expected):
    L = rs.limits()
    classes = rs.edge_classes(oracle)
    assert set(classes) == {"lane64", "C1", "C2", "r2", "G3", "C3"}
    for cls, (P, ubits, lo, hi) in classes.items():
        ok, over, plus = (expected[f"edge-{cls}-{k}"] for k in ("ok", "over", "over+"))
        assert [m["mt_draws"] for m in ok] == [TABLE - 1, ok[1]["mt_draws"], TABLE] and ok[1]["mt_draws"] < 32
        assert [m["mt_draws"] for m in over] == [TABLE + 1]
        assert [m["mt_draws"] for m in plus] == [ok[1]["mt_draws"], TABLE + 1, TABLE]
        assert ok[2]["end_draws"] == TABLE and ok[0]["end_draws"] <= TABLE  # their decodes draw nothing beyond the table
        for m in ok[::2] + over:
            assert lo <= m["n"] <= hi and m["precision"] == P
        assert calls[f"edge-{cls}-over"]["fails"] == 0 and calls[f"edge-{cls}-over+"]["fails"] == 1
    # the classes are the ones they are named after
    n = {cls: expected[f"edge-{cls}-ok"][2]["n"] for cls in classes}
    assert L["VIDC_LANE_MAX"] < n["lane64"] <= L["VIDC_LANE_MAX64"] and n["C1"] <= L["ENC_C1_MAX"]
    assert L["ENC_C1_MAX"] < n["C2"] <= min(L["ENC_C2_MAX"], L["VIDC_GRP_LEV2_MAX"]) and L["VIDC_GRP_LEV2_MAX"] < n["G3"] <= L["ENC_C2_MAX"]
    assert n["C3"] > L["ENC_C2_MAX"] and n["r2"] >= L["U_MIN_LIST"]
    assert int(calls["edge-r2-ok"]["lists"][2].max()) >= 1 << 20 and int(calls["edge-C2-ok"]["lists"][2].max()) < 1 << 18
    for cls in rs.DECODE_OVER:
        m = expected[f"edge-{cls}-decode-over"][1]
        assert (m["mt_draws"], m["end_draws"]) == (TABLE, TABLE + 1)


def test_short_classes_underflow_at_both_ends(calls, expected):
    short, longer = rs.class_bounds()
    assert short == [64, 256, 512, 1024, 2048] and longer == [4096, 8192, 16384]
    for P in (0, 3):
        c, ex = calls[f"partial-short-P{P}"], expected[f"partial-short-P{P}"]
        assert [m["n"] for m in ex[:-1]] == sorted({1} | {b + d for b in short for d in (-1, 0, 1)})
        for m in ex[1:-1]:
            assert 0 < m["mt_draws"] < TABLE and m["growth"] > 0 and m["precision"] == P
        assert all(m["nwords"] == 0 for m in ex) if P == 0 else True
    for b in longer:
        names = [k for k in calls if k.startswith(f"partial-long-n{b}-")]
        assert len(names) == 2
        for k in names:
            assert [m["n"] for m in expected[k]] == [b, 100, b + 1]
            assert all(300 < m["mt_draws"] <= TABLE - 40 for m in expected[k][::2])


def test_depth_lists_reach_exactly_8_and_9(oracle, calls, expected):
    """... under their natural precision, without filling a member row of any decoder that can take them"""
    classes = rs.depth_classes()
    for name in ("depth-lane", "depth-grp"):
        c, ex = calls[name], expected[name]
        assert c["precision_mode"] == -1
        for li, tag, m in zip(c["lists"], c["tags"], ex):
            if tag == "beside":
                assert m["depth"] <= 2 and m["clean"] and m["lossless"] and m["n"] == 100
                continue
            cls, d = tag.split("-depth")
            lo, hi, kinds = classes[cls]
            assert m["depth"] == int(d) and lo <= m["n"] <= hi and m["precision"] == oracle.list_precision(li)
            assert not rs.overflows_a_row(m, kinds) and m["mt_draws"] < 64
        depths = [m["depth"] for t, m in zip(c["tags"], ex) if t != "beside"]
        assert depths == [8, 9] * (len(depths) // 2)
    assert {t.split("-")[0] for t in calls["depth-lane"]["tags"]} == {"reg", "pair", "quad", "rows128", "rows256", "beside"}
    assert {"grpF2", "grpF3"} <= {t.split("-")[0] for t in calls["depth-grp"]["tags"]}


def test_regrowth_lists_and_their_padded_streams(oracle, calls, expected):
    L = rs.limits()
    seen = {}
    for name in calls:
        if name.startswith("regrow-"):
            for tag, m in zip(calls[name]["tags"], expected[name]):
                seen[tag] = m
    assert 30 <= seen["U18-spill"]["growth"] <= 49 and 30 <= seen["gen-spill"]["growth"] <= 49  # more than 24: one ws_spill32
    assert seen["U18-deep"]["growth"] >= 500 and seen["gen-deep"]["growth"] >= 200
    for tag in ("U18-spill", "U18-deep"):
        assert seen[tag]["n"] >= L["U_MIN_LIST"] and seen[tag]["precision"] <= 18
    for tag in ("gen-spill", "gen-deep"):
        assert L["TINY_MAX"] < seen[tag]["n"] <= L["GEN_SMALL_MAX"] and seen[tag]["precision"] >= 7
    padded = rs.padded_cases(oracle)
    assert len(padded) == 4 * len(rs.REGROW_RESIDUES)
    for name, s in padded.items():
        assert s["words"].size % 64 == s["residue"] and s["words"].size > 0
        order, end_head, end_words, end_draws, st = oracle.roc_decode_stats(s["head"], s["words"], s["n"], s["precision"], s["mt_draws"])
        assert end_words.size - s["words"].size == s["growth"] and s["base_growth"] - 1 <= s["growth"] <= s["base_growth"] and end_draws <= TABLE
        assert st["peak"] < rs.dec_stack_cap(s["n"], s["words"].size)
        tag = name[len("padded-"):name.index("-mod64")]
        assert np.array_equal(order, seen[tag]["order"])  # the words below are never reached
        assert st["min_sp"] >= s["words"].size - seen[tag]["nwords"] - 1


def test_full_precision_and_multisets(oracle, calls, expected):
    L = rs.limits()
    ex = expected["full-P32"]
    assert [m["n"] for m in ex][:3] == [1, 63, 64] and all(m["precision"] == 32 and m["lossless"] and m["clean"] for m in ex)
    assert ex[2]["nwords"] > L["VIDC_TINY_STRIP"] and ex[2]["nwords"] <= 2 * L["VIDC_TINY_STRIP"] - 2  # beyond the window, inside its reach
    assert ex[3]["n"] <= L["ENC_C1_MAX"] < ex[4]["n"] <= L["ENC_C2_MAX"] < ex[5]["n"]
    under, over = expected["multiset-under"][0], expected["multiset-over"][1]
    assert under["precision"] == over["precision"] == 2 and 500 < under["mt_draws"] < TABLE and over["mt_draws"] == TABLE + 1
    assert int(calls["multiset-over"]["lists"][1].max()) == 3
    rows = rs.graph_rows()
    deg = (rows >= 0).sum(axis=1)
    assert rows.shape == (96, 64) and deg[:3].tolist() == [0, 1, 64] and deg.max() == 64
    for i in (1, 2, 50):  # P = 0 on a row draws, P = 32 does not
        li = rows[i, :deg[i]].astype(np.uint64)
        assert rs.model(oracle, li, 0)["mt_draws"] == (0 if deg[i] < 2 else rs.model(oracle, li, 0)["end_nwords"])
        assert rs.model(oracle, li, 32)["mt_draws"] == 0


def test_truncated_streams_make_the_decoder_draw(oracle):
    """per class one import that ends at exactly 1024 draws and one at 1025, at a pushed depth the 8-deep stacks hold, inside the
    decoder's scratch; the tiny one needs more words than its strip's window"""
    L = rs.limits()
    cases = rs.truncated_cases(oracle)
    assert len(cases) == 2 * len(rs.TRUNCATED) + 5
    for cls, n, P in rs.TRUNCATED:
        a, b = cases[f"truncated-{cls}-end{TABLE}"], cases[f"truncated-{cls}-end{TABLE + 1}"]
        assert (a["end_draws"], b["end_draws"]) == (TABLE, TABLE + 1) and a["mt_draws"] < TABLE and b["mt_draws"] <= TABLE
        for s in (a, b):
            got = oracle.roc_decode_stats(s["head"], s["words"], n, P, s["mt_draws"])
            assert got[3] == s["end_draws"] and got[4]["depth"] == s["depth"] <= 4 and got[4]["peak"] < rs.dec_stack_cap(n, s["words"].size)
            assert s["end_draws"] - s["mt_draws"] >= 16  # the decoder itself draws
    assert cases[f"truncated-tiny-end{TABLE}"]["words"].size <= L["VIDC_TINY_STRIP"] and cases["truncated-tiny-end1024"]["n"] == L["TINY_MAX"]
    for cls in ("U20-P19", "U20-P20", "b2"):
        s = cases[f"truncated-{cls}-from0"]
        assert s["mt_draws"] == 0 and 280 <= s["end_draws"] <= 320 and s["n"] >= L["U_MIN_LIST"]


def test_append_batch_takes_a_list_to_the_edge_and_one_id_beyond(oracle):
    a = rs.append_case(oracle)
    P, old, add, k = a["P"], a["old"][0], a["add"], a["k_ok"]
    assert add.size == k + 1 and 700 < a["old_model"]["mt_draws"] < 900 and not a["old_model"]["decode_refused"]
    merged = np.concatenate([a["old_model"]["order"], add])  # what the old object decodes to, then the batch
    assert rs.draws_of(oracle, merged[:-1], P) == TABLE and rs.draws_of(oracle, merged, P) == TABLE + 1
    assert rs.model(oracle, merged[:-1], P)["decode_refused"] == a["new_decode_refused"]
    small = rs.model(oracle, a["old"][1], P)
    assert small["lossless"] and small["clean"] and np.array_equal(rs.model(oracle, small["order"], P)["words"], small["words"])
