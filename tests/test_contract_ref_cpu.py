"""The reference and the guard helpers of tests/contract_ref.py, pinned on the CPU: hand-written rows and lists for every kind, the
rule for nodes outside the object, and the guards seeing a single element written outside a view or left unwritten inside it."""
import numpy as np
import pytest

import contract_ref as cr


def _rows(lists, K):
    rows = np.full((len(lists), K), -1, np.int32)
    for i, l in enumerate(lists):
        rows[i, : len(l)] = l
    return rows


ROWS = _rows([[7, 2, 9], [], [5, 1, 4, 3], [6], [0, 11, 10, 8]], 4)


def test_poison_values():
    assert cr.POISON32 < 0 and cr.POISON32 != -1 and cr.POISON32 == -0x5A5A5A5B
    assert cr.POISON64 == 0xA5A5A5A5A5A5A5A5 and cr.POISON64 >= 1 << 63
    assert cr.GUARD_BYTES >= 4096


def test_expected_rows_compact_keeps_input_order():
    out, cnt = cr.expected_rows("compact", ROWS, None, 4)
    assert out.dtype == np.int32 and out.shape == (5, 4)
    assert out.tolist() == [[7, 2, 9, -1], [-1, -1, -1, -1], [5, 1, 4, 3], [6, -1, -1, -1], [0, 11, 10, 8]]
    assert cnt.tolist() == [3, 0, 4, 1, 4]


def test_expected_rows_ef_is_ascending_and_pads_to_a_wider_k():
    out, cnt = cr.expected_rows("ef", ROWS, None, 6)
    assert out.tolist() == [[2, 7, 9, -1, -1, -1], [-1] * 6, [1, 3, 4, 5, -1, -1], [6, -1, -1, -1, -1, -1], [0, 8, 10, 11, -1, -1]]
    assert cnt.tolist() == [3, 0, 4, 1, 4]


def test_expected_rows_roc_is_the_oracle_round_trip(oracle):
    out, cnt = cr.expected_rows("roc", ROWS, None, 5, oracle)
    assert cnt.tolist() == [3, 0, 4, 1, 4]
    assert (out[:, 4] == -1).all() and (out[1] == -1).all() and out[3].tolist() == [6, -1, -1, -1, -1]
    for i in (0, 2, 4):  # maxima 9, 5, 11: not powers of two, so the codec is lossless and returns the set in its own order
        ids = np.sort(ROWS[i][ROWS[i] >= 0]).astype(np.uint64)
        n = ids.size
        assert sorted(out[i, :n].tolist()) == ids.tolist() and (out[i, n:] == -1).all()
        prec = oracle.list_precision(ids)
        e = oracle.roc_encode(ids, prec)
        assert out[i, :n].tolist() == oracle.roc_decode(e["head"], e["words"], n, prec, e["mt_draws"])[0].tolist()


def test_expected_rows_roc_keeps_the_power_of_two_quirk_in_the_comparison(oracle):
    """a row whose maximum is a power of two is not left out: the expectation is the reference codec's own (lossy) answer"""
    rows = _rows([[3, 8, 5], [16, 2]], 3)
    out, cnt = cr.expected_rows("roc", rows, None, 3, oracle)
    assert cnt.tolist() == [3, 2]
    for i, ids in enumerate(([3, 5, 8], [2, 16])):
        ids = np.asarray(ids, np.uint64)
        prec = oracle.list_precision(ids)
        e = oracle.roc_encode(ids, prec)
        ref = oracle.roc_decode(e["head"], e["words"], ids.size, prec, e["mt_draws"])[0]
        assert out[i, : ids.size].tolist() == ref.tolist()
        assert (out[i, : ids.size] >= 0).all() and (out[i, ids.size:] == -1).all()


@pytest.mark.parametrize("kind", ["compact", "ef", "roc"])
def test_nodes_outside_the_object_give_minus_one_rows(kind, oracle):
    nodes = np.array([2, -1, 5, 0, 2, -(1 << 40), 1 << 33, 4], np.int64)  # repeats, negatives, >= N
    out, cnt = cr.expected_rows(kind, ROWS, nodes, 7, oracle)
    every, every_cnt = cr.expected_rows(kind, ROWS, None, 7, oracle)
    assert out.shape == (8, 7)
    for i, v in enumerate(nodes):
        if 0 <= v < 5:
            assert out[i].tolist() == every[v].tolist() and cnt[i] == every_cnt[v]
        else:
            assert (out[i] == -1).all() and cnt[i] == 0
    assert np.array_equal(out[0], out[4])


def test_expected_lists_orders(oracle):
    off = np.array([0, 3, 3, 7, 8], np.uint64)
    ids = np.array([7, 2, 9, 5, 1, 4, 3, 6], np.uint64)
    flat, oo = cr.expected_lists("packed", off, ids, None)
    assert flat.dtype == np.uint64 and flat.tolist() == ids.tolist() and oo.tolist() == [0, 3, 3, 7, 8]
    for kind in ("ef", "wt"):
        flat, oo = cr.expected_lists(kind, off, ids, None)
        assert flat.tolist() == [2, 7, 9, 1, 3, 4, 5, 6] and oo.tolist() == [0, 3, 3, 7, 8]
    flat, oo = cr.expected_lists("ef", off, ids, [2, 1, 0, 2, 3])  # a selection with a repeat and an empty list
    assert flat.tolist() == [1, 3, 4, 5, 2, 7, 9, 1, 3, 4, 5, 6] and oo.tolist() == [0, 4, 4, 7, 11, 12]
    flat, oo = cr.expected_lists("packed", off, ids, [])
    assert flat.size == 0 and oo.tolist() == [0]
    flat, oo = cr.expected_lists("roc", off, ids, None, oracle)
    assert oo.tolist() == [0, 3, 3, 7, 8]
    for a, b in ((0, 3), (3, 7), (7, 8)):
        s = np.sort(ids[a:b])
        prec = oracle.list_precision(s)
        e = oracle.roc_encode(s, prec)
        assert flat[a:b].tolist() == oracle.roc_decode(e["head"], e["words"], s.size, prec, e["mt_draws"])[0].tolist()
        assert sorted(flat[a:b].tolist()) == s.tolist()  # (maxima 9, 5, 6: lossless)
    ref = cr.ListRef("ef", off, ids)
    assert ref.item(2, 1) == 3 and ref.item(0, 2) == 9


@pytest.mark.parametrize("dtype", [np.int32, np.uint32, np.int64, np.uint64])
@pytest.mark.parametrize("misalign", [0, 1, 2, 3])
def test_guarded_layout(dtype, misalign):
    isz = np.dtype(dtype).itemsize
    whole, view = cr.guarded((5, 7), dtype, "cpu", None, misalign)
    assert view.shape == (5, 7) and view.dtype == np.dtype(dtype) and view.flags["C_CONTIGUOUS"]
    start = (view.ctypes.data - whole.ctypes.data) // isz
    assert start * isz >= cr.GUARD_BYTES and (whole.size - start - 35) * isz >= cr.GUARD_BYTES
    assert whole.ctypes.data % 16 == 0 and view.ctypes.data % 16 == (misalign * isz) % 16
    poison = 0xA5A5A5A5 if isz == 4 else 0xA5A5A5A5A5A5A5A5
    assert (whole.view(np.uint32 if isz == 4 else np.uint64) == poison).all()
    cr.assert_guards_intact(whole, view)
    cr.assert_untouched(whole, view)
    view[:] = 1  # the payload is the caller's to write
    cr.assert_guards_intact(whole, view)
    with pytest.raises(AssertionError):
        cr.assert_untouched(whole, view)
    with pytest.raises(AssertionError):
        cr.guarded(4, dtype, "cpu", 8)  # a guard below 4 KiB is refused


@pytest.mark.parametrize("dtype", [np.int32, np.uint64])
def test_guards_see_one_element_outside_the_view(dtype):
    isz = np.dtype(dtype).itemsize
    for side in ("behind", "before"):
        whole, view = cr.guarded((3, 4), dtype, "cpu", None, 1)
        view[:] = 5
        start = (view.ctypes.data - whole.ctypes.data) // isz
        whole[start + 12 if side == "behind" else start - 1] = 5  # one element past the last / in front of the first
        with pytest.raises(AssertionError, match=side):
            cr.assert_guards_intact(whole, view)
    whole, view = cr.guarded(12, dtype, "cpu")
    whole[-1] = 0  # the far end of the guard counts as well
    with pytest.raises(AssertionError):
        cr.assert_guards_intact(whole, view)
    whole, view = cr.guarded(12, dtype, "cpu")
    whole[0] = 0
    with pytest.raises(AssertionError):
        cr.assert_guards_intact(whole, view)


@pytest.mark.parametrize("dtype", [np.int32, np.uint64])
def test_a_write_one_element_short_is_seen(dtype):
    whole, view = cr.guarded((3, 4), dtype, "cpu")
    want = np.arange(12, dtype=dtype).reshape(3, 4)
    view.reshape(-1)[:11] = want.reshape(-1)[:11]  # the writer stops one element early
    cr.assert_guards_intact(whole, view)
    with pytest.raises(AssertionError, match="never written"):
        cr.assert_view_equals(view, want)
    view[2, 3] = 11
    cr.assert_view_equals(view, want)
    cr.assert_guards_intact(whole, view)
    view[0, 0] = 99
    with pytest.raises(AssertionError, match="first at flat index 0"):
        cr.assert_view_equals(view, want)
    with pytest.raises(AssertionError):
        cr.assert_view_equals(view, want[:2])  # a shorter expectation is not "the whole view"


def test_the_module_never_imports_the_product_package():
    import ast
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(cr.__file__)), "contract_ref.py")) as f:
        tree = ast.parse(f.read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names.update(a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert names <= {"numpy", "torch"}, names
