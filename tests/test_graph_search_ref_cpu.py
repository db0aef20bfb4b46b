"""CPU: the numpy model of the one-launch graph search (tests/graph_search_ref.py) against graph_search.search on the shared shapes; the
shapes hold what the GPU tests use them for; csrc/graph_search_ref.h + graph_search_plan.h built with g++ as a stand-alone program
(tests/graph_search_test.cpp), plain and with -fsanitize=address,undefined, against cases the model writes out; the one-CU batch of
the GPU test gives every slot at least three queries with a ragged last trip, by the plan header's own figures."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import graph_search_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_CU_NQ = 101  # the batch of the one-CU GPU test (test_gpu_graph_search.py imports it)


@pytest.mark.parametrize("name", sorted(gr.SHAPES))
def test_model_equals_graph_search_search(name):
    from vector_db_id_compression_amd import graph_search as gs

    s = gr.shape(name)
    nq = 8  # (graph_search.search is the slow statement: a sample of the queries)
    D, I = gs.search(gs.RawGraph(s["rows"]), s["x"], s["xq"][:nq], s["k"], L=s["L"], entry=0)
    wD, wI, _ = gr.expected(name)
    assert np.array_equal(D, wD[:nq]) and np.array_equal(I, wI[:nq])


@pytest.mark.parametrize("name", sorted(gr.SHAPES))
def test_shapes_hold_what_they_are_used_for(name):
    s = gr.shape(name)
    D, I, st = gr.expected(name)
    assert s["x"].dtype == np.float32 and np.array_equal(s["x"], np.round(s["x"])) and np.abs(s["x"]).max() <= s["R"]
    assert s["d"] * (2 * s["R"]) ** 2 < 2 ** 24  # every squared distance is an exact float32 integer
    assert int(st[:, 0].min()) >= 3  # every query takes at least three steps
    assert int(st[:, 1].min()) > s["L"]  # ... and overflows its pool: more nodes got a distance than the pool holds
    assert (I[:, : s["k"]] >= 0).all() and np.isfinite(D).all()
    ties = sum(1 for q in range(s["nq"]) if (np.diff(D[q]) == 0).any())
    assert ties >= (19 if s["nq"] == 20 else 36)  # an equal-distance tie inside the top k, decided by node id
    for q in range(s["nq"]):
        for a in range(s["k"] - 1):
            assert (D[q, a], I[q, a]) < (D[q, a + 1], I[q, a + 1])
    lens = (s["rows"] >= 0).sum(1)
    assert lens.min() == 0 and lens.max() == s["K"]  # an empty row and a full one
    # max_rounds is a real cap on these shapes
    _, _, st3 = gr.expected(name, max_rounds=3)
    assert (st3[:, 0] == 3).all()


def test_hostile_rows_hold_what_they_are_named_for():
    for empty_entry in (False, True):
        h = gr.hostile(entry_row_empty=empty_entry)
        rows, N = h["rows"], h["N"]
        r1 = rows[1][rows[1] >= 0]
        assert len(set(r1.tolist())) < r1.size  # a duplicate neighbour
        assert (rows[2] >= N).sum() >= 2 and rows[2].max() == 2 ** 31 - 1  # ids >= N, in front of and behind usable ones
        assert (rows[3] < 0).all() and ((rows[0] < 0).all() == empty_entry)
        order = gr.expanded_nodes(rows, h["x"], h["xq"], h["L"])
        D, I, st = gr.model(rows, h["x"], h["xq"], h["k"], h["L"])
        if empty_entry:
            assert all(o == [0] for o in order) and (st == [1, 1]).all() and (I[:, 0] == 0).all() and (I[:, 1:] == -1).all()
            assert np.isinf(D[:, 1:]).all()
        else:
            for node in (1, 2, 3):  # the rows are really read
                assert any(node in o for o in order), node
            assert (I < N).all()
    lean = gr.hostile(big_ids=False)
    assert (lean["rows"] < lean["N"]).all()


def test_model_rules():
    # node 1 twice in row 0, an id >= N, the row ends at the first negative entry; ties by node id
    rows = np.array([[1, 1, 9, 2, -1, 3], [3, -1, -1, -1, -1, -1], [-1] * 6, [-1] * 6], np.int32)
    x = np.array([[0], [1], [1], [0]], np.float32)
    D, I, st = gr.model(rows, x, np.array([[0]], np.float32), 4, 4)
    assert I.tolist() == [[0, 3, 1, 2]] and D.tolist() == [[0, 0, 1, 1]] and st.tolist() == [[4, 4]]
    D, I, st = gr.model(rows, x, np.array([[0]], np.float32), 2, 2, max_rounds=1)
    assert I.tolist() == [[0, 1]] and st.tolist() == [[1, 3]]
    # visited is permanent: node 2 was dropped from a pool of 2, node 1's row cannot bring it back
    rows2 = np.array([[1, 2, -1], [2, 3, -1], [-1] * 3, [-1] * 3], np.int32)
    x2 = np.array([[0], [1], [5], [6]], np.float32)
    D, I, st = gr.model(rows2, x2, np.array([[0]], np.float32), 2, 2)
    assert I.tolist() == [[0, 1]] and st.tolist() == [[2, 4]]


def _build(tmp, flags, name):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    path = str(tmp / name)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", *flags, "-o", path, os.path.join(ROOT, "tests", "graph_search_test.cpp")])
    return path


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("graph_search")
    return {"plain": _build(tmp, [], "graph_search_test"),
            "sanitized": _build(tmp, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "graph_search_test_san")}


@pytest.fixture(scope="module")
def cases():
    out = []
    for name in sorted(gr.SHAPES):
        s = gr.shape(name)
        nq = 6
        out.append((s["rows"], s["x"], s["xq"][:nq], s["k"], s["L"], 0, 0))
        out.append((s["rows"], s["x"], s["xq"][:nq], s["L"], s["L"], 0, 3))
    s = gr.shape("n300")
    out.append((s["rows"], s["x"], s["xq"][:6], 1, 1, 0, 0))
    out.append((s["rows"], s["x"], s["xq"][:6], 8, 256, 0, 0))
    out.append((s["rows"], s["x"], s["xq"][:6], 8, 8, 299, 1))
    for h in (gr.hostile(), gr.hostile(entry_row_empty=True)):
        out.append((h["rows"], h["x"], h["xq"], h["k"], h["L"], 0, 0))
    return gr.cases_text(out), len(out), sum(c[2].shape[0] for c in out)


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_self_checks(exes, which):
    out = subprocess.run([exes[which]], capture_output=True, text=True)
    assert out.returncode == 0 and "graph search ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_headers_equal_the_numpy_model(exes, cases, which):
    text, ncases, nq = cases
    assert ncases >= 13
    out = subprocess.run([exes[which], "cases"], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert f"{ncases} cases, {nq} queries" in out.stdout and "graph search ok" in out.stdout, out.stdout[-2000:]


def test_one_cu_batch_gives_every_slot_three_queries_and_a_ragged_last_trip(exes):
    s = gr.shape("n500")
    out = subprocess.run([exes["plain"], "plan", str(ONE_CU_NQ), "1", str(s["N"]), str(s["L"]), str(s["d"])], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    slots, scratch, lds, lo, hi, G, V = map(int, out.stdout.split())
    assert slots == 32 == gr.plan_slots(ONE_CU_NQ, 1)
    assert lo >= 3 and hi == lo + 1  # every slot takes three queries, some a fourth: the last trip is ragged
    assert [gr.plan_slot_queries(ONE_CU_NQ, slots, i) for i in (0, 4, 5, 31)] == [4, 4, 3, 3]
    assert scratch == slots * ((s["N"] + 63) // 64) * 8 and lds < 160 * 1024 // 32
    assert (G, V) == (1, 4)
    # the stated bound: 1024 slots, 128 MB at N = 10^6
    out = subprocess.run([exes["plain"], "plan", "10000", "256", "1000000", "64", "16"], capture_output=True, text=True)
    slots, scratch, lds, lo, hi, G, V = map(int, out.stdout.split())
    assert slots == 1024 and scratch == 128_000_000 and lds == 2112 and (G, V) == (4, 4)
