"""CPU: the shapes of tests/test_gpu_small_grid.py give every capped grid-stride loop they are there for at least three trips on a
one-CU context, the last one ragged.

This is the condition that keeps the GPU tests from passing with loops that never take a second trip; it is a condition on the inputs,
checked here without a GPU, not a measurement.  The capacities are the table at the top of the GPU test file (re-derived from the
launch sites); the choices between kernel families that depend on the data -- which ROC compaction kernel a call takes, which
promote_r2 branch, which Elias-Fano chunk form, which wavelet-tree scatter -- are asserted from the same quantities the host code
looks at.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import roc_seg_ref as sr
import test_gpu_small_grid as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIST_SHAPES = ["short", "mid", "long", "mixed", "chunky", "full", "perm", "perm_big", "seg", "rows", "rows_wide", "rows_k7"]


def trips(items, cap):
    return -(-items // cap)


def assert_three_ragged_trips(items, family, what):
    cap, granule = sg.CAPACITY[family]
    last = items % cap
    assert items > 2 * cap, f"{what}: {items} items give {family} (capacity {cap}) only {trips(items, cap)} trips"
    assert last != 0, f"{what}: {items} items fill the last trip of {family} (capacity {cap})"
    assert granule == 1 or last % granule != 0, f"{what}: the last trip of {family} ({last} items) is made of whole units of {granule}"


@pytest.mark.parametrize("name", LIST_SHAPES)
def test_every_shape_offers_its_families_three_ragged_trips(name):
    offers = sg.shape(name)["offers"]
    assert offers, name
    for family, items in offers.items():
        assert_three_ragged_trips(items, family, name)


def test_the_batches_offer_the_sorter_and_the_request_kernels_three_ragged_trips():
    for family, items in list(sg.BATCH_OFFERS.items()) + list(sg.BATCH_SHORT_OFFERS.items()):
        assert_three_ragged_trips(items, family, "batch")
    for kind, name, n in (("roc", "chunky", sg.N_PAIRS), ("wt", "perm", sg.N_PAIRS), ("ef", "short", sg.N_PAIRS_SHORT)):
        sh = sg.shape(name)
        ln, add = sg.append_batch(kind, sh, n, seed=1)
        nlist = sh["sizes"].size
        assert ln.size == add.size == n and (ln < 0).any() and (ln >= nlist).any()
        assert np.unique(add[(ln >= 0) & (ln < nlist)]).size == int(((ln >= 0) & (ln < nlist)).sum()), "the batch ids are distinct"
        assert not np.isin(add, sh["ids"]).any(), "the batch ids are new"
        assert int(add.max()) < (1 << sg.BITS)
    sh = sg.shape("chunky")
    ln, ids = sg.pair_batch(sh["off"], sh["ids"], sg.N_PAIRS, seed=2)
    hit = np.isin(ids, sh["ids"])
    assert 0.5 < hit.mean() < 0.95 and (ln < 0).any() and (ln >= sh["sizes"].size).any()


def test_the_list_shapes_are_what_the_cases_count_on(oracle):
    for name in ("short", "mid", "long", "mixed", "chunky", "full", "many_long"):
        sh = sg.shape(name)
        assert int(sh["ids"].max()) < (1 << 31) and sh["off"][-1] == sh["ids"].size
        assert name not in ("short", "chunky", "full") or int(sh["ids"].max()) < (1 << sg.BITS), "the shapes packed bits run on"
        for li in sh["lists"][:: max(1, len(sh["lists"]) // 200)]:
            assert np.all(li[1:] > li[:-1]), f"{name}: ascending and distinct"
    # empty lists between working ones (the early `continue` paths), one list per size class of the chunk kernels
    sizes = sg.shape("chunky")["sizes"]
    assert (sizes == 0).sum() >= 20 and {512, 513, 1023, 1024, 1025, 2049, 4097, 5000} <= set(sizes.tolist())
    assert (sg.shape("short")["sizes"] == 0).sum() > 170
    # Elias-Fano chunk forms (ef_plan.h ef_chunk_form): short lists, half-full chunks, full chunks
    for name, form in (("short", "short"), ("chunky", "half"), ("full", "full")):
        s = sg.shape(name)["sizes"]
        nchunks = sg.chunks_of(s, 512)
        got = "short" if s.max() <= 256 else "half" if int(s.sum()) < 256 * nchunks else "full"
        assert got == form, (name, got)


def stream_words(oracle, name):
    sh = sg.shape(name)
    return sum(oracle.roc_encode(li, oracle.list_precision(li))["words"].size for li in sh["lists"] if li.size) / len(sh["lists"])


def test_the_roc_shapes_take_the_compaction_kernel_they_are_named_for(oracle):
    """roc.hip finish_complete picks by the call's average stream words per list: below 64 a lane per list, below 200 a wavefront per
    four lists, else a workgroup per list"""
    assert stream_words(oracle, "short") < 64 and stream_words(oracle, "mixed") < 64 and stream_words(oracle, "chunky") >= 64
    assert 64 <= stream_words(oracle, "mid") < 200
    assert stream_words(oracle, "long") >= 200
    # the lists the reference codec round-trips: no power-of-two maximum
    for name in ("short", "mid", "long", "chunky"):
        for li in sg.shape(name)["lists"]:
            assert li.size == 0 or int(li.max()) < (1 << oracle.list_precision(li)), name


def n_long(sizes):
    """lists at least half as long as the longest one"""
    return int((2 * sizes >= sizes.max()).sum())


def test_both_promote_r2_branches_at_one_cu(tmp_path):
    """csrc/roc_enc_plan.h itself, built with g++ (tests/small_grid_r2_test.cpp), classifies the shapes' lists and runs promote_r2 at
    one and at 256 compute units -> lists in the chain class, and what stays in the three general classes"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path / "small_grid_r2_test")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "small_grid_r2_test.cpp")])

    def chains(name, num_cu):
        sh = sg.shape(name)
        out = subprocess.run([exe, str(num_cu), str(int(sh["ids"].max()))] + [str(int(n)) for n in sh["sizes"]], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        return [int(x) for x in out.stdout.split()]

    # n_long <= cap = 4: the four lists at least half as long as the longest go to the chains; at 256 CUs every list above 256 ids does
    assert n_long(sg.shape("long")["sizes"]) == 4
    assert chains("long", 1) == [4, 36, 0, 0] and chains("long", 256) == [40, 0, 0, 0]
    # n_long = 7 > cap: cap + cap / 2 = 6 chains, one list stays in the deepest general class; at 256 CUs all seven are chains
    many = sg.shape("many_long")["sizes"]
    assert n_long(many) == 7 and 32768 < many.min() and many.max() <= 65536
    assert chains("many_long", 1) == [6, 0, 0, 1] and chains("many_long", 256) == [7, 0, 0, 0]
    assert chains("mixed", 1)[0] == 4 and chains("mixed", 256)[0] == 40


def test_the_segmented_shape(oracle):
    sh = sg.shape("seg")
    k = np.array([sr.seg_k(int(n), sg.SEG_T, sg.SEG_B) for n in sh["sizes"]])
    assert (k == 10).sum() == 17 and (k == 7).sum() == 3 and (k == 0).sum() == 35 and (sh["sizes"] == 0).sum() == 5
    chunks, tbl = sr.chunk_table(sh["off"], sg.SEG_T, sg.SEG_B)
    assert len(chunks) == sh["offers"]["chunk1024"] and int(tbl[-1]) > 8192, "the three-launch scan of the count table"
    # unsplit and empty lists stand between split ones in chunk order
    kinds = [int(k[l]) > 0 for l, _ in chunks]
    assert sum(a != b for a, b in zip(kinds, kinds[1:])) > 20
    assert int(sh["ids"].max()) < (1 << sg.SEG_B)


def test_the_wavelet_and_graph_shapes():
    for name in ("perm", "perm_big"):
        sh = sg.shape(name)
        assert np.array_equal(np.sort(sh["ids"]), np.arange(sh["ids"].size)), "a permutation"
        assert np.array_equal(sh["sym"][sh["ids"].astype(np.int64)], np.repeat(np.arange(sh["sizes"].size), sh["sizes"])), "sym[id] = its list"
        assert all(np.all(np.diff(li.astype(np.int64)) > 0) for li in sh["lists"]), "ascending inside every list"
    big = sg.shape("perm_big")["ids"].size
    assert 2 * sg.CAPACITY["wt_rrr_blocks"][0] < big <= (1 << 24) and -(-big // 63) > 2 * 8192, "three trips of 8192 blocks"
    sh = sg.shape("perm")
    assert (1 << 18) <= sh["ids"].size <= (1 << 24) and (sh["sizes"] == 0).sum() > 80, "the partitioned scatter unless VIDC_WT_SCATTER is set"
    for l in (1, 2, 599):
        li = sh["lists"][l]
        assert li.size and np.all(li[1:] > li[:-1])
    import rows_ref as rr

    assert sg.ROWS_SHAPES == {"rows": 16, "rows_wide": 80, "rows_k7": 7}
    # rows_tile.h tile_grid at K = 16: the LDS bytes of a compact tile (packed.hip compact_rows_launch) leave room for 16 tiles a CU
    for N in (sg.ROWS_N, sg.ROWS_N + sg.ROWS_GROW):
        SD = rr.compact_stride(N, 16) // 4
        assert min(16, (150 << 10) // ((64 * (SD | 1) + 1) * 4)) * 64 == sg.CAPACITY["rows_tile"][0]
    for name, K in sg.ROWS_SHAPES.items():
        # (packed.hip compact_tile: K <= 64 and a stride of whole dwords take the tile kernels)
        assert (K <= 64 and rr.compact_stride(sg.ROWS_N, K) % 4 == 0) == (name == "rows"), name
        assert (K <= 64 and rr.compact_stride(sg.ROWS_N + sg.ROWS_GROW, K) % 4 == 0) == (name == "rows"), name
        assert sg.shape(name)["rows"].shape == (sg.ROWS_N, K) and sg.shape(name)["upd_rows"].shape == (sg.ROWS_M, K)
    g = sg.shape("rows")
    N = g["rows"].shape[0]
    assert g["rows"].shape == (sg.ROWS_N, sg.ROWS_K) and g["nodes"].size == g["upd_nodes"].size == g["upd_rows"].shape[0] == sg.ROWS_M
    assert (g["nodes"] < 0).any() and (g["nodes"] >= N).any() and np.unique(g["nodes"][(g["nodes"] >= 0) & (g["nodes"] < N)]).size > 0.9 * N
    assert (g["upd_nodes"] < 0).any() and (g["upd_nodes"] >= g["n_new"]).any() and ((g["upd_nodes"] >= N) & (g["upd_nodes"] < g["n_new"])).any()
    assert int(g["upd_rows"].max()) < N
