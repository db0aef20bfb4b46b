"""CPU: the numpy model of the residual-PQ scan and range search (tests/ivf_residual_ref.py) against the brute force written from the
header text, on the designed objects; and the inputs held to what they are for: the centroid matters on every row with results, a
table of another list gives another result, `distinct` is (nearly) tie-free and `ties` has ties inside every top k."""
import numpy as np
import pytest

import ivf_range_ref as rr
import ivf_residual_ref as rs
import ivf_scan_ref as ir

KS = (1, 10, 64, 256)
NONEMPTY = [l for l, n in enumerate(ir.EDGE_SIZES) if n]


def same(got, want):
    return all(np.array_equal(np.asarray(g), np.asarray(w)) for g, w in zip(got, want))


@pytest.mark.parametrize("d,M", rs.FORMS)
def test_model_against_brute_force(d, M):
    o = rs.obj(d, M)
    a = (o["offsets"], o["codes"], o["codebooks"], o["centroids"])
    for xq, rows in ((rs.queries(d, len(rs.EDGE_ROWS)), rs.EDGE_ROWS), (rs.queries(d, 5), ir.probe_rows(5, 7))):
        full = rs.brute_force(*a, xq, rows, 256)
        for k in KS:
            want = (full[0][:, :k], full[1][:, :k], full[2])  # (the first k of the first 256)
            if k < 256:
                assert same(rs.brute_force(*a, xq[:2], rows[:2], k), [w[:2] for w in want])
            for S in (1, 2, 4):
                assert same(rs.model(*a, xq, rows, k, S), want), (d, M, k, S)
        for radius in rs.radii(d, M):
            got, want = rs.range_model(*a, xq, rows, radius), rs.range_brute_force(*a, xq, rows, radius)
            assert same(got, want) and rr.same_bits(got[1], want[1]), (d, M, radius)
    none, some, every = (rs.range_model(*a, rs.queries(d, len(rs.EDGE_ROWS)), rs.EDGE_ROWS, r)[1].size for r in rs.radii(d, M))
    assert none == 0 < some < every


@pytest.mark.parametrize("d,M", rs.FORMS)
def test_the_centroid_and_the_list_of_a_table_matter(d, M):
    o, xq = rs.obj(d, M), rs.queries(d, len(rs.EDGE_ROWS))
    a = (o["offsets"], o["codes"], o["codebooks"])
    want = rs.model(*a, o["centroids"], xq, rs.EDGE_ROWS, 64)
    with_results = np.flatnonzero(want[1][:, 0] >= 0)
    assert with_results.size == 10
    dropped = rs.model(*a, np.zeros_like(o["centroids"]), xq, rs.EDGE_ROWS, 64)
    changed = [q for q in with_results if not (np.array_equal(want[0][q], dropped[0][q]) and np.array_equal(want[1][q], dropped[1][q]))]
    assert len(changed) == 10  # a kernel that forgot the centroid fails every row
    # every list scanned with the table of the row's first non-empty list
    several, moved = 0, 0
    for q, row in enumerate(rs.EDGE_ROWS):
        lists = [l for l in ir.valid_lists(row, o["nlist"]) if l in NONEMPTY]
        if len(lists) < 2:
            continue
        several += 1
        first = np.tile(o["centroids"][lists[0]], (o["nlist"], 1))
        stale = rs.model(*a, first, xq[q:q + 1], row[None, :], 64)
        moved += not (np.array_equal(stale[0][0], want[0][q]) and np.array_equal(stale[1][0], want[1][q]))
    assert several == 5 and moved >= 4, (several, moved)


def test_shapes_are_what_they_are_for():
    s = rs.shape("distinct")
    assert s["M"] == 4 and s["codes"].shape == (s["ntotal"], 4)
    free = ir.tie_free(s["offsets"], s["vecs"], s["xq"], s["probes"], s["k"])
    assert free.sum() >= 60, int(free.sum())
    t = rs.shape("ties")
    D = rs.expected("ties")[0]
    assert all(np.unique(row).size < row.size for row in D)  # every query has ties inside its top k
    for name in rs.SHAPE_M:  # the model on the shapes, against the brute force
        s = rs.shape(name)
        a = (s["offsets"], s["codes"], s["codebooks"], s["centroids"])
        assert same(rs.brute_force(*a, s["xq"][:6], s["probes"][:6], s["k"]), [w[:6] for w in rs.expected(name)])
    assert t["d"] * (3 * t["R"]) ** 2 < 2 ** 24 and s["d"] * (3 * s["R"]) ** 2 < 2 ** 24
