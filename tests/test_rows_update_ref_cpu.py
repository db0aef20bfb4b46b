"""CPU: the numpy model of update_rows (tests/rows_update_ref.py) against the definition spelled out as a Python loop, on random and
adversarial batches; the host-side statement of csrc/rows_update.h (slot table, sources, re-stride) as a stand-alone program, plain and
under -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rows_ref as rr
import rows_update_ref as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ru.BATCHES)
@pytest.mark.parametrize("n_old,grow,K,m", [(1, 0, 1, 1), (1, 1, 7, 65), (63, 0, 7, 64), (64, 1, 32, 63), (65, 3, 33, 1000), (200, 56, 64, 65),
                                            (200, 0, 5, 0), (0, 5, 4, 9), (0, 0, 4, 3)])
def test_model_against_the_loop(name, n_old, grow, K, m):
    rng = np.random.default_rng([n_old, grow, K, m])
    n_new = n_old + grow
    rows = rr.family("uniform", n_old, K, seed=1) if n_old else np.zeros((0, K), np.int32)
    batch = rr.family("uniform", max(n_new, 1), K, seed=2, nrows=m) if m else np.zeros((0, K), np.int32)
    nodes = ru.batch_nodes(name, m, n_new, seed=int(rng.integers(1 << 30)))
    got, invalid, slot = ru.update_rows(rows, nodes, batch, n_new)
    want, want_invalid = ru.update_rows_loop(rows, nodes, batch, n_new)
    assert got.shape == (n_new, K) and np.array_equal(got, want)
    assert invalid == want_invalid
    # the slot table says where every row came from
    for v in range(n_new):
        mentions = np.flatnonzero(nodes == v)
        assert slot[v] == (mentions[-1] + 1 if mentions.size else 0)


def test_last_mention_wins_and_skipped_nodes_change_nothing():
    rows = np.array([[1, 2, -1], [0, -1, -1], [-1, -1, -1]], np.int32)
    nodes = np.array([1, -1, 1, 5, 3, -7, 1 << 40], np.int64)
    batch = np.arange(21, dtype=np.int32).reshape(7, 3)
    got, invalid, slot = ru.update_rows(rows, nodes, batch, 5)
    assert invalid == 2 and slot.tolist() == [0, 3, 0, 5, 0]
    assert got.tolist() == [[1, 2, -1], [6, 7, 8], [-1, -1, -1], [12, 13, 14], [-1, -1, -1]]
    same, invalid, _ = ru.update_rows(rows, np.array([-1, 9]), batch[:2], None)
    assert invalid == 1 and np.array_equal(same, rows)
    empty, invalid, _ = ru.update_rows(rows, np.zeros(0, np.int64), np.zeros((0, 3), np.int32), 4)
    assert invalid == 0 and np.array_equal(empty[:3], rows) and empty[3].tolist() == [-1, -1, -1]


def test_batches_are_what_their_names_say():
    m, n = 1000, 200
    t = ru.batch_nodes("repeats_in_tile", m, n)
    assert (t[:7] == t[0]).all()
    a = ru.batch_nodes("repeats_across_tiles", m, n)
    assert np.array_equal(a[:64], a[64:128])
    assert (ru.batch_nodes("negatives", m, n) < 0).sum() > m // 5
    assert (ru.batch_nodes("beyond", m, n) >= n).sum() > m // 5
    assert np.unique(ru.batch_nodes("every_node", m, n)).size == n
    assert np.bincount(ru.batch_nodes("every_node_twice", m, n), minlength=n).min() >= 2
    mixed = ru.batch_nodes("mixed", m, n)
    assert (mixed < 0).any() and (mixed >= n).any() and np.bincount(mixed[(mixed >= 0) & (mixed < n)]).max() > 64


@pytest.mark.parametrize("sanitize", [False, True])
def test_host_statement_of_the_header(tmp_path, sanitize):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / ("rows_update_plan_test" + ("_san" if sanitize else "")))
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    if sanitize:  # a stand-alone host program: the sanitizer runtimes are linked into it
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([gxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "rows_update_plan_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "rows update plan ok" in out.stdout, out.stdout + out.stderr
