"""CPU: vidc_ivf_kmeans_step_dev is declared, listed and loadable; every limit is VIDC_ERR_INVALID before any device work; the plan
header holds its written-out table, plain and under the address and undefined-behaviour sanitizers (a stand-alone program); the
model's chunk rule equals a plain loop; IVFIndex.train_device is an instance attribute that defaults to False."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ivf_kmeans_ref as km

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vidc_ivf_kmeans_step_dev"


def test_symbol_declared_listed_and_loadable():
    from vector_db_id_compression_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "vidc.h")).read()
    assert NAME in re.findall(r"\b(vidc_[a-z0-9_]+)\s*\(", hdr) and NAME in _lib.EXPORTED_SYMBOLS and hasattr(ctypes.CDLL(build.build()), NAME)
    fn = getattr(_lib.lib(), NAME)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 11
    assert hdr.index("vidc_ivf_pq_encode_dev(") < hdr.index(NAME + "(")


@pytest.mark.parametrize("kw", [dict(ctx=None), dict(ctx=None, n=0), dict(x=None), dict(c_in=None), dict(c_out=None), dict(G=0), dict(k=0),
                                dict(dsub=0), dict(dsub=2049, ld=4096), dict(ld=7), dict(G=1, k=2 ** 24 + 1), dict(n=2 ** 32),
                                dict(c_out=8), dict(n=0, G=0)], ids=str)
def test_limits_are_refused_before_any_device_work(kw):
    from vector_db_id_compression_amd import _lib

    a = dict(ctx=8, n=5, x=8, ld=8, G=2, dsub=4, k=3, c_in=8, c_out=16, assign=8, counts=8)  # (never dereferenced)
    a.update(kw)
    st = _lib.lib().vidc_ivf_kmeans_step_dev(a["ctx"], a["n"], a["x"], a["ld"], a["G"], a["dsub"], a["k"], a["c_in"], a["c_out"], a["assign"],
                                             a["counts"])
    assert st == -1 and b"ivf kmeans step:" in _lib.lib().vidc_last_error()


@pytest.mark.parametrize("flags", ([], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), ids=("plain", "sanitized"))
def test_the_plan_against_its_table(tmp_path, flags):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path / "ivf_kmeans_plan_test")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", *flags, "-I", os.path.join(ROOT, "vector_db_id_compression_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "ivf_kmeans_plan_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok ") and not out.stderr, out.stderr


@pytest.mark.parametrize("m", (1, 255, 256, 257, 513))
def test_the_chunk_rule_of_the_model(m):
    """update() against a loop written out: chunks of 256 members in ascending point order, partials added in chunk order"""
    rng = np.random.default_rng(m)
    x = rng.standard_normal((m + 40, 3)).astype(np.float32)
    a = np.zeros((1, m + 40), np.int32)
    a[0, rng.permutation(m + 40)[:40]] = 2  # 40 points elsewhere; cluster 1 stays empty
    c = rng.standard_normal((1, 3, 3)).astype(np.float32)
    total, part, seen = np.zeros(3, np.float32), np.zeros(3, np.float32), 0
    for i in range(m + 40):
        if a[0, i] == 0:
            part, seen = part + x[i], seen + 1
            if seen % 256 == 0:
                total, part = total + part, np.zeros(3, np.float32)
    if seen % 256:
        total = total + part
    out, counts = km.update(x, c, a)
    assert counts.tolist() == [[m, 0, 40]] and np.array_equal(out[0, 0], total / np.float32(m)) and np.array_equal(out[0, 1], c[0, 1])
    assert np.array_equal(km.assign(np.array([[0.0, 0, 0], [1, 1, 1]], np.float32), np.array([[[1, 1, 1], [0, 0, 0], [0, 0, 0]]], np.float32)),
                          [[1, 0]])  # first-index ties


def test_train_device_defaults_to_off_and_is_no_class_attribute():
    from vector_db_id_compression_amd import ivf_train
    from vector_db_id_compression_amd.ivf import IVFIndex

    assert not hasattr(IVFIndex, "train_device") and IVFIndex(8, 2, ("PQ", 2)).train_device is False
    assert all(callable(getattr(ivf_train, f)) for f in ("kmeans_step_device", "kmeans_device", "pq_train_device"))
