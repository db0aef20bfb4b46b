"""CPU: vidc_ivf_pq_encode_dev is declared, listed and loadable; every limit is VIDC_ERR_INVALID before any device work and n == 0
returns VIDC_OK without a device; the plan header holds its bounds over a grid of shapes, plain and under the address and
undefined-behaviour sanitizers (a stand-alone program); IVFIndex.pq_device is an instance attribute that defaults to False."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vidc_ivf_pq_encode_dev"


def test_symbol_declared_listed_and_loadable():
    from vector_db_id_compression_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "vidc.h")).read()
    assert NAME in re.findall(r"\b(vidc_[a-z0-9_]+)\s*\(", hdr) and NAME in _lib.EXPORTED_SYMBOLS and hasattr(ctypes.CDLL(build.build()), NAME)
    fn = getattr(_lib.lib(), NAME)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 10
    assert hdr.index("vidc_ivf_probe_dev(") < hdr.index(NAME + "(") and NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _encode(**kw):
    from vector_db_id_compression_amd import _lib

    p = 8  # (never dereferenced)
    a = dict(ctx=p, n=5, x=p, d=128, M=16, pq=p, nlist=7, cent=p, assign=p, codes=p)
    a.update(kw)
    return _lib.lib().vidc_ivf_pq_encode_dev(a["ctx"], a["n"], a["x"], a["d"], a["M"], a["pq"], a["nlist"], a["cent"], a["assign"], a["codes"])


@pytest.mark.parametrize("kw", [dict(ctx=None), dict(ctx=None, n=0), dict(x=None), dict(pq=None), dict(codes=None), dict(assign=None),
                                dict(nlist=0), dict(nlist=2 ** 31), dict(d=0), dict(d=2049), dict(M=0), dict(M=3), dict(d=258, M=2),
                                dict(n=2 ** 32), dict(n=0, M=0), dict(n=0, assign=None)], ids=str)
def test_limits_are_refused_before_any_device_work(kw):
    from vector_db_id_compression_amd import _lib

    assert _encode(**kw) == -1 and b"ivf pq encode:" in _lib.lib().vidc_last_error()


def test_an_empty_call_needs_no_device():
    assert _encode(n=0) == 0 and _encode(n=0, x=None, pq=None, codes=None, cent=None, assign=None, nlist=0) == 0
    assert _encode(n=0, d=2048, M=16, nlist=2 ** 31 - 1) == 0


@pytest.mark.parametrize("flags", ([], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), ids=("plain", "sanitized"))
def test_the_plan_over_a_grid_of_shapes(tmp_path, flags):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path / "ivf_pq_encode_plan_test")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", *flags, "-I", os.path.join(ROOT, "vector_db_id_compression_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "ivf_pq_encode_plan_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok ") and not out.stderr, out.stderr
    assert int(out.stdout.split()[1]) == 2 * 8 * 8 * 4


def test_pq_device_defaults_to_off_and_is_no_class_attribute():
    from vector_db_id_compression_amd import ivf_encode
    from vector_db_id_compression_amd.ivf import IVFIndex

    assert not hasattr(IVFIndex, "pq_device") and IVFIndex(8, 2, ("PQ", 2)).pq_device is False
    assert callable(ivf_encode.pq_encode_device) and callable(ivf_encode.encode_device)
