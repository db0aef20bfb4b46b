"""The wide IVF scans (vidc_ivf_scan_wide_dev, vidc_ivf_scan_aq_wide_dev: 1 <= k <= 2048) without a GPU: the plan header through a
stand-alone g++ program, plain and sanitized; both symbols declared, listed and loadable; every refusal through the C-ABI before
any device work; IVFIndex.scan_device(..., 1000) names the missing device."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vidc_ivf_scan_wide_dev", "vidc_ivf_scan_aq_wide_dev")
P = 8  # (a pointer that is never dereferenced)
# the 17 arguments of the two calls, all acceptable
FLAT = dict(ctx=P, nlist=16, off=P, ntotal=2000, codes=P, kind=1, d=128, M=16, cb=P, nq=5, xq=P, nprobe=4, probes=P, k=1000, D=P, lab=P, stats=None)
AQ = dict(ctx=P, nlist=16, off=P, ntotal=2000, codes=P, d=128, M=8, cb=P, cent=None, nq=5, xq=P, nprobe=4, probes=P, k=1000, D=P, lab=P, stats=None)
SHARED = [dict(ctx=None), dict(off=None), dict(codes=None), dict(xq=None), dict(probes=None), dict(D=None), dict(lab=None), dict(k=0), dict(k=2049),
          dict(k=2 ** 32 - 1), dict(nprobe=0), dict(nprobe=1025), dict(d=0), dict(d=2049), dict(ntotal=2 ** 32), dict(nlist=2 ** 31),
          dict(M=0), dict(M=65), dict(cb=None), dict(nq=0, k=0), dict(nq=0, k=2049)]
BAD = {NAMES[0]: SHARED + [dict(kind=2), dict(kind=-1), dict(M=3)], NAMES[1]: SHARED + [dict(nq=2 ** 32)]}


@pytest.mark.parametrize("flags", ([], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), ids=("plain", "sanitized"))
def test_the_plan_header(tmp_path, flags):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path / "ivf_wide_plan_test")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", *flags, "-I", os.path.join(ROOT, "vector_db_id_compression_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "ivf_wide_plan_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout == "ok\n" and not out.stderr, out.stderr


@pytest.mark.parametrize("name", NAMES)
def test_refusals_come_before_any_device_work(name):
    from vector_db_id_compression_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "vidc.h")).read()
    fn = getattr(_lib.lib(), name)
    assert name in re.findall(r"\b(vidc_[a-z0-9_]+)\s*\(", hdr) and name in _lib.EXPORTED_SYMBOLS and len(fn.argtypes) == 17
    assert hdr.index("vidc_ivf_scan_aq_dev(") < hdr.index(name + "(") < hdr.index("update rows (graph objects") and _lib.lib().vidc_version() == 100
    ok = FLAT if name == NAMES[0] else AQ
    for kw in BAD[name]:
        assert fn(*dict(ok, **kw).values()) == -1, kw
        assert b"wide scan" in _lib.lib().vidc_last_error(), kw
    # nq == 0 touches no array and needs no device, at either end of k
    for k in (1, 257, 2048):
        assert fn(*dict(ok, nq=0, k=k, off=None, codes=None, xq=None, probes=None, D=None, lab=None).values()) == 0, k


@pytest.mark.parametrize("code", ("Flat", ("PQ", 2), ("RQ", 2)), ids=str)
def test_a_short_list_of_1000_without_a_gpu_names_the_device(code):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from vector_db_id_compression_amd import VidcError
    from vector_db_id_compression_amd.ivf import IVFIndex

    with pytest.raises(VidcError, match="no HIP device"):
        IVFIndex(4, 2, code).scan_device(np.zeros((1, 4), np.float32), 1000)
