"""Additive-quantiser codes without a GPU: the layout model (tests/ivf_aq_ref.py) round-trips and gives the known row; the plan header
(every refusal, the chunk rule, the LDS sizes) through a stand-alone g++ program; the two entry points are listed and loadable;
IVFIndex takes ("RQ", M), and range search refuses such an index before any device call."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ivf_aq_ref as aq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_layout():
    assert aq.pack([[1, 2]], [1.0]).tolist() == [[0x01, 0x02, 0x00, 0x00, 0x80, 0x3F]]
    rng = np.random.default_rng(1)
    idx, norm = rng.integers(0, 256, size=(97, 5)), rng.standard_normal(97).astype(np.float32)
    codes = aq.pack(idx, norm)
    got = aq.unpack(codes, 5)
    assert codes.shape == (97, 9) and np.array_equal(got[0], idx) and np.array_equal(got[1].view(np.uint32), norm.view(np.uint32))


@pytest.mark.parametrize("flags", ([], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), ids=("plain", "sanitized"))
def test_the_plan_header(tmp_path, flags):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path / "ivf_aq_plan_test")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", *flags, "-I", os.path.join(ROOT, "vector_db_id_compression_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "ivf_aq_plan_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout == "ok\n" and not out.stderr, out.stderr


def test_the_index_takes_the_code_and_range_search_refuses_it():
    from vector_db_id_compression_amd import _lib, ivf_range
    from vector_db_id_compression_amd.ivf import IVFIndex

    for name, nargs in (("vidc_ivf_aq_lut_dev", 7), ("vidc_ivf_scan_aq_dev", 17)):
        assert name in _lib.EXPORTED_SYMBOLS and len(getattr(_lib.lib(), name).argtypes) == nargs
    idx = IVFIndex(16, 8, ("RQ", 4), by_residual=True)
    assert (idx.code_size, idx.M, idx.aq, idx.packed, idx.invlists.code_size) == (8, 4, True, False, 8)
    assert not IVFIndex(16, 8, ("PQ", 8)).aq and not IVFIndex(16, 8).aq
    with pytest.raises(ValueError, match="no third entry"):  # (stage widths other than 8 bits are out of scope)
        IVFIndex(16, 8, ("RQ", 4, 10))
    with pytest.raises(ValueError, match="range search over"):  # (raised before the device is looked for; xq is never read)
        ivf_range.range_scan_device(idx, None, 1.0)
