"""CPU: the packed PQ layout in numpy (tests/ivf_pqbits_ref.py) round-trips, is the identity on bytes at 8 bits and gives the known
row; the two plan headers (sizes, slots, every refusal) through a stand-alone g++ program; the two entry points are listed and
loadable; IVFIndex takes ("PQ", M, nbits), and range search refuses such an index before any device call."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ivf_pqbits_ref as pb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("M,nbits", [(8, 10), (3, 10), (5, 5), (16, 4), (2, 12), (7, 1), (4, 8)])
def test_pack_round_trips(M, nbits):
    f = np.random.default_rng(M + nbits).integers(0, 1 << nbits, size=(97, M))
    f[0], f[1] = 0, (1 << nbits) - 1
    codes = pb.pack(f, nbits)
    assert codes.shape == (97, (M * nbits + 7) // 8) and np.array_equal(pb.unpack(codes, M, nbits), f)
    if M * nbits % 8:
        assert (codes[:, -1] >> (M * nbits % 8) == 0).all(), "pad bits"
    if nbits == 8:
        assert np.array_equal(codes, f.astype(np.uint8))


def test_the_known_row():
    assert pb.pack([[1, 2, 3]], 10).tolist() == [[0x01, 0x08, 0x30, 0x00]]


@pytest.mark.parametrize("flags", ([], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), ids=("plain", "sanitized"))
def test_the_plan_headers(tmp_path, flags):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path / "ivf_pqbits_plan_test")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", *flags, "-I", os.path.join(ROOT, "vector_db_id_compression_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "ivf_pqbits_plan_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout == "ok\n" and not out.stderr, out.stderr


def test_the_index_takes_the_code_and_range_search_refuses_it():
    from vector_db_id_compression_amd import _lib, ivf_range
    from vector_db_id_compression_amd.ivf import IVFIndex

    for name, nargs in (("vidc_ivf_pq_encode_bits_dev", 11), ("vidc_ivf_scan_pqbits_dev", 18)):
        assert name in _lib.EXPORTED_SYMBOLS and len(getattr(_lib.lib(), name).argtypes) == nargs
    idx = IVFIndex(16, 8, ("PQ", 8, 10), by_residual=True)
    assert (idx.code_size, idx.nbits, idx.packed, idx.invlists.code_size) == (10, 10, True, 10)
    old = IVFIndex(16, 8, ("PQ", 8))
    assert (old.code_size, old.nbits, old.packed, old.code) == (8, 8, False, ("PQ", 8))
    with pytest.raises(ValueError, match="nbits"):
        IVFIndex(16, 8, ("PQ", 8, 13))
    with pytest.raises(ValueError, match="range search over"):  # (raised before the device is looked for; xq is never read)
        ivf_range.range_scan_device(idx, None, 1.0)
