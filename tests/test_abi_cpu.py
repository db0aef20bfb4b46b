"""CPU: the C-ABI library builds, loads, exports every symbol include/vidc.h declares, and fails loudly without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libpath():
    from vector_db_id_compression_amd import build

    return build.build()


def test_header_symbols_are_exported(libpath):
    hdr = open(os.path.join(ROOT, "include", "vidc.h")).read()
    declared = set(re.findall(r"\b(vidc_[a-z0-9_]+)\s*\(", hdr))
    from vector_db_id_compression_amd import _lib

    assert declared == set(_lib.EXPORTED_SYMBOLS), declared ^ set(_lib.EXPORTED_SYMBOLS)
    assert {"vidc_roc_last_decode_nonclean", "vidc_roc_last_decode_handed_back"} <= declared
    dll = ctypes.CDLL(libpath)
    for sym in sorted(declared):
        assert hasattr(dll, sym), sym


def test_pure_host_entry_points(libpath):
    from vector_db_id_compression_amd import _lib

    L = _lib.lib()
    assert L.vidc_version() == 100
    assert L.vidc_packed_bits_for(0) == 0 and L.vidc_packed_bits_for(1) == 1
    assert L.vidc_packed_bits_for(1_000_000) == 20 and L.vidc_packed_bits_for(1023) == 10
    assert L.vidc_packed_bits_for(1024) == 11
    # the decode self-checks of a ROC object: u64 accessors, 0 without an object
    for name in ("vidc_roc_last_decode_nonclean", "vidc_roc_last_decode_handed_back"):
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_uint64 and fn(None) == 0, name
    # the compute-unit count a context sizes its grids by (VIDC_NUM_CU test hook): u32, 0 without a context
    assert "vidc_ctx_num_cu" in _lib.EXPORTED_SYMBOLS and hasattr(_lib.Context, "num_cu")
    assert L.vidc_ctx_num_cu.restype is ctypes.c_uint32 and L.vidc_ctx_num_cu(None) == 0


def test_no_gpu_fails_loudly(libpath):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from vector_db_id_compression_amd import VidcError, _lib
    from vector_db_id_compression_amd.codecs import RocLists

    h = ctypes.c_void_p()
    assert _lib.lib().vidc_ctx_create(-1, ctypes.byref(h)) == -2  # VIDC_ERR_NO_DEVICE
    assert b"no CPU fallback" in _lib.lib().vidc_last_error()
    with pytest.raises(VidcError):
        RocLists.encode(np.array([0, 2], dtype=np.uint64), np.array([1, 2], dtype=np.uint64))


def test_product_does_not_touch_oracle():
    """The product package must never import / call anything under oracle/."""
    pkg = os.path.join(ROOT, "vector_db_id_compression_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f), errors="replace").read()
                assert "oracle" not in src.replace("the oracle", "").lower() or f == "never", (dirpath, f)


def test_build_staleness_is_decided_by_content_not_mtime(tmp_path):
    """build.needs_build(): a `touch` of a source (or a checkout / copy that changes mtimes) must not trigger a recompile, a
    changed byte must; the library is never compiled into place (temporary file + rename under a lock)."""
    import os
    import time

    from vector_db_id_compression_amd import build

    build.build()
    assert not build.needs_build()
    src = build.sources()[0]
    st = os.stat(src)
    try:
        os.utime(src, (time.time() + 100, time.time() + 100))  # newer than libvidc.so
        assert not build.needs_build()
    finally:
        os.utime(src, (st.st_atime, st.st_mtime))
    h0 = build.source_hash()
    hdr = os.path.join(build.CSRC, "_hash_probe.h")  # an extra header changes the hash of the source set
    try:
        open(hdr, "w").write("// probe\n")
        assert build.source_hash() != h0 and build.needs_build()
    finally:
        os.remove(hdr)
    assert build.source_hash() == h0 and not build.needs_build()
    assert "os.replace" in open(build.__file__).read()
