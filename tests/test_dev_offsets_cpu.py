"""Device-offsets entry points without a GPU: argument checks that return before any device work, and the header block compiling
from plain C."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["vidc_packed_encode_dev", "vidc_ef_encode_dev", "vidc_wt_build_dev", "vidc_roc_encode_dev"]


def _call(name, ctx, out):
    from vector_db_id_compression_amd import _lib

    fn = getattr(_lib.lib(), name)
    fake_dev = C.c_void_p(0x1000)  # never dereferenced: the calls reject the arguments first
    if name == "vidc_roc_encode_dev":
        return fn(ctx, 4, fake_dev, 10, fake_dev, -1, 0, out)
    return fn(ctx, 4, fake_dev, 10, fake_dev, 0, out)


@pytest.mark.parametrize("name", NAMES)
def test_null_ctx_or_out_is_invalid(name):
    h = C.c_void_p()
    assert _call(name, None, C.byref(h)) == -1
    dummy = C.create_string_buffer(64)
    assert _call(name, C.cast(dummy, C.c_void_p), None) == -1
    assert _call(name, None, None) == -1


def test_offsets_exports_reject_null():
    from vector_db_id_compression_amd import _lib

    buf = (C.c_uint64 * 4)()
    assert _lib.lib().vidc_packed_offsets(None, None, buf) == -1
    assert _lib.lib().vidc_wt_offsets(None, None, buf) == -1


def test_header_compiles_from_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler")
    src = tmp_path / "dev_offsets.c"
    src.write_text(
        "#include \"vidc.h\"\n"
        "int use(vidc_ctx *ctx, const uint64_t *d_off, const uint64_t *d_ids) {\n"
        "    vidc_packed *p; vidc_ef *e; vidc_wt *w; vidc_roc *r; uint64_t h[2];\n"
        "    int s = vidc_packed_encode_dev(ctx, 1, d_off, 4, d_ids, 3, &p);\n"
        "    s |= vidc_ef_encode_dev(ctx, 1, d_off, 4, d_ids, VIDC_EF_WANT_PERM, &e);\n"
        "    s |= vidc_wt_build_dev(ctx, 1, d_off, 4, d_ids, 0, &w);\n"
        "    s |= vidc_roc_encode_dev(ctx, 1, d_off, 4, d_ids, VIDC_PREC_REFERENCE, VIDC_ROC_WANT_PERM, &r);\n"
        "    s |= vidc_packed_offsets(ctx, p, h) | vidc_wt_offsets(ctx, w, h);\n"
        "    return s;\n"
        "}\n")
    r = subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "dev_offsets.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
