"""Device-resident request entry points (vidc_*_translate_labels_dev, vidc_*_decode_rows_dev, vidc_compact_rows_decode_dev) without a
GPU: argument checks that return before any device work, and the header block compiling from plain C."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LABELS = ["vidc_packed_translate_labels_dev", "vidc_ef_translate_labels_dev", "vidc_wt_translate_labels_dev",
          "vidc_roc_translate_labels_dev"]
ROWS = ["vidc_compact_rows_decode_dev", "vidc_ef_decode_rows_dev", "vidc_roc_decode_rows_dev"]

FAKE = C.c_void_p(0x1000)  # never dereferenced: the calls reject the arguments first


def _fn(name):
    from vector_db_id_compression_amd import _lib

    return getattr(_lib.lib(), name)


def _call(name, ctx, obj, n, arr, K=16):
    fn = _fn(name)
    if name in LABELS:
        return fn(ctx, obj, n, arr, arr, None)
    if name == "vidc_compact_rows_decode_dev":
        return fn(ctx, obj, n, arr, arr, None, None)
    return fn(ctx, obj, n, arr, K, arr, None, None)


@pytest.mark.parametrize("name", LABELS + ROWS)
def test_null_arguments_are_invalid(name):
    dummy = C.create_string_buffer(64)
    obj = C.cast(dummy, C.c_void_p)
    assert _call(name, None, obj, 4, FAKE) == -1
    assert _call(name, obj, None, 4, FAKE) == -1
    assert _call(name, obj, obj, 4, None) == -1
    assert _call(name, None, None, 0, None) == -1


@pytest.mark.parametrize("name", LABELS + ROWS)
def test_null_array_is_fine_for_an_empty_request(name):
    dummy = C.create_string_buffer(64)
    obj = C.cast(dummy, C.c_void_p)
    assert _call(name, obj, obj, 0, None) == 0


@pytest.mark.parametrize("codec", ["ef", "roc"])
def test_k0_is_rejected_as_the_host_node_call_rejects_it(codec):
    dummy = C.create_string_buffer(64)
    obj = C.cast(dummy, C.c_void_p)
    host = _fn(f"vidc_{codec}_decode_rows")(obj, obj, 4, FAKE, 0, FAKE, None)
    assert host != 0
    assert _fn(f"vidc_{codec}_decode_rows_dev")(obj, obj, 4, FAKE, 0, FAKE, None, None) == host
    assert _fn(f"vidc_{codec}_decode_rows_dev")(obj, obj, 0, None, 0, None, None, None) == host


def test_header_compiles_from_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler")
    src = tmp_path / "device_requests.c"
    src.write_text(
        "#include \"vidc.h\"\n"
        "int use(vidc_ctx *ctx, vidc_packed *p, vidc_ef *e, vidc_wt *w, vidc_roc *r, vidc_compact *c, int64_t *d_lab,\n"
        "        int32_t *d_out, uint32_t *d_cnt, uint64_t *d_inv) {\n"
        "    int s = vidc_packed_translate_labels_dev(ctx, p, 4, d_lab, d_lab, d_inv);\n"
        "    s |= vidc_ef_translate_labels_dev(ctx, e, 4, d_lab, d_lab, d_inv);\n"
        "    s |= vidc_wt_translate_labels_dev(ctx, w, 4, d_lab, d_lab, NULL);\n"
        "    s |= vidc_roc_translate_labels_dev(ctx, r, 4, d_lab, d_lab, d_inv);\n"
        "    s |= vidc_compact_rows_decode_dev(ctx, c, 4, d_lab, d_out, d_cnt, d_inv);\n"
        "    s |= vidc_ef_decode_rows_dev(ctx, e, 4, d_lab, 32, d_out, NULL, d_inv);\n"
        "    s |= vidc_roc_decode_rows_dev(ctx, r, 4, d_lab, 32, d_out, d_cnt, NULL);\n"
        "    return s;\n"
        "}\n")
    r = subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "device_requests.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_surface_exists():
    from vector_db_id_compression_amd import altid, codecs, custom_invlists, graph_search

    for cls in (codecs.PackedLists, codecs.EfLists, codecs.WaveletTreeLists, codecs.RocLists,
                custom_invlists.InvertedListsArrayCodes):
        assert callable(getattr(cls, "translate_labels"))
    assert callable(altid.CompactBitNSGGraph.get_neighbors_device)
    assert callable(graph_search.RawGraph.get_neighbors_device)
