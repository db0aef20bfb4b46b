"""GPU: Elias-Fano coded IVF lists on the structured id families of tests/lists_ref.py -- every word of every list against the numpy
model, every position through every random-access entry point.

tests/test_lists_ref_cpu.py proves (without a GPU) that the model equals the CPU oracle on these lists and that every family reaches
the boundary it is named after; the case distinctions of csrc/ef.hip map to families like this:

  low-bit width without a division (ef_meta_tile)             quotient_edges, low_widths          info / export of every list
  word ownership between chunks (wlo / whi / tail_bits)       chunk_seams, constant_runs          export: every high word
  the 128-word LDS window                                     window_spans, batch_seams           export: every high word
  the select directory: 0 / 1 / 4 / 5 / > 64 owned batches    owned_batches, batch_seams          get / translate / gather / decode at every position
  full, empty and tied directory batches                      constant_runs, head_and_outlier     the same
  four lanes x four words of k_ef_translate_g16               batch_seams, chunk_seams, runs      translate_labels at every position

The encoder picks its chunk kernel per OBJECT, so the families are dealt into objects by list length (lists_ref.base_lists), and every
object is encoded along four routes (lists_ref.object_lists); lists_ref.encoder_form restates the host's choice (csrc/ef_plan.h: ef_chunk_form;
tests/test_ef_plan_cpu.py asserts that the two agree on every object) and the CPU file asserts this table from it:

  object      route      encoder                                              bulk decoder (decode_all)
  short       host       k_ef_lowhigh32<4, SMALL>   (no list above 256 ids)   k_ef_decode_rec<uint32_t, 4>
  half        host       k_ef_lowhigh32<8, SMALL>   (ntotal < 256 nchunks)    k_ef_decode_rec<uint32_t, 8>
  full_*      host       k_ef_lowhigh32<8>                                    k_ef_decode_rec<uint32_t, 8>
  any         dev        k_ef_lowhigh32_dev, the form of the same name        as under host
  any         wide       k_ef_lowhigh               (an id of 2^32 or more)   k_ef_decode_rec<uint64_t, 4> (short) / <uint64_t, 8>
  any         unsorted   k_ef_sort / k_ef_low / k_ef_high / k_ef_hrank        records built on the first decode_all (k_ef_build_recs),
                         (the whole object)                                    k_ef_decode_rec<uint32_t, 4 | 8>
  chunks of exactly 256 ids take the predicate-free (FULL) body in the SMALL forms: short and half hold lists of 256, half one of 768
  lists of more than 8 chunks get their chunk records from k_ef_big_recs: full_q / full_runs hold 4096 (not yet) and 4097 ids
  VIDC_EF_LAZY_RECS=1: every object builds its records on the first decode_all instead of in the encoder
  decode_lists of the three longest lists of a full_* object: k_ef_decode with nsplit > 1 (a list of 4096 ids or more)
  save -> load: the directory comes from k_ef_hrank_from_high

Every expectation is the model or the input; the one comparison between outputs of the library is the route equality named in
test_streams_equal_the_model_word_for_word."""
import numpy as np
import pytest

import lists_ref as lr

pytestmark = pytest.mark.gpu

CASES = [(o, r) for o in lr.OBJECTS for r in lr.ROUTES]
_DATA, _MODELS, _OBJ, _WORDS = {}, {}, {}, {}  # filled on demand (any test order), emptied when the file is done


@pytest.fixture(scope="module", autouse=True)
def _release_objects():
    yield
    for cache in (_OBJ, _WORDS, _DATA, _MODELS):  # the encoded objects live on the GPU: do not keep them for the rest of the suite
        cache.clear()


class Data:
    """one object's input (lists; the first nbase are the same under every route) and what every entry point must answer"""

    def __init__(self, lists, nbase, models=None):
        self.lists, self.nbase = lists, nbase
        self.want = [np.sort(li) for li in lists]  # (only the unsorted route's extra list changes)
        self.sizes = np.array([li.size for li in lists], dtype=np.int64)
        self.off = lr.offsets_of(lists)
        self.ids = lr.concat(lists)
        self.flat = lr.concat(self.want)
        self.models = models if models is not None else [lr.ef_list(li) if li.size else None for li in self.want]
        self.ql = np.repeat(np.arange(len(lists), dtype=np.uint64), self.sizes)
        self.qo = np.arange(self.flat.size, dtype=np.uint64) - np.repeat(self.off[:-1], self.sizes)


def data(name, route):
    if (name, route) not in _DATA:
        lists, nbase = lr.object_lists(name, route)
        if name not in _MODELS:  # the model of the object's own lists, computed once for the four routes
            _MODELS[name] = [lr.ef_list(li) if li.size else None for li in lists[:nbase]]
        extra = [lr.ef_list(np.sort(li)) for li in lists[nbase:]]
        _DATA[name, route] = Data(lists, nbase, _MODELS[name] + extra)
    return _DATA[name, route]


def encode(d, route):
    import torch
    from vector_db_id_compression_amd.codecs import EfLists

    ids = torch.from_numpy(d.ids.view(np.int64)).cuda()
    off = torch.from_numpy(d.off.view(np.int64)).cuda() if route == "dev" else d.off
    return EfLists.encode(off, ids)


def obj(name, route):
    if (name, route) not in _OBJ:
        _OBJ[name, route] = encode(data(name, route), route)
    return _OBJ[name, route]


def check_streams(ef, d, tag):
    """info, sizes and every word of every list against the model -> the exported words per list"""
    info = ef.info()
    assert np.array_equal(info["sizes"], d.sizes), tag
    assert ef.compressed_bytes == lr.ef_sizes(d.want)["compressed_bytes"], tag
    words = []
    for l, m in enumerate(d.models):
        low, high, lb, hb = ef.export(l)
        words.append((low, high))
        if m is None:
            assert (lb, hb, low.size, high.size) == (0, 0, 0, 0), (tag, l)
            continue
        assert (int(info["low_bits"][l]), int(info["universe"][l])) == (m.l, m.u), (tag, l)
        assert (lb, hb) == (m.low_nbits, m.high_nbits), (tag, l)
        assert np.array_equal(low, m.low), (tag, l, "low words")
        assert np.array_equal(high, m.high), (tag, l, "high words")
    return words


def check_every_position(ef, d, tag):
    got = ef.get(d.ql, d.qo)
    assert np.array_equal(got, d.flat.view(np.int64)), (tag, "get", np.flatnonzero(got != d.flat.view(np.int64))[:8])


def decoded(ef):
    return ef.decode_all().cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("name,route", CASES)
def test_streams_equal_the_model_word_for_word(name, route):
    d = data(name, route)
    assert lr.encoder_form(d.lists) == {"wide": "wide", "unsorted": "general"}.get(route, name.split("_")[0])
    words = check_streams(obj(name, route), d, (name, route))
    # the object's own lists written by the host-offset, device-offset, 64-bit and three-pass encoders: the same words
    if "host" not in _WORDS.setdefault(name, {}):
        _WORDS[name]["host"] = words if route == "host" else check_streams(obj(name, "host"), data(name, "host"), (name, "host"))
    for l in range(d.nbase):
        for a, b in zip(words[l], _WORDS[name]["host"][l]):
            assert np.array_equal(a, b), (name, route, l)


@pytest.mark.parametrize("name,route", CASES)
def test_decode_all_with_encoder_records_lazy_records_and_dirty_pool_blocks(name, route, monkeypatch):
    from vector_db_id_compression_amd import _lib

    d = data(name, route)
    monkeypatch.delenv("VIDC_EF_LAZY_RECS", raising=False)
    ef = encode(d, route)  # (a fresh object: its first decode_all)
    assert np.array_equal(decoded(ef), d.flat), "records from the encoder"
    assert np.array_equal(decoded(ef), d.flat), "second call"
    monkeypatch.setenv("VIDC_EF_LAZY_RECS", "1")
    lazy = encode(d, route)
    assert np.array_equal(decoded(lazy), d.flat), "records built by the first decode_all"
    assert np.array_equal(decoded(lazy), d.flat), "second call"
    monkeypatch.delenv("VIDC_EF_LAZY_RECS")
    ctx = _lib.default_context()
    ctx.set_pool_poison(True)  # every block the pool hands out is filled with 0xFF: nothing clears the high stream beforehand
    try:
        dirty = encode(d, route)
        out = decoded(dirty)
        words = check_streams(dirty, d, (name, route, "poisoned pool"))
        again = decoded(encode(d, route))  # (blocks released by the first poisoned pass, poisoned again)
    finally:
        ctx.set_pool_poison(False)
    assert np.array_equal(out, d.flat) and np.array_equal(again, d.flat) and len(words) == len(d.lists)


@pytest.mark.parametrize("name,route", CASES)
def test_decode_lists(name, route):
    d = data(name, route)
    ef = obj(name, route)
    nlist = len(d.lists)
    longest = np.argsort(d.sizes)[::-1][:3]
    empties = np.flatnonzero(d.sizes == 0)
    reqs = [np.arange(nlist), longest, longest[:2],
            np.concatenate([longest[:1], empties[:2], longest[:2], [1, 1, nlist - 1], empties[-1:], np.arange(nlist)[::-5]])]
    for req in reqs:
        got, goff = ef.decode_lists(np.asarray(req, dtype=np.uint64))
        got = got.cpu().numpy().view(np.uint64)
        assert np.array_equal(goff, lr.offsets_of([d.want[int(l)] for l in req])), (name, route)
        assert np.array_equal(got, lr.concat([d.want[int(l)] for l in req])), (name, route, list(req[:4]))


@pytest.mark.parametrize("name,route", CASES)
def test_get_at_every_position(name, route):
    check_every_position(obj(name, route), data(name, route), (name, route))


@pytest.mark.parametrize("name,route", CASES)
def test_translate_labels_at_every_position_mixed_with_invalid_ones(name, route):
    import torch

    d = data(name, route)
    lab = lr.all_labels(d.sizes, np.random.default_rng(5))
    want, n_invalid = lr.expect_labels(lab, d.sizes, d.flat)
    invalid = torch.zeros(1, dtype=torch.int64, device="cuda")
    got = obj(name, route).translate_labels(torch.from_numpy(lab).cuda(), invalid=invalid).cpu().numpy()
    assert np.array_equal(got, want), (name, route, np.flatnonzero(got != want)[:8])
    assert int(invalid.item()) == n_invalid


@pytest.mark.parametrize("name,route", CASES)
def test_decode_gather_at_every_position(name, route):
    d = data(name, route)
    ne = np.flatnonzero(d.sizes)
    slot_of = np.zeros(len(d.lists), dtype=np.int64)
    slot_of[ne] = np.arange(ne.size)
    p = np.random.default_rng(6).permutation(d.flat.size)
    got = obj(name, route).decode_gather(ne, slot_of[d.ql.astype(np.int64)][p], d.qo[p])
    assert np.array_equal(got, d.flat.view(np.int64)[p]), (name, route)


@pytest.mark.parametrize("name,route", CASES)
def test_loaded_object_answers_like_the_model(name, route, tmp_path):
    """save -> load: the streams travel, the select directory is rebuilt from the high stream (k_ef_hrank_from_high)"""
    from vector_db_id_compression_amd.codecs import EfLists

    d = data(name, route)
    obj(name, route).save(tmp_path / "ef.npz")
    ef = EfLists.load(tmp_path / "ef.npz")
    check_streams(ef, d, (name, route, "loaded"))
    assert np.array_equal(decoded(ef), d.flat)
    check_every_position(ef, d, (name, route, "loaded"))


@pytest.mark.parametrize("name", ["short", "half", "full_seams"])
def test_append_creates_a_run_a_chunk_seam_and_a_list_of_4097_ids(name):
    """One append per encoder form, compared with the model of the merged lists: a constant run that grows across a word (63 -> 65
    copies) and one that starts in an empty list; (half, full) the ids 1, 3, 5, ... of a chunk-seam list merged into the ids 0, 2, 4,
    ...; (full) a list of 4096 ids and a run of 4096 zeros that grow to 4097.  The short object stays short, so it gets the runs."""
    import torch

    rng = np.random.default_rng(11)
    lists, _ = lr.object_lists(name, "host")
    old = list(lists) + [np.full(63, 7, np.uint64), np.zeros(0, np.uint64)]
    run, fresh = len(old) - 2, len(old) - 1
    add = [(run, np.full(2, 7, np.uint64)), (fresh, np.full(64, 5, np.uint64))]
    # a few ids into every ninth list, its largest id among them
    for l in np.flatnonzero([0 < li.size <= 250 or (li.size > 0 and name != "short") for li in lists])[::9]:
        add.append((int(l), np.concatenate([rng.integers(0, int(lists[l][-1]) + 1, 3, dtype=np.uint64), lists[l][-1:]])))
    if name != "short":
        seam = lr.family("chunk_seams")[len(lr.SEAM_IDS) * len(lr.SEAM_KINDS) + 1]  # 1024 ids, id 511 at bit 0, 63 followers
        assert seam.size == 1024
        old.append(seam[::2])
        add.append((len(old) - 1, seam[1::2]))
    if name.startswith("full"):
        old += [np.arange(4096, dtype=np.uint64) * np.uint64(3), np.zeros(4096, np.uint64)]
        add += [(len(old) - 2, lr.u64([6000])), (len(old) - 1, lr.u64([0]))]
    ln = np.concatenate([np.full(x.size, l, np.int64) for l, x in add])
    ids = np.concatenate([x for _, x in add])
    p = rng.permutation(ln.size)
    ln, ids = ln[p], ids[p]
    merged = [np.sort(np.concatenate([li] + [x for l, x in add if l == k])) for k, li in enumerate(old)]
    d0, d1 = Data(old, len(old)), Data(merged, len(merged))
    assert lr.encoder_form(merged) == name.split("_")[0]
    assert d1.sizes[run] == 65 and d1.sizes[fresh] == 64 and (not name.startswith("full") or 4097 in d1.sizes)
    ef0 = encode(d0, "host")
    ef1, lab = ef0.append(torch.from_numpy(ln).cuda(), torch.from_numpy(ids.view(np.int64)).cuda())
    check_streams(ef1, d1, (name, "appended"))
    check_every_position(ef1, d1, (name, "appended"))
    assert np.array_equal(decoded(ef1), d1.flat)
    lab = lab.cpu().numpy()
    assert np.array_equal(lab >> 32, ln)
    assert np.array_equal(d1.flat[(d1.off[ln].astype(np.int64) + (lab & 0xFFFFFFFF))], ids)  # the label names the id's place
    check_streams(ef0, d0, (name, "the old object is unchanged"))
