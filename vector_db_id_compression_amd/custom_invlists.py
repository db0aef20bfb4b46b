"""Drop-in counterpart of the reference's `custom_invlists` SWIG module (custom_invlist_cpp/custom_invlists.swig).

Same class names, constructor signatures (`Cls(invlists)`, wavelet tree with `wt_type`), methods
(`list_size`, `get_codes`, `get_ids`, `get_single_id`, `release_ids`) and public attributes
(`compressed_ids_size_in_bytes`, `overhead_in_bytes`, `codes_size_in_bytes`, `bits`, `wt_type`,
`id_symbol_precision`) as custom_invlists_impl.h:22-124.  The compressed ids live in HBM behind the
C-ABI; the vector codes are kept (re-ordered where the reference re-orders them) in a device tensor.

Beyond the reference's one-list-at-a-time virtuals, the containers expose the batched entry points the
GPU wants: `decode_lists(list_nos)` (replaces the OpenMP loop over touched lists,
custom_invlists_impl.cpp:508-525) and `get_single_ids(list_nos, offsets)` (:466-475).
"""
import numpy as np

from . import _lib
from .codecs import EfLists, PackedLists, RocLists, RocSegLists, WaveletTreeLists
from .invlists import to_csr


def _torch():
    import torch

    return torch


class InvertedListsArrayCodes:
    """custom_invlists_impl.h:22-33: nlist / code_size / codes_all + list_size / get_codes."""

    def __init__(self, il):
        self.nlist = int(il.nlist)
        self.code_size = int(il.code_size)
        self._offsets, self._ids_host, codes = to_csr(il)
        self._codes_src = codes  # uint8 [ntotal, code_size] in the source order
        self.codes_all = None    # device uint8 [ntotal, code_size] in the container's order
        self.ntotal = int(self._offsets[-1])

    def _store_codes(self, perm_local=None):
        """codes_all[offsets[l] + i] = source code at position perm_local[offsets[l] + i] of list l."""
        torch = _torch()
        codes = self._codes_src
        if perm_local is not None and self.code_size:
            base = np.repeat(self._offsets[:-1].astype(np.int64), (self._offsets[1:] - self._offsets[:-1]).astype(np.int64))
            codes = codes[base + perm_local.astype(np.int64)]
        self.codes_all = torch.from_numpy(np.ascontiguousarray(codes)).cuda()
        self._codes_src = None

    def list_size(self, list_no):
        return int(self._offsets[list_no + 1] - self._offsets[list_no])

    def get_codes(self, list_no):
        a, b = int(self._offsets[list_no]), int(self._offsets[list_no + 1])
        return self.codes_all[a:b]

    def get_single_code(self, list_no, offset):
        return self.codes_all[int(self._offsets[list_no]) + int(offset)]

    def release_codes(self, list_no, codes):
        pass

    def release_ids(self, list_no, ids):  # buffers are Python-owned; the reference does delete[] (:116-118)
        pass

    def compute_ntotal(self):
        return self.ntotal

    # ReadOnlyInvertedLists: mutators throw (custom_invlists_impl.cpp:19-20)
    def add_entries(self, *a, **k):
        raise RuntimeError("not implemented: read-only inverted lists")

    update_entries = resize = add_entries

    # -- growth: the one mutator these containers have.  add_entries / update_entries / resize above keep mirroring the reference's
    # read-only virtuals; a batch of (list number, id, code) triples from a coarse quantizer on the GPU goes through the codec's append.
    def _append_ids(self, list_nos, ids, invalid):
        """-> (new codec object, labels, permutation over the merged lists as a host array or None)"""
        raise NotImplementedError

    def _refresh_sizes(self):
        """the public size attributes, as a fresh container over the same lists reports them"""
        raise NotImplementedError

    def add_batch(self, list_nos, ids, codes=None):
        """Append a batch: list_nos int64 [n] (negative = not assigned, skipped), ids int64 [n], codes uint8 [n, code_size]; CUDA
        tensors (numpy arrays are uploaded).  Entry i goes behind the entries of list list_nos[i], in batch order (what add_entries per
        list does to an ArrayInvertedLists).  The compressed ids are appended by the codec (vidc_*_append_dev: a new object replaces
        `self._c`), codes_all is rebuilt on the device in the new object's order, and the size attributes become what a fresh
        container over the same lists reports.  Returns the labels (list_no << 32 | offset, int64 CUDA tensor) of the batch."""
        torch = _torch()
        as_dev = lambda x, dt: (torch.from_numpy(np.ascontiguousarray(x)).cuda() if isinstance(x, np.ndarray) else x).to(dt).reshape(-1)
        ln, di = as_dev(list_nos, torch.int64).contiguous(), as_dev(ids, torch.int64).contiguous()
        n = ln.numel()
        if di.numel() != n:
            raise ValueError("list_nos and ids must have one entry per vector")
        cs = self.code_size
        if cs:
            if codes is None:
                raise ValueError("this container keeps codes: add_batch needs them")
            codes = as_dev(codes, torch.uint8).reshape(n, cs)
        invalid = torch.zeros(1, dtype=torch.int64, device=ln.device)
        new_c, labels, perm = self._append_ids(ln, di, invalid)
        if int(invalid.item()):
            raise _lib.VidcError(f"add_batch: {int(invalid.item())} list numbers are >= nlist = {self.nlist}")
        valid = ln >= 0
        lv = ln[valid]
        add_cnt = torch.bincount(lv, minlength=self.nlist)
        old_off = torch.from_numpy(self._offsets.astype(np.int64)).to(ln.device)
        new_off = old_off + torch.cat([add_cnt.new_zeros(1), torch.cumsum(add_cnt, 0)])
        ntotal_new = int(new_off[-1].item())
        if cs:
            lists = torch.arange(self.nlist, device=ln.device)
            new_codes = torch.empty((ntotal_new, cs), dtype=torch.uint8, device=ln.device)
            old_n = old_off[1:] - old_off[:-1]
            if perm is None:  # input-order containers: the old codes keep their offsets, the batch codes go behind them
                l_old = torch.repeat_interleave(lists, old_n)
                new_codes[torch.arange(self.ntotal, device=ln.device) + (new_off - old_off)[l_old]] = self.codes_all
            else:  # re-ordering containers: position q of list l holds entry perm[q] of the merged input; entries < |old_l| are old ones
                l_new = torch.repeat_interleave(lists, new_off[1:] - new_off[:-1])
                j = torch.from_numpy(perm.astype(np.int64)).to(ln.device)
                is_old = j < old_n[l_new]
                new_codes[is_old] = self.codes_all[(old_off[l_new] + j)[is_old]]
            new_codes[new_off[lv] + (labels[valid] & 0xFFFFFFFF)] = codes[valid]
            self.codes_all = new_codes
        self._c = new_c
        self._offsets = new_off.cpu().numpy().astype(np.uint64)
        self.ntotal = ntotal_new
        self._refresh_sizes()
        return labels

    # -- shrinkage: the counterpart of add_batch.  The compressed ids go through the codec's remove (vidc_*_remove_dev).
    _reorders = False  # the container keeps its codes in the order of the codec's permutation (ROC: sampling order)

    def remove_batch(self, list_nos, ids):
        """Remove a batch: entry of list l leaves iff (l, id) is a pair of the batch; list_nos=None removes the ids from every list
        (Faiss's remove_ids over an IDSelectorBatch).  list_nos int64 [n] (negative = skipped), ids int64 [n]; CUDA tensors (numpy
        arrays are uploaded).  A new codec object replaces `self._c`, codes_all loses the same rows on the device (and follows the
        new permutation of the lists the codec re-ordered), and the size attributes become what a fresh container over the
        surviving lists reports -- packed bits keeps its width: the surviving ids still need it.  Returns the number removed."""
        from . import removal

        torch = _torch()
        as_dev = lambda x, dt: (torch.from_numpy(np.ascontiguousarray(x)).cuda() if isinstance(x, np.ndarray) else x).to(dt).reshape(-1)
        di = as_dev(ids, torch.int64).contiguous()
        ln = None if list_nos is None else as_dev(list_nos, torch.int64).contiguous()
        if ln is not None and ln.numel() != di.numel():
            raise ValueError("list_nos and ids must have one entry per pair")
        invalid = torch.zeros(1, dtype=torch.int64, device=di.device)
        want = self._reorders and self.code_size > 0
        new_c, mask = removal.remove(self._c, ln, di, want_perm=want or self._keeps_perm(), invalid=invalid)
        if int(invalid.item()):
            raise _lib.VidcError(f"remove_batch: {int(invalid.item())} list numbers are >= nlist = {self.nlist}")
        gone = torch.cat([mask.new_zeros(1, dtype=torch.int64), torch.cumsum(mask.to(torch.int64), 0)])
        n_removed = int(gone[-1].item())
        if not n_removed:
            return 0
        old_off = torch.from_numpy(self._offsets.astype(np.int64)).to(di.device)
        new_off = old_off - gone[old_off]
        if self.code_size:
            codes = self.codes_all[mask == 0]
            if want:  # position q of list l holds survivor perm[q] of that list
                sizes = new_off[1:] - new_off[:-1]
                base = torch.repeat_interleave(new_off[:-1], sizes)
                codes = codes[base + torch.from_numpy(new_c.perm().astype(np.int64)).to(di.device)]
            self.codes_all = codes
        self._c = new_c
        self._offsets = new_off.cpu().numpy().astype(np.uint64)
        self.ntotal -= n_removed
        self._n_removed = getattr(self, "_n_removed", 0) + n_removed
        self._refresh_sizes()
        return n_removed

    def _keeps_perm(self):
        """whether a fresh constructor keeps the codec's permutation (the new object then does as well)"""
        return False

    # -- union: two containers over the same lists become one.  The compressed ids go through the codec's merge (vidc_*_merge_dev).
    def _merge_args(self, other):
        """the codec arguments of merge.merge for this container"""
        return {}

    def merge_from(self, other, add_id=0):
        """Faiss's InvertedLists::merge_from(other, add_id): every list of `other` goes behind the same list of this container, add_id
        added to its ids.  `other` is a container of the same class, list count and code size (it may be this one).  A new codec
        object replaces `self._c` (merge.merge), codes_all is rebuilt with one gather through the merge's `src`, and offsets, ntotal
        and the size attributes become what a fresh container over the merged lists reports.  `other` is left unchanged -- Faiss
        empties it; a caller that wants that drops its reference."""
        from . import merge

        if type(other) is not type(self):
            raise TypeError(f"merge_from: {type(other).__name__} is not a {type(self).__name__}")
        if other.nlist != self.nlist or other.code_size != self.code_size:
            raise ValueError(f"merge_from: nlist / code_size differ ({other.nlist} / {other.code_size} against {self.nlist} / {self.code_size})")
        torch = _torch()
        n_a, n_b = self.ntotal, other.ntotal
        src = torch.empty(n_a + n_b, dtype=torch.int64, device="cuda")
        new_c = merge.merge(self._c, other._c, int(add_id), src=src, **self._merge_args(other))
        if self.code_size:
            rows = torch.where(src >= 0, src, n_a + ~src)
            self.codes_all = torch.cat([self.codes_all, other.codes_all])[rows]
        self._c = new_c
        self._offsets = (self._offsets.astype(np.uint64) + other._offsets.astype(np.uint64)).astype(np.uint64)
        self.ntotal = n_a + n_b
        # (vectors ever added = those of both sides, also when other is this container: what _merge_args sized the width by)
        self._n_removed = getattr(self, "_n_removed", 0) + getattr(other, "_n_removed", 0)
        self._refresh_sizes()

    # -- split: the inverse of merge_from.  The compressed ids go through the codec's subset (vidc_*_subset_dev).
    def copy_subset_to(self, other, subset_type, a1, a2):
        """Faiss's InvertedLists::copy_subset_to(other, subset_type, a1, a2): the entries of every list that the rule takes
        (subset.ID_RANGE .. subset.INVLIST, see subset.subset) go behind the same list of `other`, ids unchanged -> the number added.
        `other` is a container of the same class, list count and code size.  The subset is built as a codec object of its own
        (subset.subset), its codes are the rows of codes_all the mask names (following the new permutation where the container
        re-orders, as remove_batch does), and both are merged into `other` with other.merge_from(<the subset as a container>, 0).
        This container is left unchanged.  The positions of ELEMENT_RANGE and INVLIST_FRACTION are those of the container's own
        order (ROC: sampling order; Elias-Fano: ascending), which need not be the order the entries were added in."""
        from . import subset

        if type(other) is not type(self):
            raise TypeError(f"copy_subset_to: {type(other).__name__} is not a {type(self).__name__}")
        if other.nlist != self.nlist or other.code_size != self.code_size:
            raise ValueError(f"copy_subset_to: nlist / code_size differ ({other.nlist} / {other.code_size} against {self.nlist} / {self.code_size})")
        torch = _torch()
        want = self._reorders and self.code_size > 0
        sub_c, mask = subset.subset(self._c, subset_type, a1, a2, want_perm=want or self._keeps_perm())
        part = type(self).__new__(type(self))  # the subset as a container over the same lists: what merge_from reads
        part.__dict__.update({k: v for k, v in self.__dict__.items() if k not in ("_c", "codes_all", "_offsets", "ntotal", "_n_removed")})
        taken = torch.cat([mask.new_zeros(1, dtype=torch.int64), torch.cumsum(mask.to(torch.int64), 0)])
        old_off = torch.from_numpy(self._offsets.astype(np.int64)).to(mask.device)
        new_off = taken[old_off]
        n_taken = int(new_off[-1].item())
        codes = None
        if self.code_size:
            codes = self.codes_all[mask == 1]
            if want:  # position q of list l holds taken entry perm[q] of that list
                sizes = new_off[1:] - new_off[:-1]
                base = torch.repeat_interleave(new_off[:-1], sizes)
                codes = codes[base + torch.from_numpy(sub_c.perm().astype(np.int64)).to(mask.device)]
        part._c, part.codes_all = sub_c, codes
        part._offsets = new_off.cpu().numpy().astype(np.uint64)
        part.ntotal = n_taken
        # (the ids of the part were handed out among the vectors ever added here: the width of a merged packed-bits container covers them)
        part._n_removed = self.ntotal + getattr(self, "_n_removed", 0) - n_taken
        other.merge_from(part, 0)
        return n_taken

    # -- batched helpers shared by the subclasses
    def get_single_id(self, list_no, offset):
        return int(self.get_single_ids([list_no], [offset])[0])

    def get_ids(self, list_no):
        """numpy int64 array of the ids of one list (empty list -> None like the reference's nullptr, :212-214)."""
        if self.list_size(list_no) == 0:
            return None
        ids, _ = self.decode_lists([list_no])
        return ids.cpu().numpy()

    def get_ids_all(self):
        """Every list decoded on the device: int64 CUDA tensor in CSR order."""
        raise NotImplementedError

    def decode_gather(self, list_nos, item_slot, item_off):
        """The decode section of the deferred search in one library call (custom_invlists_impl.cpp:508-525): ids of the
        (slot in list_nos, offset) items, picked on the device; numpy int64."""
        return self._c.decode_gather(np.asarray(list_nos, dtype=np.uint64), item_slot, item_off)

    def translate_labels(self, labels, out=None, invalid=None):
        """Faiss labels of a search (int64 CUDA tensor, list_no << 32 | offset) -> ids, on the device, in place when out is labels:
        the loop of custom_invlists_impl.cpp:508-525 for a caller whose labels come from a GPU top-k (codec translate_labels)."""
        return self._c.translate_labels(labels, out=out, invalid=invalid)

    def locate_batch(self, list_nos, ids):
        """The inverse of translate_labels, Faiss's direct map (locate.locate on the codec): labels (int64 CUDA tensor, list_no << 32 |
        offset, -1 = not found) of the ids; list_nos=None looks in every list, else id i is looked for in list list_nos[i] only.  The
        offsets are positions in the container's own order: row offsets[list_no] + offset of codes_all is the id's code."""
        from . import locate

        return locate.locate(self._c, list_nos, ids)


class CompressedIDInvertedListsPackedBits(InvertedListsArrayCodes):
    """custom_invlists_impl.cpp:64-118."""

    def __init__(self, il):
        super().__init__(il)
        ids = self._ids_host
        if ids.size and int(ids.max()) >= self.ntotal:  # FAISS_THROW_IF_NOT(ids_in[i] >= 0 && ids_in[i] < ntotal), :87
            raise _lib.VidcError("Error: 'ids_in[i] >= 0 && ids_in[i] < ntotal' failed")
        self._c = PackedLists.encode(self._offsets, ids, bits=PackedLists.bits_for(self.ntotal))
        self._refresh_sizes()
        self._store_codes()
        self._ids_host = None

    def _refresh_sizes(self):
        self.bits = self._c.bits
        self.compressed_ids_size_in_bytes = self._c.compressed_bytes

    def _append_ids(self, list_nos, ids, invalid):
        # the width a fresh container takes for the grown index (:68-70); an id that does not fit it fails as the constructor does (:87)
        # (ids handed out after a removal continue from the number of vectors ever added: the width covers those)
        ntotal_new = self.ntotal + getattr(self, "_n_removed", 0) + int((list_nos >= 0).sum().item())
        new_c, labels = self._c.append(list_nos, ids, bits=PackedLists.bits_for(ntotal_new), invalid=invalid)
        return new_c, labels, None

    def _merge_args(self, other):
        # the width a fresh container takes for the merged index (:68-70), over the vectors ever added on both sides (see _append_ids)
        return dict(bits=PackedLists.bits_for(self.ntotal + other.ntotal + getattr(self, "_n_removed", 0) + getattr(other, "_n_removed", 0)))

    def get_ids_all(self):
        return self._c.decode_all()

    def decode_lists(self, list_nos):
        return self._c.decode_lists(np.asarray(list_nos, dtype=np.uint64))  # work ~ the requested lists (:96-105)

    def get_single_ids(self, list_nos, offsets):
        return self._c.get(list_nos, offsets)


class CompressedIDInvertedListsFenwickTree(InvertedListsArrayCodes):
    """ROC / bits-back ANS container (custom_invlists_impl.cpp:133-223); the name is the reference's."""

    def __init__(self, il):
        super().__init__(il)
        self._c = RocLists.encode(self._offsets, self._ids_host, want_perm=self.code_size > 0)
        self.overhead_in_bytes = 0                                   # declared, never written (:62)
        # codes are re-ordered into sampling order (:188-193)
        self._store_codes(self._c.perm() if self.code_size else None)
        self._refresh_sizes()
        self._ids_host = None

    def _refresh_sizes(self):
        info = self._c.info()
        self.id_symbol_precision = info["precision"].astype(np.uint64)
        self.compressed_ids_size_in_bytes = self._c.compressed_bytes  # :196-206
        # the reference adds the size of ALL code arrays once per non-empty list (:203-205, accidental O(nlist^2))
        nonempty = int(np.count_nonzero(self._offsets[1:] > self._offsets[:-1]))
        self.codes_size_in_bytes = nonempty * self.ntotal * self.code_size

    _reorders = True

    def _append_ids(self, list_nos, ids, invalid):
        want = self.code_size > 0
        new_c, labels = self._c.append(list_nos, ids, want_perm=want, invalid=invalid)  # (the constructor's precision mode)
        return new_c, labels, (new_c.perm() if want else None)

    def _merge_args(self, other):
        return dict(want_perm=self.code_size > 0)  # (the constructor's precision mode)

    def get_ids_all(self):
        return self._c.decode_all()

    def decode_lists(self, list_nos):
        return self._c.decode_lists(np.asarray(list_nos, dtype=np.uint64))

    def get_single_ids(self, list_nos, offsets):
        # not overridden in the reference: InvertedLists::get_single_id = get_ids()[offset]
        # (one library call: the touched lists are decoded and indexed on the device, 8 bytes per result come back)
        ln = np.asarray(list_nos, dtype=np.uint64)
        uniq, inv = np.unique(ln, return_inverse=True)
        return self._c.decode_gather(uniq, inv, offsets)


class CompressedIDInvertedListsEliasFano(InvertedListsArrayCodes):
    """custom_invlists_impl.cpp:229-339."""

    def __init__(self, il):
        super().__init__(il)
        self._c = EfLists.encode(self._offsets, self._ids_host, want_perm=self.code_size > 0)
        self.overhead_in_bytes = 0
        self._store_codes(self._c.perm() if self.code_size else None)  # canonicalize_order_inplace, :324-339
        self._refresh_sizes()
        self._ids_host = None

    def _refresh_sizes(self):
        self.compressed_ids_size_in_bytes = self._c.compressed_bytes  # :272-282
        nonempty = int(np.count_nonzero(self._offsets[1:] > self._offsets[:-1]))
        self.codes_size_in_bytes = nonempty * self.ntotal * self.code_size

    def _keeps_perm(self):
        return self.code_size > 0  # (the survivors of an ascending list are ascending: the permutation is the identity)

    def _append_ids(self, list_nos, ids, invalid):
        want = self.code_size > 0
        new_c, labels = self._c.append(list_nos, ids, want_perm=want, invalid=invalid)
        return new_c, labels, (new_c.perm() if want else None)

    def _merge_args(self, other):
        return dict(want_perm=self.code_size > 0)

    def get_ids_all(self):
        return self._c.decode_all()

    def decode_lists(self, list_nos):
        return self._c.decode_lists(np.asarray(list_nos, dtype=np.uint64))

    def get_single_ids(self, list_nos, offsets):
        return self._c.get(list_nos, offsets)

    def rank_batch(self, list_nos, ids):
        """How many ids of list list_nos[i] are smaller than ids[i] (rank.rank on the codec: searched in the compressed lists, nothing is
        decoded): int64 CUDA tensor, -1 for a negative or too large list number.  The rank is the offset of the first id >= ids[i] in the
        container's own order: row offsets[list_no] + rank of codes_all is the successor's code."""
        from . import rank

        return rank.rank(self._c, list_nos, ids)

    def contains_batch(self, list_nos, ids):
        """Is ids[i] in list list_nos[i]? -> bool CUDA tensor (rank.contains on the codec)."""
        from . import rank

        return rank.contains(self._c, list_nos, ids)


class CompressedIDInvertedListsWaveletTree(InvertedListsArrayCodes):
    """custom_invlists_impl.cpp:346-397; wt_type 0 = bit_vector levels, 1 = rrr_vector<63> levels."""

    def __init__(self, il, wt_type=0):
        super().__init__(il)
        assert wt_type in (0, 1)
        self.wt_type = wt_type
        self._c = WaveletTreeLists.build(self._offsets, self._ids_host, wt_type)
        self._refresh_sizes()
        self._store_codes()
        self._ids_host = None

    def _refresh_sizes(self):
        self.compressed_ids_size_in_bytes = self._c.size_in_bytes

    def _append_ids(self, list_nos, ids, invalid):
        new_c, labels = self._c.append(list_nos, ids, invalid=invalid)
        return new_c, labels, None

    def remove_batch(self, list_nos, ids):
        raise RuntimeError("not implemented: a wavelet tree holds a permutation of 0 .. ntotal - 1, which a removal breaks")

    def copy_subset_to(self, other, subset_type, a1, a2):
        raise RuntimeError("not implemented: a wavelet tree holds a permutation of 0 .. ntotal - 1, which a subset breaks: no copy_subset_to")

    def _merge_args(self, other):
        if other.wt_type != self.wt_type:
            raise ValueError(f"merge_from: wt_type differs ({other.wt_type} against {self.wt_type})")
        return {}

    def get_ids_all(self):
        return self._c.decode_all()

    def decode_lists(self, list_nos):
        return self._c.decode_lists(np.asarray(list_nos, dtype=np.uint64))  # get_ids loops get_single_id (:381-392)

    def get_single_ids(self, list_nos, offsets):
        return self._c.select(list_nos, offsets)


class CompressedIDInvertedListsROCSegmented(InvertedListsArrayCodes):
    """ROC with parallel chains inside a list (vidc_rocseg, include/vidc.h): the surface of the FenwickTree container over a RocSegLists.
    Long lists are cut by value range into segments of about `seg_ids` ids (None: the library's default), so a deferred search decodes
    only the segments its labels touch.  Not a reference container (it is not in AVAILABLE_COMPRESSED_IVFS): the streams are not the
    reference's, and add_batch / remove_batch are out of scope."""

    def __init__(self, il, seg_ids=None):
        super().__init__(il)
        self.seg_ids = seg_ids
        self._c = RocSegLists.encode(self._offsets, self._ids_host, seg_ids=seg_ids, want_perm=self.code_size > 0)
        self.overhead_in_bytes = 0
        self._store_codes(self._c.perm() if self.code_size else None)  # codes follow the decode order, as in the FenwickTree container
        self._refresh_sizes()
        self._ids_host = None

    def _refresh_sizes(self):
        self.id_symbol_precision = self._c.inner.info()["precision"].astype(np.uint64)  # per SEGMENT
        self.compressed_ids_size_in_bytes = self._c.compressed_bytes  # the inner object's + 4 bytes per segment of a split list
        nonempty = int(np.count_nonzero(self._offsets[1:] > self._offsets[:-1]))
        self.codes_size_in_bytes = nonempty * self.ntotal * self.code_size

    def add_batch(self, list_nos, ids, codes=None):
        raise RuntimeError("not implemented: segmented ROC lists have no append (re-encode, or use the FenwickTree container)")

    def remove_batch(self, list_nos, ids):
        raise RuntimeError("not implemented: segmented ROC lists have no remove (re-encode, or use the FenwickTree container)")

    def locate_batch(self, list_nos, ids):
        raise RuntimeError("not implemented: segmented ROC lists have no locate (use the FenwickTree container)")

    def merge_from(self, other, add_id=0):
        raise RuntimeError("not implemented: segmented ROC lists have no merge (re-encode, or use the FenwickTree container)")

    def copy_subset_to(self, other, subset_type, a1, a2):
        raise RuntimeError("not implemented: segmented ROC lists have no copy_subset_to (re-encode, or use the FenwickTree container)")

    def get_ids_all(self):
        return self._c.decode_all()

    def decode_lists(self, list_nos):
        return self._c.decode_lists(np.asarray(list_nos, dtype=np.uint64))

    def get_single_ids(self, list_nos, offsets):
        ln = np.asarray(list_nos, dtype=np.uint64)
        uniq, inv = np.unique(ln, return_inverse=True)
        return self._c.decode_gather(uniq, inv, offsets)


AVAILABLE_COMPRESSED_IVFS = {  # bench_invlists.py:19-25
    "elias-fano": CompressedIDInvertedListsEliasFano,
    "roc": CompressedIDInvertedListsFenwickTree,
    "packed-bits": CompressedIDInvertedListsPackedBits,
    "wavelet-tree": CompressedIDInvertedListsWaveletTree,
    "ref": None,  # must be last
}


def search_IVF_defer_id_decoding(index, x, k, decode_1by1=False, return_codes=0):
    """custom_invlists.swig:92-122 / custom_invlists_impl.cpp:407-526 on an `ivf.IVFIndex`."""
    return index.search_defer_id_decoding(x, k, decode_1by1=decode_1by1, return_codes=return_codes)


ID_COMPRESSION_CHOICES = "none packed-bits elias-fano roc wavelet-tree wavelet-tree-1".split()  # search_ivf_qinco.py:384-388


def apply_id_compression(index, id_compression):
    """The `--id_compression` switch of the reference's large-scale driver (search_ivf_qinco.py:502-523): build the chosen
    container from `index.invlists`, install it with `replace_invlists(il, False)` and return
    (il, {"compressed_ids_size_in_bytes": ..., "id_compression_time": ...})."""
    import time

    if id_compression == "none":
        return index.invlists, {}
    t0 = time.time()
    if id_compression == "packed-bits":
        il = CompressedIDInvertedListsPackedBits(index.invlists)
    elif id_compression == "elias-fano":
        il = CompressedIDInvertedListsEliasFano(index.invlists)
    elif id_compression == "roc":
        il = CompressedIDInvertedListsFenwickTree(index.invlists)
    elif id_compression == "wavelet-tree":
        il = CompressedIDInvertedListsWaveletTree(index.invlists)
    elif id_compression == "wavelet-tree-1":
        il = CompressedIDInvertedListsWaveletTree(index.invlists, 1)
    else:
        raise ValueError(f"id_compression must be one of {ID_COMPRESSION_CHOICES}")
    t1 = time.time()
    index.replace_invlists(il, False)
    return il, {"compressed_ids_size_in_bytes": il.compressed_ids_size_in_bytes, "id_compression_time": t1 - t0}
