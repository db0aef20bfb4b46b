"""A small IVF index used as the *caller* of the ID codecs where Faiss is not installed.

It reproduces the call pattern the reference exercises through Faiss:
  * `search`                      -> scan the probed lists, ids via `invlists.get_ids` of every probed list
                                     (IndexIVF::search_preassigned with store_pairs = false)
  * `search_defer_id_decoding`    -> scan with (list_no << 32 | offset) labels, translate afterwards, either one
                                     by one (`get_single_id`, custom_invlists_impl.cpp:466-475) or per touched list
                                     (`get_ids`, :477-525) -- here as ONE batched device decode
The vector side (k-means, flat / PQ codes, distance scan) is plain torch: it is harness plumbing, not the
product.  Codes: "Flat" (float32 bytes) or ("PQ", M) with 8-bit sub-quantizers (PQ4np / PQ16 style); by_residual=True makes the PQ
code that of (vector - its list's centroid), as faiss.index_factory(d, "IVF<n>,PQ<M>") does.
"""
import numpy as np

from .invlists import ArrayInvertedLists, to_csr


def _torch():
    import torch

    return torch


def _assign(x, c, chunk=1 << 16):
    """argmin_j ||x_i - c_j|| in chunks (keeps the distance matrix small)."""
    torch = _torch()
    out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    for a in range(0, x.shape[0], chunk):
        out[a:a + chunk] = torch.cdist(x[a:a + chunk], c).argmin(1)
    return out


def _kmeans(x, k, iters=10, seed=123):
    torch = _torch()
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    n = x.shape[0]
    perm = torch.randperm(n, generator=g)[:k].to(x.device)
    c = x[perm].clone()
    if c.shape[0] < k:  # fewer points than centroids: pad with jittered copies
        reps = (k + c.shape[0] - 1) // c.shape[0]
        c = c.repeat(reps, 1)[:k] + 1e-3 * torch.arange(k, device=x.device, dtype=x.dtype)[:, None]
    for _ in range(iters):
        a = _assign(x, c)
        sums = torch.zeros_like(c).index_add_(0, a, x)
        cnt = torch.bincount(a, minlength=k).to(x.dtype)[:, None]
        c = torch.where(cnt > 0, sums / cnt.clamp(min=1), c)
    return c


def _host_rows(il, ids):
    """The direct map of uncompressed lists on the host: row of to_csr(il)'s codes for every id (of equal ids the first in list
    order, the smallest label); raises on an id that is not in the lists."""
    want = np.asarray(ids, dtype=np.int64).reshape(-1)
    all_ids = to_csr(il)[1].view(np.int64)
    order = np.argsort(all_ids, kind="stable")
    at = np.searchsorted(all_ids[order], want)
    ok = at < order.size
    ok[ok] = all_ids[order[at[ok]]] == want[ok]
    if not ok.all():
        raise RuntimeError(f"reconstruct_batch: {int((~ok).sum())} ids are not in the index")
    return order[at]


def _host_subset(il, subset_type, a1, a2):
    """the five rules of subset.subset on an ArrayInvertedLists -> one boolean keep array per list (unsigned 64-bit arithmetic)"""
    sizes = [int(x.size) for x in il._ids]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    T = int(off[-1])
    ok = {0: True, 1: a1 >= 1 and a2 < a1, 2: a1 <= a2 <= T, 3: 1 <= a1 < 2 ** 32 and a2 < a1, 4: True}.get(subset_type)
    if ok is None or min(a1, a2) < 0 or max(a1, a2) >> 64:
        raise ValueError(f"copy_subset_to: subset_type {subset_type} is not one of 0 .. 4, or an argument is outside [0, 2^64)")
    if not ok:
        raise ValueError(f"copy_subset_to: subset_type {subset_type} does not take a1 = {a1}, a2 = {a2}")
    keeps = []
    for l, n in enumerate(sizes):
        ids = il._ids[l].view(np.uint64)
        if subset_type == 0:
            keep = (ids >= np.uint64(a1)) & (ids < np.uint64(a2))
        elif subset_type == 1:
            keep = np.array([int(x) % a1 == a2 for x in ids], bool) if n else np.zeros(0, bool)
        else:
            if subset_type == 2:
                o0, o1 = int(off[l]), int(off[l + 1])
                i1, i2 = (o1 * a1 // T - o0 * a1 // T, o1 * a2 // T - o0 * a2 // T) if T else (0, 0)
            elif subset_type == 3:
                i1, i2 = n * a2 // a1, n * (a2 + 1) // a1
            else:
                i1, i2 = (0, n) if a1 <= l < a2 else (0, 0)
            pos = np.arange(n)
            keep = (pos >= i1) & (pos < i2)
        keeps.append(keep)
    return keeps


class IVFIndex:
    def __init__(self, d, nlist, code="Flat", by_residual=False):
        self.d, self.nlist = int(d), int(nlist)
        self.code = code
        self.by_residual = bool(by_residual)
        if self.by_residual and not isinstance(code, tuple):
            raise ValueError("by_residual needs (\"PQ\", M) codes")
        self.nprobe = 1
        self.parallel_mode = 0
        self.centroids = None
        self.pq = None  # [M, 256, dsub]
        self.M = code[1] if isinstance(code, tuple) else 0
        self.code_size = 4 * self.d if code == "Flat" else self.M
        self.invlists = ArrayInvertedLists(self.nlist, self.code_size)
        self.ntotal = 0
        self._next_id = 0  # vectors ever added: ids handed out by add never repeat, also after remove_ids
        self._dev = None

    # -- build
    def train(self, xt):
        torch = _torch()
        xt = torch.as_tensor(np.asarray(xt, dtype=np.float32)).cuda()
        if xt.shape[0] > 200_000:  # like Faiss, train on a subsample
            g = torch.Generator(device="cpu")
            g.manual_seed(99)
            xt = xt[torch.randperm(xt.shape[0], generator=g)[:200_000].to(xt.device)]
        self.centroids = _kmeans(xt, self.nlist)
        if self.M:
            dsub = self.d // self.M
            assert dsub * self.M == self.d
            if self.by_residual:
                xt = xt - self.centroids[_assign(xt, self.centroids)]
            self.pq = torch.stack([_kmeans(xt[:, m * dsub:(m + 1) * dsub], 256, seed=7 + m) for m in range(self.M)])

    def _encode_dev(self, x, assign=None):
        """codes of x as a uint8 CUDA tensor [n, code_size]; assign: the list of every row (by_residual encodes x - centroids[assign])"""
        torch = _torch()
        if not self.M:
            return x.contiguous().view(torch.uint8).reshape(x.shape[0], 4 * self.d)
        if self.by_residual:
            x = x - self.centroids[assign]
        dsub = self.d // self.M
        codes = torch.stack([_assign(x[:, m * dsub:(m + 1) * dsub].contiguous(), self.pq[m]) for m in range(self.M)], 1)
        return codes.to(torch.uint8)

    def _encode(self, x, assign=None):
        return self._encode_dev(x, assign).cpu().numpy()

    def add(self, xb):
        torch = _torch()
        xb = torch.as_tensor(np.asarray(xb, dtype=np.float32)).cuda()
        if hasattr(self.invlists, "add_batch"):  # a compressed container: assignments, ids and codes stay on the device
            n = xb.shape[0]
            ids = torch.arange(self._next_id, self._next_id + n, dtype=torch.int64, device=xb.device)
            assign = _assign(xb, self.centroids)
            self.invlists.add_batch(assign, ids, self._encode_dev(xb, assign))
            self.ntotal += n
            self._next_id += n
            self._dev = None
            return
        assign = _assign(xb, self.centroids)
        codes = self._encode(xb, assign)
        assign = assign.cpu().numpy()
        ids = np.arange(self._next_id, self._next_id + xb.shape[0], dtype=np.int64)
        order = np.argsort(assign, kind="stable")
        bounds = np.searchsorted(assign[order], np.arange(self.nlist + 1))
        for l in range(self.nlist):
            sel = order[bounds[l]:bounds[l + 1]]
            if sel.size:
                self.invlists.add_entries(l, ids[sel], codes[sel])
        self.ntotal += xb.shape[0]
        self._next_id += xb.shape[0]
        self._dev = None

    def remove_ids(self, ids):
        """IndexIVF::remove_ids over an IDSelectorBatch: every entry whose id is in `ids` leaves its list -> the number removed.
        A compressed container removes on the device (remove_batch, any-list mode); ArrayInvertedLists is filtered on the host."""
        il = self.invlists
        if hasattr(il, "remove_batch"):
            n = il.remove_batch(None, ids)
        elif isinstance(il, ArrayInvertedLists):
            sel = np.asarray(ids.cpu() if hasattr(ids, "cpu") else ids, dtype=np.int64).reshape(-1)
            n = 0
            for l in range(il.nlist):
                keep = ~np.isin(il._ids[l], sel)
                n += int(keep.size - keep.sum())
                il._ids[l], il._codes[l] = il._ids[l][keep], il._codes[l][keep]
        else:
            raise RuntimeError("remove_ids: the inverted lists are read-only")
        self.ntotal -= n
        self._dev = None
        return n

    def merge_from(self, other, add_id=None):
        """IndexIVF::merge_from: every list of `other` goes behind the same list of this index, add_id added to its ids (None: the
        number of vectors ever added here, so ids stay distinct).  Both indexes must share d, nlist, code, centroids (and PQ
        codebooks) and the class of their inverted lists.  A compressed container merges on the device (its merge_from);
        ArrayInvertedLists is merged on the host.  `other` is left unchanged (Faiss empties it)."""
        self._check_same_index(other, "merge_from")
        il, ol = self.invlists, other.invlists
        add_id = self._next_id if add_id is None else int(add_id)
        if isinstance(il, ArrayInvertedLists):
            for l in range(il.nlist):
                ids, codes = ol._ids[l] + add_id, ol._codes[l]  # (read before the append: other may be this index)
                if ids.size:
                    il.add_entries(l, ids, codes)
        elif hasattr(il, "merge_from"):
            il.merge_from(ol, add_id)
        else:
            raise RuntimeError("merge_from: the inverted lists are read-only")
        self.ntotal += other.ntotal
        self._next_id = max(self._next_id, add_id + other._next_id)
        self._dev = None

    def _check_same_index(self, other, what):
        if not isinstance(other, IVFIndex):
            raise TypeError(f"{what}: other must be an IVFIndex")
        if (other.d, other.nlist, other.code) != (self.d, self.nlist, self.code):
            raise ValueError(f"{what}: d, nlist or code differ")
        if other.by_residual != self.by_residual:
            raise ValueError(f"{what}: by_residual differs")
        for mine, theirs, name in ((self.centroids, other.centroids, "centroids"), (self.pq, other.pq, "PQ codebooks")):
            if (mine is None) != (theirs is None) or (mine is not None and not _torch().equal(mine, theirs)):
                raise ValueError(f"{what}: the {name} differ")
        if type(self.invlists) is not type(other.invlists):
            raise TypeError(f"{what}: the inverted lists are a {type(self.invlists).__name__} and a {type(other.invlists).__name__}")

    def copy_subset_to(self, other, subset_type, a1, a2):
        """IndexIVF::copy_subset_to: the entries the rule takes (subset.ID_RANGE .. subset.INVLIST, see subset.subset) go behind the
        same lists of `other`, ids unchanged -> the number copied.  The compatibility checks are merge_from's.  A compressed container
        takes the subset on the device (its copy_subset_to); ArrayInvertedLists is filtered on the host by the same five rules.  This
        index is left unchanged."""
        self._check_same_index(other, "copy_subset_to")
        il, ol = self.invlists, other.invlists
        if isinstance(il, ArrayInvertedLists):
            n = 0
            for l, keep in enumerate(_host_subset(il, int(subset_type), int(a1), int(a2))):
                if keep.any():
                    ol.add_entries(l, il._ids[l][keep], il._codes[l][keep])
                    n += int(keep.sum())
        elif hasattr(il, "copy_subset_to"):
            n = il.copy_subset_to(ol, subset_type, a1, a2)
        else:
            raise RuntimeError("copy_subset_to: the inverted lists are read-only")
        other.ntotal += n
        other._next_id = max(other._next_id, self._next_id)
        other._dev = None
        return n

    def reconstruct_batch(self, ids):
        """IndexIVF::reconstruct_batch through the direct map: the stored vectors of `ids` -> float32 CUDA tensor [n, d].  A compressed
        container locates the ids on the device (locate_batch, any-list mode); ArrayInvertedLists is searched on the host.  Raises
        on an id that is not in the index."""
        torch = _torch()
        il = self.invlists
        off, codes = self._device_lists()
        if hasattr(il, "locate_batch"):
            if not hasattr(ids, "is_cuda"):
                ids = torch.from_numpy(np.asarray(ids, dtype=np.int64))
            labels = il.locate_batch(None, ids.to(torch.int64).cuda().reshape(-1))
            absent = int((labels < 0).sum().item())
            if absent:
                raise RuntimeError(f"reconstruct_batch: {absent} ids are not in the index")
            rows = torch.from_numpy(off).to(labels.device)[labels >> 32] + (labels & 0xFFFFFFFF)
        elif isinstance(il, ArrayInvertedLists):
            rows = torch.from_numpy(_host_rows(il, np.asarray(ids.cpu() if hasattr(ids, "cpu") else ids, dtype=np.int64))).cuda()
        else:
            raise RuntimeError("reconstruct_batch: the inverted lists have no direct map")
        vecs = self._decode_codes(codes[rows])
        if self.by_residual:
            vecs = vecs + self.centroids[self._rows_lists(rows)]
        return vecs

    def _rows_lists(self, rows):
        """the list every row of the code array lies in, as an int64 CUDA tensor (the last l with offsets[l] <= row)"""
        torch = _torch()
        off, _ = self._device_lists()
        return torch.searchsorted(torch.from_numpy(off[1:].copy()).to(rows.device), rows, right=True)

    def replace_invlists(self, il, own=False):
        self.invlists = il
        self._dev = None

    # -- device view of the codes of the current invlists
    def _device_lists(self):
        torch = _torch()
        if self._dev is None:
            il = self.invlists
            if getattr(il, "codes_all", None) is not None:  # compressed container: codes already resident
                off, codes = il._offsets, il.codes_all
            else:
                off, _, codes = to_csr(il)
                codes = torch.from_numpy(codes).cuda()
            self._dev = (np.asarray(off, dtype=np.int64), codes)
        return self._dev

    def _decode_codes(self, codes):
        torch = _torch()
        if not self.M:
            return codes.contiguous().view(torch.float32).reshape(-1, self.d)
        dsub = self.d // self.M
        parts = [self.pq[m][codes[:, m].long()] for m in range(self.M)]
        return torch.cat(parts, 1).reshape(-1, dsub * self.M)

    def _scan(self, xq, k):
        """-> D [nq,k] float32, labels [nq,k] int64 = list_no << 32 | offset (-1 when fewer than k candidates)."""
        torch = _torch()
        off, codes = self._device_lists()
        xq = torch.as_tensor(np.asarray(xq, dtype=np.float32)).cuda()
        nq = xq.shape[0]
        probe = torch.cdist(xq, self.centroids).topk(min(self.nprobe, self.nlist), largest=False).indices.cpu().numpy()
        D = np.full((nq, k), np.inf, dtype=np.float32)
        L = np.full((nq, k), -1, dtype=np.int64)
        for q in range(nq):
            rows, labs = [], []
            for l in probe[q]:
                a, b = int(off[l]), int(off[l + 1])
                if b > a:
                    rows.append(torch.arange(a, b, device="cuda"))
                    labs.append((int(l) << 32) + torch.arange(b - a, device="cuda", dtype=torch.int64))
            if not rows:
                continue
            rows, labs = torch.cat(rows), torch.cat(labs)
            vecs = self._decode_codes(codes[rows])
            if self.by_residual:
                vecs = vecs + self.centroids[labs >> 32]
            dist = ((vecs - xq[q][None, :]) ** 2).sum(1)
            kk = min(k, dist.numel())
            top = torch.topk(dist, kk, largest=False, sorted=True)
            D[q, :kk] = top.values.cpu().numpy()
            L[q, :kk] = labs[top.indices].cpu().numpy()
        return D, L

    # -- the scan on the device (vidc_ivf_scan_dev): _scan above stays the baseline
    def _device_offsets(self):
        """(offsets as a uint64-valued int64 CUDA tensor, the ids of plain lists in list order or None): uploaded once and kept for as
        long as the _device_lists view they belong to"""
        torch = _torch()
        off, codes = self._device_lists()
        held = getattr(self, "_dev_off", None)
        if held is None or held[0] is not self._dev:
            ids = None
            if getattr(self.invlists, "codes_all", None) is None:
                ids = torch.from_numpy(to_csr(self.invlists)[1].view(np.int64).copy()).to(codes.device)
            held = self._dev_off = (self._dev, torch.from_numpy(off.astype(np.int64)).to(codes.device), ids)
        return held[1], held[2]

    def scan_device(self, xq, k, probes=None):
        """The scan of _scan as one library call (vidc_ivf_scan_dev): -> (D float32 [nq, k], labels int64 [nq, k] = list_no << 32 |
        offset) as CUDA tensors, +inf / -1 padded, ascending in (distance, label).  probes: an int64 [nq, nprobe] CUDA tensor of list
        numbers, used as it is (-1 = no list); None picks them on the device with the cdist + topk of _scan.  Works over the codes of
        a compressed container and of ArrayInvertedLists, for "Flat" and ("PQ", M), raw or by_residual (the latter through
        vidc_ivf_scan_residual_dev).  Runs on torch's current stream."""
        from . import _lib

        torch = _torch()
        if not torch.cuda.is_available():
            raise _lib.VidcError("no HIP device: scan_device needs an MI355X (there is no CPU fallback)")
        if not (isinstance(xq, torch.Tensor) and xq.is_cuda):
            xq = torch.from_numpy(np.array(xq, dtype=np.float32, order="C")).cuda()
        xq = xq.to(torch.float32).contiguous()
        if xq.dim() != 2 or xq.shape[1] != self.d:
            raise ValueError(f"xq must be [nq, {self.d}]")
        if probes is None:
            probes = torch.cdist(xq, self.centroids).topk(min(self.nprobe, self.nlist), largest=False).indices
        if not (isinstance(probes, torch.Tensor) and probes.is_cuda and probes.dtype == torch.int64 and probes.dim() == 2
                and probes.shape[0] == xq.shape[0]):
            raise ValueError("probes must be an int64 CUDA tensor [nq, nprobe]")
        probes = probes.contiguous()
        _, codes = self._device_lists()
        off, _ = self._device_offsets()
        nq, k = int(xq.shape[0]), int(k)
        if not 0 <= k < 2 ** 32:
            raise ValueError("k is an unsigned 32-bit number")
        D = torch.empty((nq, k), dtype=torch.float32, device=xq.device)
        labels = torch.empty((nq, k), dtype=torch.int64, device=xq.device)
        ptr = _lib.ptr
        pq = self.pq.to(torch.float32).contiguous() if self.M else None
        ctx = _lib.default_context()
        if self.by_residual:
            cent = self.centroids.to(torch.float32).contiguous()
            _lib.check(_lib.lib().vidc_ivf_scan_residual_dev(
                ctx.h, self.nlist, ptr(off), int(codes.shape[0]), ptr(codes) if codes.numel() else None, self.d, self.M, ptr(pq), ptr(cent),
                nq, ptr(xq) if nq else None, int(probes.shape[1]), ptr(probes) if probes.numel() else None, k,
                ptr(D) if D.numel() else None, ptr(labels) if labels.numel() else None, None))
            return D, labels
        _lib.check(_lib.lib().vidc_ivf_scan_dev(
            ctx.h, self.nlist, ptr(off), int(codes.shape[0]), ptr(codes) if codes.numel() else None,
            _lib.VIDC_IVF_PQ8 if self.M else _lib.VIDC_IVF_FLAT, self.d, self.M, ptr(pq) if self.M else None, nq, ptr(xq) if nq else None,
            int(probes.shape[1]), ptr(probes) if probes.numel() else None, k, ptr(D) if D.numel() else None,
            ptr(labels) if labels.numel() else None, None))
        return D, labels

    def search_device(self, xq, k):
        """search_defer_id_decoding with nothing on the host: scan_device, then the labels -> ids on the device (translate_labels of
        a compressed container; one gather of the ids of plain lists).  -> (D, I) CUDA tensors, I = -1 where D = +inf."""
        torch = _torch()
        D, labels = self.scan_device(xq, k)
        il = self.invlists
        if hasattr(il, "translate_labels"):
            return D, il.translate_labels(labels)
        off, ids = self._device_offsets()
        if ids is None:
            raise RuntimeError("search_device: the inverted lists cannot translate labels")
        valid = labels >= 0
        safe = torch.where(valid, labels, torch.zeros_like(labels))
        rows = off[safe >> 32] + (safe & 0xFFFFFFFF)
        if ids.numel() == 0:
            return D, torch.full_like(labels, -1)
        return D, torch.where(valid, ids[rows.clamp(max=ids.numel() - 1)], torch.full_like(labels, -1))

    # -- searches
    def search(self, xq, k):
        """Non-deferred path: every probed list is fully decoded (get_ids) like IndexIVF::search_preassigned."""
        D, L = self._scan(xq, k)
        I = np.full_like(L, -1)
        valid = L >= 0
        lists = (L[valid] >> 32).astype(np.int64)
        offs = (L[valid] & 0xFFFFFFFF).astype(np.int64)
        cache = {}
        out = np.zeros(lists.size, np.int64)
        for i, (l, o) in enumerate(zip(lists, offs)):
            if l not in cache:
                cache[l] = np.asarray(self.invlists.get_ids(int(l)))
            out[i] = cache[l][o]
        I[valid] = out
        return D, I

    def search_defer_id_decoding(self, xq, k, decode_1by1=False, return_codes=0):
        """custom_invlists_impl.cpp:407-526 (parallel_mode == 3 is required there, :420-422)."""
        torch = _torch()
        if self.parallel_mode != 3:
            raise RuntimeError("set the parallel mode to 3 otherwise search will be single-threaded")
        D, L = self._scan(xq, k)
        I = np.full_like(L, -1)
        valid = L >= 0
        lists = (L[valid] >> 32).astype(np.uint64)
        offs = (L[valid] & 0xFFFFFFFF).astype(np.uint64)
        il = self.invlists
        if decode_1by1:
            if hasattr(il, "get_single_ids"):
                I[valid] = il.get_single_ids(lists, offs)
            else:
                I[valid] = [il.get_single_id(int(l), int(o)) for l, o in zip(lists, offs)]
        else:
            uniq, inv = np.unique(lists, return_inverse=True)  # touched lists (:477-502)
            if hasattr(il, "decode_gather"):  # ONE library call: batched device decode + device-side scatter (:508-525)
                I[valid] = il.decode_gather(uniq, inv, offs)
            elif hasattr(il, "decode_lists"):  # a container with a batched decode only: index on the device with torch
                ids, out_off = il.decode_lists(uniq)
                pos = torch.from_numpy((out_off[inv].astype(np.int64) + offs.astype(np.int64))).cuda()
                I[valid] = ids[pos].cpu().numpy()
            else:
                per = [np.asarray(il.get_ids(int(l))) for l in uniq]
                I[valid] = [per[i][int(o)] for i, o in zip(inv, offs)]
        if not return_codes:
            return D, I
        off, codes = self._device_lists()
        cs1 = self.code_size + (1 if return_codes == 2 else 0)  # coarse_code_size() = 1 byte for nlist <= 256
        out = np.full(L.shape + (cs1,), 0xFF, dtype=np.uint8)  # memset(code1, -1, code_size_1), :444-446
        rows = off[lists.astype(np.int64)] + offs.astype(np.int64)
        got = codes[torch.from_numpy(rows).cuda()].cpu().numpy()
        if return_codes == 2:
            got = np.concatenate([lists.astype(np.uint8)[:, None], got], 1)  # encode_listno, :455-458
        out[valid] = got
        return D, I, out
