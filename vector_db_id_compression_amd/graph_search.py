"""Greedy best-first search over a (compressed) neighbour graph -- the caller side of `get_neighbors`
(faiss::NSG::search_on_graph in the reference's flow).  Harness plumbing in numpy/torch; the codec
work is the batched `get_neighbors_batch` of the graph object (one device launch per expansion round)."""
import numpy as np


class RawGraph:
    """Uncompressed nsg::Graph<int32_t> stand-in: rows int32 [N, K], -1 padded."""

    def __init__(self, rows):
        self.rows = np.ascontiguousarray(rows, dtype=np.int32)
        self.N, self.K = self.rows.shape

    def get_neighbors_batch(self, nodes):
        out = self.rows[np.asarray(nodes, dtype=np.int64)]
        return out, (out >= 0).sum(1).astype(np.uint32)

    def get_neighbors_device(self, nodes):
        """rows of `nodes` as an int32 CUDA tensor; a CUDA tensor of nodes stays on the device, and its nodes outside [0, N) give a row
        of -1 (as the compressed graphs do)"""
        import torch

        if getattr(self, "_dev", None) is None:
            self._dev = torch.from_numpy(self.rows).cuda()
        if isinstance(nodes, torch.Tensor) and nodes.is_cuda:
            nd = nodes.long()
            if self.N == 0:
                return torch.full((nd.numel(), self.K), -1, dtype=torch.int32, device=nd.device)
            ok = (nd >= 0) & (nd < self.N)
            out = self._dev[torch.where(ok, nd, torch.zeros_like(nd))]
            return torch.where(ok[:, None], out, torch.full_like(out, -1))
        return self._dev[torch.as_tensor(np.asarray(nodes, dtype=np.int64), device="cuda")]


def knn_graph(x, K, seed=0):
    """Exact kNN graph (brute force on the GPU) with random out-degrees in [K/2, K], -1 padded: an NSG-shaped input."""
    import torch

    xt = torch.as_tensor(np.asarray(x, dtype=np.float32)).cuda()
    N = xt.shape[0]
    rows = np.full((N, K), -1, dtype=np.int32)
    rng = np.random.default_rng(seed)
    deg = rng.integers(K // 2, K + 1, size=N)
    for a in range(0, N, 4096):
        d = torch.cdist(xt[a:a + 4096], xt)
        idx = d.topk(K + 1, largest=False).indices[:, 1:].cpu().numpy()
        rows[a:a + 4096] = idx
    rows[np.arange(K)[None, :] >= deg[:, None]] = -1
    return rows


def search(graph, x, xq, k, L=32, entry=0):
    """Best-first search with a candidate pool of size L (NSG search_on_graph style). -> (D, I) arrays [nq, k]."""
    x = np.asarray(x, dtype=np.float32)
    xq = np.asarray(xq, dtype=np.float32)
    nq = xq.shape[0]
    D = np.full((nq, k), np.inf, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        visited = {entry}
        d0 = float(((x[entry] - xq[q]) ** 2).sum())
        pool = [(d0, entry, False)]  # (distance, node, expanded)
        while True:
            cand = [i for i, (_, _, e) in enumerate(pool) if not e]
            if not cand:
                break
            i = cand[0]
            dist, node, _ = pool[i]
            pool[i] = (dist, node, True)
            nb, cnt = graph.get_neighbors_batch([node])
            for v in nb[0, : int(cnt[0])]:
                v = int(v)
                if v in visited:
                    continue
                visited.add(v)
                pool.append((float(((x[v] - xq[q]) ** 2).sum()), v, False))
            pool.sort(key=lambda t: (t[0], t[1]))
            pool = pool[:L]
        top = pool[:k]
        D[q, : len(top)] = [t[0] for t in top]
        I[q, : len(top)] = [t[1] for t in top]
    return D, I


def _device_rows(graph):
    """-> ("rows" | "compact" | "ef", the object the C call takes, N, K) of a graph `search_device` can walk; VidcError by class name
    for everything else (decided before the device is looked at)."""
    from . import altid, codecs
    from ._lib import VidcError

    if isinstance(graph, RawGraph):
        return "rows", graph, graph.N, graph.K
    if isinstance(graph, (altid.CompactBitNSGGraph, altid.EliasFanoNSGGraph)):
        graph = graph._c
    if isinstance(graph, codecs.CompactRows):
        return "compact", graph, getattr(graph, "N", None), getattr(graph, "K", 0)
    if isinstance(graph, codecs.EfLists):
        n = getattr(graph, "_nlist", None) if getattr(graph, "_offsets", None) is None else graph._offsets.size - 1
        return "ef", graph, n, getattr(graph, "K", 0)
    raise VidcError(f"search_device: {type(graph).__name__} rows cannot be decoded inside the search kernel (raw, compact and "
                    "Elias-Fano rows can; a ROC row is a serial ANS chain): use graph_search.search_batched")


def search_device(graph, x, xq, k, L=64, entry=0, max_rounds=None, stats=False):
    """The best-first search of `search` for a whole batch as ONE kernel launch (vidc_{rows,compact,ef}_search_dev): a wavefront per query
    decodes the rows it expands inside the kernel; pools, frontier and visited sets stay on the device.

    graph: RawGraph, CompactBitNSGGraph, EliasFanoNSGGraph, or the CompactRows / EfLists graph objects behind them (Elias-Fano: rows of
    at most 64 edges).  ROCNSGGraph and every other class: VidcError naming the class (search_batched is their path).  x: float32 [N, d]
    (a CUDA tensor stays where it is, anything else is uploaded once); xq: [nq, d]; 1 <= k <= L <= 256; max_rounds None / 0: no cap.
    -> (D float32 [nq, k], I int64 [nq, k]) CUDA tensors, +inf / -1 padded, and with stats=True a third, int32 [nq, 2] = (steps taken,
    distances computed) per query.  Runs on torch's current stream; the call waits for its kernel."""
    from . import _lib
    from ._lib import VidcError, check, lib, ptr

    kind, obj, N, K = _device_rows(graph)
    import torch

    if not torch.cuda.is_available():
        raise VidcError("no HIP device: search_device needs an MI355X (there is no CPU fallback)")

    def f32(a):
        if not (isinstance(a, torch.Tensor) and a.is_cuda):
            a = torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()  # (a copy: torch wants a writable array)
        return a.to(torch.float32).contiguous()

    xt, qt = f32(x), f32(xq)
    if xt.dim() != 2 or qt.dim() != 2 or qt.shape[1] != xt.shape[1]:
        raise ValueError("x must be [N, d] and xq [nq, d]")
    if N is not None and xt.shape[0] != N:
        raise ValueError(f"x holds {xt.shape[0]} vectors, the graph {N} nodes")
    nq, d = int(qt.shape[0]), int(xt.shape[1])
    k, L, entry, rounds = int(k), int(L), int(entry), int(max_rounds or 0)
    if min(k, L, entry, rounds) < 0 or max(k, L, entry, rounds) >= 2 ** 32:
        raise ValueError("k, L, entry and max_rounds are unsigned 32-bit numbers")
    D = torch.empty((nq, max(k, 0)), dtype=torch.float32, device=xt.device)
    I = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=xt.device)
    S = torch.empty((nq, 2), dtype=torch.int32, device=xt.device) if stats else None
    tail = (ptr(xt) if xt.numel() else None, d, nq, ptr(qt) if nq else None, k, L, entry, rounds, ptr(D) if D.numel() else None,
            ptr(I) if I.numel() else None, ptr(S) if stats and nq else None)
    if kind == "rows":
        if getattr(graph, "_dev", None) is None:
            graph._dev = torch.from_numpy(graph.rows).cuda()
        ctx = _lib.default_context()
        st = lib().vidc_rows_search_dev(ctx.h, xt.shape[0], K, ptr(graph._dev) if graph._dev.numel() else None, *tail)
    else:
        from .codecs import _on_torch_stream

        _on_torch_stream(obj.ctx)
        fn = lib().vidc_compact_search_dev if kind == "compact" else lib().vidc_ef_search_dev
        st = fn(obj.ctx.h, obj.h, *tail)
    try:
        check(st)
    except VidcError as e:
        raise VidcError(f"search_device: {type(graph).__name__}: {e}") from None
    return (D, I, S) if stats else (D, I)


def search_batched(graph, x, xq, k, L=64, entry=0, max_rounds=None):
    """The same best-first search for a whole batch of queries in lock step on the GPU: every round expands the best
    unexpanded candidate of every query with ONE `get_neighbors_device` call (one decode launch for the whole
    frontier, handed over as a CUDA tensor: -1 for a query that is done) -- the shape in which a compressed graph pays off on a GPU.  Pools are ordered by (distance, node id), so
    the result does not depend on the order in which a container returns the neighbours of a node.
    -> (D float32 [nq, k], I int64 [nq, k])"""
    import torch

    xt = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float32)).cuda()
    qt = torch.as_tensor(np.asarray(xq, dtype=np.float32)).cuda()
    nq, N = qt.shape[0], xt.shape[0]
    INF = torch.tensor(float("inf"), device="cuda")
    visited = torch.zeros((nq, N + 1), dtype=torch.bool, device="cuda")  # column N absorbs the -1 padding
    visited[:, entry] = True
    pool_d = torch.full((nq, L), float("inf"), device="cuda")
    pool_n = torch.full((nq, L), -1, dtype=torch.int64, device="cuda")
    pool_e = torch.ones((nq, L), dtype=torch.bool, device="cuda")  # expanded (empty slots count as expanded)
    pool_d[:, 0] = ((xt[entry][None, :] - qt) ** 2).sum(1)
    pool_n[:, 0] = entry
    pool_e[:, 0] = False
    rows = torch.arange(nq, device="cuda")
    rounds = 0
    while True:
        cand = torch.where(pool_e, INF, pool_d)
        best = cand.argmin(1)
        active = torch.isfinite(cand[rows, best])
        if not bool(active.any()) or (max_rounds is not None and rounds >= max_rounds):
            break
        rounds += 1
        nodes = torch.where(active, pool_n[rows, best], torch.full_like(best, -1))  # (a finished query asks for no row)
        pool_e[rows, best] = True
        nb = graph.get_neighbors_device(nodes).long()  # [nq, K], -1 padded; the frontier stays on the device
        ok = (nb >= 0) & active[:, None]
        nbv = torch.where(nb >= 0, nb, torch.full_like(nb, N))
        nbc = nb.clamp(min=0)
        ok &= ~visited.gather(1, nbv)
        # the neighbours of a node are distinct, so a scatter marks exactly the new ones
        visited.scatter_(1, nbv, visited.gather(1, nbv) | ok)
        d = ((xt[nbc] - qt[:, None, :]) ** 2).sum(2)
        d = torch.where(ok, d, INF)
        all_d = torch.cat([pool_d, d], 1)
        all_n = torch.cat([pool_n, torch.where(ok, nbc, torch.full_like(nbc, -1))], 1)
        all_e = torch.cat([pool_e, ~ok], 1)
        # order by (distance, node): float32 bits of a non-negative distance sort like the value
        key = (all_d.view(torch.int32).long() << 32) | all_n.clamp(min=0)
        key = torch.where(torch.isfinite(all_d), key, torch.full_like(key, 0x7FFFFFFFFFFFFFFF))
        idx = key.argsort(1)[:, :L]
        pool_d, pool_n, pool_e = all_d.gather(1, idx), all_n.gather(1, idx), all_e.gather(1, idx)
    return pool_d[:, :k].cpu().numpy(), pool_n[:, :k].cpu().numpy()
