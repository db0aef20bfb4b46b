"""Drop-in counterpart of the reference's `altid` SWIG module (alt-graph-index/altid.swig):
compressed replacements of faiss::nsg::Graph<int32_t> (alt-graph-index/altid_impl.h:29-67).

Each class is built from the final NSG graph (an int32 [N, K] array, -1 padded) and answers
`get_neighbors(i)`; `get_neighbors_batch(nodes)` is the GPU-friendly form (one launch for a frontier).
"""
import numpy as np

from .codecs import CompactRows, EfLists, RocLists, update_rows


def _graph_rows(graph):
    """Accepts a numpy/torch [N, K] int32 array or an object with .data/.N/.K (nsg::Graph surface)."""
    if hasattr(graph, "N") and hasattr(graph, "K") and hasattr(graph, "data"):
        return np.asarray(graph.data, dtype=np.int32).reshape(int(graph.N), int(graph.K))
    if hasattr(graph, "cpu"):
        return graph
    return np.ascontiguousarray(graph, dtype=np.int32)


class _GraphBase:
    def __init__(self, graph):
        rows = _graph_rows(graph)
        self.N, self.K = int(rows.shape[0]), int(rows.shape[1])
        self.data = None  # the reference sets data = nullptr after compression (altid_impl.cpp:38,89,150)
        self._rows = rows

    def get_neighbors(self, i):
        """-> numpy int32 array of the neighbours of node i (the reference writes them into a caller buffer)."""
        out, cnt = self.get_neighbors_batch([i])
        return out[0, : int(cnt[0])].copy()

    def get_neighbors_batch(self, nodes):
        out, cnt = self._c.decode_rows(np.asarray(nodes, dtype=np.uint64))
        return out.cpu().numpy(), cnt

    def get_neighbors_device(self, nodes):
        """The same with the rows left in HBM: int32 [m, K] CUDA tensor, -1 padded (no edge counts cross PCIe).  `nodes` may be a CUDA
        tensor (a frontier from a GPU argmin): it stays on the device, and a negative node gives a row of -1."""
        if type(nodes).__module__.split(".")[0] == "torch" and nodes.is_cuda:
            return self._c.decode_rows(nodes, self.K, want_counts=False)[0]
        return self._c.decode_rows(np.asarray(nodes, dtype=np.uint64), self.K, want_counts=False)[0]

    def update_rows(self, nodes, rows, n_new=None):
        """What an insert does to the adjacency: batch row i replaces the row of nodes[i] (the last mention of a node wins, a negative
        node is skipped), and the graph grows to n_new nodes (None: as many as now; new nodes without a batch row have no edges) -> a
        NEW graph object of the same class; this one stays valid.  nodes: [m] integers, rows: [m, K] int32, -1 terminated; numpy arrays
        or CUDA tensors.  Nothing is re-encoded but the batch rows (codecs.update_rows)."""
        g = object.__new__(type(self))
        g._c = update_rows(self._c, nodes, rows, n_new=n_new)
        g.N, g.K = int(self.N if n_new is None else n_new), self.K
        g.data, g._rows = None, None
        g._derive()
        return g


class CompactBitNSGGraph(_GraphBase):
    """altid_impl.cpp:20-51: ceil(log2(N+1)) bits per edge, fixed stride, sentinel N."""

    def __init__(self, graph):
        super().__init__(graph)
        self._c = CompactRows.encode_rows(self._rows)
        self._derive()
        self._rows = None

    def _derive(self):
        self.bits = self._c.bits
        self.stride = self._c.stride
        self.compressed_ids_size_in_bytes = self._c.size_in_bytes  # compressed_data.size() = N * stride


class EliasFanoNSGGraph(_GraphBase):
    """altid_impl.cpp:53-101."""

    def __init__(self, graph):
        super().__init__(graph)
        self._c = EfLists.encode_rows(self._rows)
        self._derive()
        self._rows = None

    def _derive(self):
        self.compressed_ids_size_in_bytes = self._c.compressed_bytes  # :86,88
        # :55-57: size of each friend list + its max id, ceil(log2 N) bits each
        # (a size_t incremented twice by a double: the value truncates after EACH addition)
        x = self.N * np.ceil(np.log2(self.N)) / 8.0 if self.N > 1 else 0.0
        self.overhead_in_bytes = int(int(x) + x)

    def has_edges(self, u, v):
        """-> bool CUDA tensor: is v[i] a neighbour of u[i]?  Searched inside the compressed rows (rank.contains), no row is decoded.  u, v:
        integer arrays or CUDA tensors with one entry per pair; a node u[i] outside 0 .. N-1 gives False, and so does a v[i] that is no
        node id (negative: as an unsigned number it is above every id a row holds)."""
        from . import rank
        from .codecs import _is_cuda, _torch

        torch = _torch()

        def dev(a):
            if _is_cuda(a):
                return a.reshape(-1).to(torch.int64)
            return np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int64)

        return rank.contains(self._c, dev(u), dev(v))


class ROCNSGGraph(_GraphBase):
    """altid_impl.cpp:103-165."""

    def __init__(self, graph):
        super().__init__(graph)
        self._c = RocLists.encode_rows(self._rows)
        self._derive()
        self._rows = None

    def _derive(self):
        info = self._c.info()
        self.id_symbol_precision = info["precision"].astype(np.uint64)
        self.num_outgoing_edges = info["sizes"].astype(np.uint32)  # altid_impl.h:61
        # :148 adds ans_states[list_no].size() for EVERY node (8 bytes even for an empty state)
        self.compressed_ids_size_in_bytes = int(8 * self.N + 4 * int(info["nwords"].sum()))
        self.overhead_in_bytes = int(self.N * np.ceil(np.log2(self.N)) / 8.0) if self.N > 1 else 0  # :105


AVAILABLE_COMPRESSED_GRAPHS = {  # graph_dynamic_bench_invlists.py:21-26
    "elias-fano": EliasFanoNSGGraph,
    "roc": ROCNSGGraph,
    "compact": CompactBitNSGGraph,
    "ref": None,
}
