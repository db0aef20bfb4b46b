"""The numpy statement of a packed PQ code (include/vidc.h, csrc/ivf_pqbits_plan.h) and the objects the CPU and GPU tests share.

A code row is one little-endian bit string of ceil(M * nbits / 8) bytes: sub-quantiser m occupies the bits [m * nbits, (m + 1) * nbits),
least significant bit first; bit i of the row is bit i % 8 of byte i / 8; pad bits are 0.  Data are integer grids (ivf_scan_ref.py).
"""
import functools

import numpy as np

import ivf_scan_ref as ir

FORMS = ((16, 8, 10), (12, 3, 10), (10, 5, 5), (16, 16, 4), (8, 2, 12), (7, 7, 1))  # (d, M, nbits)


def pack(fields, nbits):
    """fields integer [n, M] -> uint8 [n, ceil(M * nbits / 8)]"""
    fields = np.asarray(fields, dtype=np.int64)
    n, M = fields.shape
    bits = (fields[:, :, None] >> np.arange(nbits)) & 1  # [n, M, nbits]: bit m * nbits + b of the row
    bits = np.concatenate([bits.reshape(n, M * nbits), np.zeros((n, -M * nbits % 8), np.int64)], 1)
    return (bits.reshape(n, -1, 8) << np.arange(8)).sum(2).astype(np.uint8)


def unpack(codes, M, nbits):
    """uint8 [n, code_size] -> int64 fields [n, M]"""
    codes = np.asarray(codes, dtype=np.uint8)
    bits = (codes[:, :, None].astype(np.int64) >> np.arange(8)) & 1
    bits = bits.reshape(codes.shape[0], -1)[:, :M * nbits].reshape(-1, M, nbits)
    return (bits << np.arange(nbits)).sum(2)


def decode(codes, cb, nbits):
    f = unpack(codes, cb.shape[0], nbits)
    return np.concatenate([cb[m][f[:, m]] for m in range(cb.shape[0])], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def obj(d, M, nbits, sizes=ir.EDGE_SIZES, R=ir.R_EDGES, seed=3):
    """random fields, integer codebooks [M, 2^nbits, d / M], integer centroids; vecs = the decoded codes (raw), rvecs = decoded +
    the centroid of the row's list (residual).  d * (3R)^2 < 2^24: query - centroid - codeword stays on the exact grid."""
    assert d * (3 * R) ** 2 < 2 ** 24 and d % M == 0
    rng = np.random.default_rng(seed + 1000 * d + 10 * M + nbits)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ntotal = int(off[-1])
    cb = rng.integers(-R, R + 1, size=(M, 1 << nbits, d // M)).astype(np.float32)
    fields = rng.integers(0, 1 << nbits, size=(ntotal, M))
    cent = rng.integers(-R, R + 1, size=(len(sizes), d)).astype(np.float32)
    codes = pack(fields, nbits)
    vecs = decode(codes, cb, nbits)
    lists = np.repeat(np.arange(len(sizes)), sizes)
    return ir._freeze(dict(offsets=off, ntotal=ntotal, nlist=len(sizes), fields=fields, codes=codes, vecs=vecs, rvecs=vecs + cent[lists],
                           codebooks=cb, centroids=cent, d=d, M=M, nbits=nbits))
