#!/usr/bin/env python3
"""Dev tool: encodes from DEVICE offsets only (packed bits, Elias-Fano, wavelet tree), nothing else -- run under
`rocprofv3 --memory-copy-trace --kernel-trace --stats` to list the copies and kernels such a call is made of (no copy of the
offsets to or from the host should appear).  usage: trace_dev_offsets.py [workload] [reps]"""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vector_db_id_compression_amd import _lib, synth
from vector_db_id_compression_amd.codecs import EfLists, PackedLists, WaveletTreeLists
ctx = _lib.default_context(0)
w = synth.workload(sys.argv[1] if len(sys.argv) > 1 else "uniform_16m", seed=1)
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
ids = w["ids"] if not isinstance(w["ids"], np.ndarray) else torch.from_numpy(w["ids"].view(np.int64)).cuda()
d_off = torch.from_numpy(w["offsets"].view(np.int64)).cuda()
# the wavelet tree needs ids = a permutation of 0..ntotal-1, ascending per list: the list positions themselves
wt_ids = torch.arange(w["ntotal"], dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
for _ in range(reps):
    PackedLists.encode(d_off, ids, ctx=ctx)
    EfLists.encode(d_off, ids, ctx=ctx)
WaveletTreeLists.build(d_off, wt_ids, ctx=ctx)
torch.cuda.synchronize()
print("nlist", w["nlist"], "offsets bytes", 8 * (w["nlist"] + 1), "reps", reps)
