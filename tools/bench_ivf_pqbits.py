"""Packed PQ codes in the device IVF scan and encoder (IVFIndex(d, nlist, ("PQ", 8, 10), by_residual=True): vidc_ivf_scan_pqbits_dev,
vidc_ivf_pq_encode_bits_dev) against what stands beside them, on the same data, lists and probes.

Shape: the reference's PQ8x10 column (custom_invlist_cpp/bench_invlists.py): 10^6 clustered vectors, IVF1024, d = 128, k = 20, nprobe 1
and 16, batches of 10, 10^3 and 10^4 queries, residual codes.  Arms, alternating in one process after a warm-up, inputs
device-resident, probes given:
  pqbits   scan_device on the PQ8x10 residual index (10 code bytes a vector, a 32 KB table per (query, list))
  pq16     scan_device on a PQ16 (8-bit) residual index over the same lists: similar code bytes (16), a 16 KB table -- the floor
  batch    a padded all-torch batch that unpacks the 10-bit fields and decodes residuals: a table per (query, probe), one topk per
           chunk of queries (chunks sized to ~1 GiB) -- the arm `pqbits` is judged against
Table share: the pqbits kernel's time on the same probes with every list that is not empty cut to one code (one table and one trip
per list; an empty list stays empty, so exactly `tables_built` tables are built), next to the full kernel time.  Encoder: pq_encode_bits_device on the database (residual) against M calls of torch.cdist(...).argmin(1) plus a
torch pack.  Recorded per arm: every wall time (perf_counter around the call, ending in a synchronise), median, minimum, maximum, and
vidc_ctx_last_kernel_ms for the device arms.  Hardware counters are not collected.

  python tools/bench_ivf_pqbits.py [--nb 1000000] [--nq 10,1000,10000] [--steps 5] [--out profiles/r49_ivf_pqbits.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

M, NBITS = 8, 10


def spread(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4),
                all=[round(float(x), 4) for x in v])


def torch_fields(codes):
    """uint8 [..., 10] -> int64 fields [..., 8] with torch integer operations"""
    import torch

    wide = torch.nn.functional.pad(codes, (0, 2)).to(torch.int32)
    out = []
    for m in range(M):
        b = m * NBITS
        w = wide[..., b >> 3] | (wide[..., (b >> 3) + 1] << 8) | (wide[..., (b >> 3) + 2] << 16)
        out.append((w >> (b & 7)) & ((1 << NBITS) - 1))
    return torch.stack(out, -1).long()


def torch_pack(fields):
    """int64 fields [n, 8] -> uint8 [n, 10]"""
    import torch

    n = fields.shape[0]
    bits = ((fields[:, :, None] >> torch.arange(NBITS, device=fields.device)) & 1).reshape(n, -1, 8)
    return (bits << torch.arange(8, device=fields.device)).sum(2).to(torch.uint8)


def torch_batch(index, xq, k, probes, off, codes, budget=1 << 30):
    """the padded all-torch scan over packed residual codes -> (D, labels) CUDA tensors"""
    import torch

    nq, nprobe = probes.shape
    sizes = off[1:] - off[:-1]
    d, ksub = index.d, 1 << NBITS
    dsub = d // M
    outD, outL = [], []
    maxlen_all = int(sizes[probes].max().item())
    step = max(1, min(budget // max(1, nprobe * maxlen_all * M * 24), budget // (nprobe * M * ksub * dsub * 4 * 2)))
    for q0 in range(0, nq, step):
        pr, q = probes[q0:q0 + step], xq[q0:q0 + step]
        c = pr.shape[0]
        sz = sizes[pr]
        maxlen = max(1, int(sz.max().item()))
        ar = torch.arange(maxlen, device=xq.device)
        valid = (ar[None, None, :] < sz[:, :, None]).reshape(c, -1)
        pos = (off[pr][:, :, None] + ar[None, None, :]).clamp(max=codes.shape[0] - 1)  # [c, nprobe, P]
        r = q[:, None, :] - index.centroids[pr]  # [c, nprobe, d]
        tab = ((r.view(c, nprobe, M, 1, dsub) - index.pq[None, None]) ** 2).sum(-1)  # [c, nprobe, M, ksub]
        cd = torch_fields(codes[pos]).permute(0, 1, 3, 2)  # [c, nprobe, M, P]
        dist = tab.gather(3, cd).sum(2).reshape(c, -1)
        dist = torch.where(valid, dist, torch.full_like(dist, float("inf")))
        top = dist.topk(min(k, dist.shape[1]), largest=False, sorted=True)
        lab = ((pr << 32)[:, :, None] + ar[None, None, :]).reshape(c, -1).gather(1, top.indices)
        outD.append(top.values)
        outL.append(torch.where(torch.isfinite(top.values), lab, torch.full_like(lab, -1)))
    return torch.cat(outD), torch.cat(outL)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nq", default="10,1000,10000")
    ap.add_argument("--nprobe", default="1,16")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r49_ivf_pqbits.json"))
    a = ap.parse_args()
    import torch

    from _harness import ClusteredVectors
    from vector_db_id_compression_amd import _lib, ivf_encode
    from vector_db_id_compression_amd.ivf import IVFIndex

    torch.cuda.set_device(0)
    ctx = _lib.default_context()
    k, d = 20, 128
    nqs = [int(v) for v in a.nq.split(",")]
    data = ClusteredVectors(nq=max(nqs), d=d, nt=min(200_000, a.nb), nb=a.nb)
    bits_index = IVFIndex(d, a.nlist, ("PQ", M, NBITS), by_residual=True)
    bits_index.train(data.get_train())
    pq16_index = IVFIndex(d, a.nlist, ("PQ", 16), by_residual=True)
    pq16_index.train(data.get_train())
    pq16_index.centroids = bits_index.centroids.clone()  # the same lists and the same probes
    pq16_index.pq_device = True
    for index in (bits_index, pq16_index):
        index.add(data.get_database())
    off_np, codes = bits_index._device_lists()
    assert np.array_equal(off_np, pq16_index._device_lists()[0]) and codes.shape[1] == 10
    off = torch.from_numpy(off_np.astype(np.int64)).cuda()
    sizes = off[1:] - off[:-1]
    allq = torch.from_numpy(np.ascontiguousarray(data.get_queries(), dtype=np.float32)).cuda()
    one_codes = codes[off[:-1][sizes > 0]].contiguous()  # every list cut to its first code; an empty list stays empty (no table)
    one_off = torch.cat([sizes.new_zeros(1), (sizes > 0).long().cumsum(0)]).contiguous()
    pq, cent = bits_index.pq.to(torch.float32).contiguous(), bits_index.centroids.to(torch.float32).contiguous()
    ptr = _lib.ptr

    def one_code_scan(xq, probes):
        nq, nprobe = probes.shape
        D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        L = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        _lib.check(_lib.lib().vidc_ivf_scan_pqbits_dev(ctx.h, a.nlist, ptr(one_off), int(one_codes.shape[0]), ptr(one_codes), d, M, NBITS, ptr(pq), ptr(cent),
                                                       nq, ptr(xq), nprobe, ptr(probes), k, ptr(D), ptr(L), None))
        return ctx.last_kernel_ms()

    res = dict(tool="tools/bench_ivf_pqbits.py", device=torch.cuda.get_device_name(0), nb=a.nb, nlist=a.nlist, d=d, M=M, nbits=NBITS, k=k,
               steps=a.steps, warmup=a.warmup, num_cu=ctx.num_cu(),
               arms=dict(pqbits="IVFIndex((\"PQ\", 8, 10), by_residual=True).scan_device (vidc_ivf_scan_pqbits_dev), probes given",
                         pq16="IVFIndex((\"PQ\", 16), by_residual=True).scan_device over the same lists (vidc_ivf_scan_residual_dev)",
                         batch="padded all-torch batch that unpacks the fields and decodes residuals, probes given, chunked to ~1 GiB"),
               table_share="last_kernel_ms of the pqbits call on the same probes with every non-empty list cut to one code (one table, one trip per list)",
               not_measured="hardware counters; raw (non-residual) PQ8x10; other k, M, nbits, d; per-kernel split of a cut call", rows=[])

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")

    # the encoder: the database's residual codes, device against torch
    xb = torch.from_numpy(np.ascontiguousarray(data.get_database(), dtype=np.float32)).cuda()
    assign = bits_index._assign_lists(xb)
    dsub = d // M

    def torch_encode():
        r = xb - bits_index.centroids[assign]
        f = torch.stack([torch.cat([torch.cdist(r[i:i + 65536, m * dsub:(m + 1) * dsub].contiguous(), bits_index.pq[m]).argmin(1)
                                    for i in range(0, r.shape[0], 65536)]) for m in range(M)], 1)
        return torch_pack(f)

    ewall, ek = {"device": [], "torch": []}, []
    for it in range(a.warmup + a.steps):
        for arm in ("device", "torch"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = ivf_encode.pq_encode_bits_device(xb, bits_index.pq, NBITS, bits_index.centroids, assign) if arm == "device" else torch_encode()
            torch.cuda.synchronize()
            if it >= a.warmup:
                ewall[arm].append(1e3 * (time.perf_counter() - t0))
                if arm == "device":
                    ek.append(ctx.last_kernel_ms())
            if arm == "device":
                dev_codes = out
            else:
                agree = float((out == dev_codes).all(1).float().mean().item())
            del out
    row = dict(kind="encode", n=a.nb, device=dict(wall_ms=spread(ewall["device"]), last_kernel_ms=spread(ek)), torch=dict(wall_ms=spread(ewall["torch"])),
               vectors_per_s_device=round(a.nb / (np.median(ewall["device"]) * 1e-3)), rows_equal_to_torch=round(agree, 5),
               wall_ratio_torch_over_device=round(float(np.median(ewall["torch"]) / np.median(ewall["device"])), 2))
    res["rows"].append(row)
    print(json.dumps(row), flush=True)
    save()
    del xb, dev_codes
    torch.cuda.empty_cache()

    for nprobe in [int(v) for v in a.nprobe.split(",")]:
        for nq in nqs:
            xq = allq[:nq].contiguous()
            probes = torch.cdist(xq, bits_index.centroids).topk(nprobe, largest=False).indices.contiguous()
            arms = ["pqbits", "pq16", "batch"]
            wall = {arm: [] for arm in arms}
            kms = {"pqbits": [], "pq16": []}
            got = {}
            for it in range(a.warmup + a.steps):
                for arm in arms:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if arm == "pqbits":
                        out = bits_index.scan_device(xq, k, probes=probes)
                    elif arm == "pq16":
                        out = pq16_index.scan_device(xq, k, probes=probes)
                    else:
                        out = torch_batch(bits_index, xq, k, probes, off, codes)
                    torch.cuda.synchronize()
                    ms = 1e3 * (time.perf_counter() - t0)
                    if it >= a.warmup:
                        wall[arm].append(ms)
                        if arm in kms:
                            kms[arm].append(ctx.last_kernel_ms())
                    got[arm] = out[0]
                    del out
            tables = [one_code_scan(xq, probes) for _ in range(a.steps)]
            same = torch.isclose(got["pqbits"], got["batch"], rtol=1e-4, atol=0).all(dim=1)
            nonempty = int((sizes[probes] > 0).sum().item())
            row = dict(kind="scan", nprobe=nprobe, nq=nq, code_bytes=int(sizes[probes].sum().item()) * 10, tables_built=nonempty,
                       codebook_bytes_read=nonempty * 1024 * d * 4,
                       pqbits=dict(wall_ms=spread(wall["pqbits"]), last_kernel_ms=spread(kms["pqbits"]), last_kernel_ms_one_code_lists=spread(tables)),
                       pq16=dict(wall_ms=spread(wall["pq16"]), last_kernel_ms=spread(kms["pq16"])),
                       batch=dict(wall_ms=spread(wall["batch"])),
                       table_share_of_kernel_time=round(float(np.median(tables) / np.median(kms["pqbits"])), 3),
                       kernel_ratio_pqbits_over_pq16=round(float(np.median(kms["pqbits"]) / np.median(kms["pq16"])), 2),
                       wall_ratio_batch_over_pqbits=round(float(np.median(wall["batch"]) / np.median(wall["pqbits"])), 2),
                       D_rows_close_to_batch=int(same.sum().item()))
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            save()
            del got
            torch.cuda.empty_cache()
    if a.out:
        print("wrote", a.out)


if __name__ == "__main__":
    main()
