"""Range search over IVF lists on the device (ivf_range.range_scan_device: vidc_ivf_range_count_dev + vidc_ivf_range_fill_dev)
against the torch form it stands beside and against one top-k distance pass, on the same index and the same probes.

Shapes: 10^6 clustered vectors, IVF1024, PQ16 at d = 128 and Flat at d = 32, nprobe 1 and 16, batches of 10, 10^3 and 10^4 queries.
Radii: per (code, nprobe) three radii, for about 10, 100 and 1000 results per query on the median over the 10^4 queries.  The first
two are the median k-th distance of a scan_device run at k = 10 and k = 100.  The scan's k stops at 256, so the third starts from
the median 256th distance and is widened by bisection over vidc_ivf_range_count_dev until the median count is about 1000 (with
nprobe = 1 a list holds about 977 entries: the radius then takes nearly the whole list, and the count that was reached is recorded).
Arms, alternating in one process after a warm-up:
  range    ivf_range.range_scan_device (probes given: the coarse quantiser is outside every arm): count, 8 bytes back, allocation, fill
  torch    the padded all-torch batch of tools/bench_ivf_scan.py (probed lists gathered to a common length, PQ by table lookup, chunks
           of ~1 GiB of gathered codes), then dist < radius, nonzero, the gathers of D and the labels and the cumulative sum of the
           counts: the best path without the new calls
  scan     IVFIndex.scan_device at k = 20 on the same probes: the cost of one distance pass with a top-k behind it
Recorded per row: every wall time (perf_counter around the call, ending in a synchronise), median, minimum, maximum; the kernel
time of the count and of the fill separately (vidc_ctx_last_kernel_ms after each, from direct calls of the two entry points) and of
the scan; (count + fill) / scan in kernel time; the results per query; agreement of lims and D with the torch arm.  No threshold:
every arm is reported, also where it loses, and the markdown table the tool prints sets a range time that loses to torch in bold.
Hardware counters are not collected.

  python tools/bench_ivf_range.py [--nb 1000000] [--nq 10,1000,10000] [--steps 5] [--out profiles/r44_ivf_range.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def spread(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4),
                all=[round(float(x), 4) for x in v])


def torch_range(index, xq, radius, probes, off, codes, budget=1 << 30):
    """the padded all-torch range search -> (lims, D, labels) CUDA tensors, in probe-row order and then offset order"""
    import torch

    nq, nprobe = probes.shape
    sizes = off[1:] - off[:-1]
    M, d = index.M, index.d
    width = M if M else 4 * d
    outD, outL, outN = [], [], []
    q0 = 0
    maxlen_all = int(sizes[probes].max().item())
    step = max(1, budget // max(1, nprobe * maxlen_all * width * 8))
    while q0 < nq:
        pr, q = probes[q0:q0 + step], xq[q0:q0 + step]
        c = pr.shape[0]
        sz = sizes[pr]
        maxlen = max(1, int(sz.max().item()))
        ar = torch.arange(maxlen, device=xq.device)
        valid = (ar[None, None, :] < sz[:, :, None]).reshape(c, -1)
        pos = (off[pr][:, :, None] + ar[None, None, :]).reshape(c, -1).clamp(max=codes.shape[0] - 1)
        if M:
            dsub = d // M
            tab = ((q.view(c, M, 1, dsub) - index.pq[None]) ** 2).sum(-1)  # [c, M, 256]
            cd = codes[pos].permute(0, 2, 1).long()  # [c, M, P]
            dist = tab.gather(2, cd).sum(1)
        else:
            vec = codes.view(torch.float32).reshape(-1, d)[pos]
            dist = ((vec - q[:, None, :]) ** 2).sum(-1)
        hit = valid & (dist < radius)
        at = hit.nonzero(as_tuple=True)
        lab = (pr << 32)[at[0], at[1] // maxlen] + at[1] % maxlen
        outD.append(dist[at])
        outL.append(lab)
        outN.append(hit.sum(1))
        q0 += step
    counts = torch.cat(outN)
    lims = torch.zeros(nq + 1, dtype=torch.int64, device=xq.device)
    lims[1:] = counts.cumsum(0)
    return lims, torch.cat(outD), torch.cat(outL)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nq", default="10,1000,10000")
    ap.add_argument("--nprobe", default="1,16")
    ap.add_argument("--targets", default="10,100,1000")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r44_ivf_range.json"))
    a = ap.parse_args()
    import torch

    import ivf_range_ref as rr
    import ivf_scan_ref as ir
    from _harness import ClusteredVectors
    from vector_db_id_compression_amd import _lib, ivf_range
    from vector_db_id_compression_amd.custom_invlists import CompressedIDInvertedListsPackedBits
    from vector_db_id_compression_amd.ivf import IVFIndex

    torch.cuda.set_device(0)
    ctx = _lib.default_context()
    nqs = [int(v) for v in a.nq.split(",")]
    targets = [int(v) for v in a.targets.split(",")]

    res = dict(tool="tools/bench_ivf_range.py", device=torch.cuda.get_device_name(0), nb=a.nb, nlist=a.nlist, steps=a.steps, warmup=a.warmup,
               num_cu=ctx.num_cu(),
               arms=dict(range="ivf_range.range_scan_device (count, 8 bytes back, allocation, fill), probes given",
                         torch="padded all-torch batch, dist < radius, nonzero, gathers, cumsum; probes given, ~1 GiB chunks",
                         scan="IVFIndex.scan_device at k = 20, probes given: one distance pass with a top-k"),
               not_measured="hardware counters (no cause is claimed for any ratio); range_search_device end to end (translate_labels "
                            "behind the fill); other M and d; radii beyond ~1000 results per query; float data whose hits lie at the "
                            "radius (the agreement columns count the queries where both arms agree)",
               rows=[])
    table = ["| code | nprobe | queries | results / query | S | `range_scan_device` | count + fill kernels | torch batch + nonzero | "
             "`scan_device` k = 20 | scan kernels | (count + fill) / scan |", "|---|---|---|---|---|---|---|---|---|---|---|"]

    for code, d in ((("PQ", 16), 128), ("Flat", 32)):
        data = ClusteredVectors(nq=max(nqs), d=d, nt=min(200_000, a.nb), nb=a.nb)
        index = IVFIndex(d, a.nlist, code)
        index.train(data.get_train())
        index.add(data.get_database())
        index.replace_invlists(CompressedIDInvertedListsPackedBits(index.invlists))
        off_np, codes = index._device_lists()
        off, _ = index._device_offsets()
        kind = ir.PQ8 if index.M else ir.FLAT
        pq = index.pq.to(torch.float32).contiguous() if index.M else None
        allq = torch.from_numpy(np.ascontiguousarray(data.get_queries(), dtype=np.float32)).cuda()

        def two_pass(xq, probes, radius, fill=True):
            """the two entry points called directly -> (total, count kernel ms, fill kernel ms)"""
            nq, nprobe = probes.shape
            head = (ctx.h, index.nlist, _lib.ptr(off), int(codes.shape[0]), _lib.ptr(codes), kind, index.d, index.M, _lib.ptr(pq), nq,
                    _lib.ptr(xq), nprobe, _lib.ptr(probes), float(radius))
            lims = torch.empty(nq * nprobe + 1, dtype=torch.int64, device=xq.device)
            total = ctypes.c_uint64(0)
            _lib.check(_lib.lib().vidc_ivf_range_count_dev(*head, _lib.ptr(lims), ctypes.byref(total)))
            cms = ctx.last_kernel_ms()
            if not fill or not total.value:
                return int(total.value), cms, 0.0, lims
            D = torch.empty(total.value, dtype=torch.float32, device=xq.device)
            L = torch.empty(total.value, dtype=torch.int64, device=xq.device)
            _lib.check(_lib.lib().vidc_ivf_range_fill_dev(*head, _lib.ptr(lims), total.value, _lib.ptr(D), _lib.ptr(L)))
            return int(total.value), cms, ctx.last_kernel_ms(), lims

        def median_count(xq, probes, radius):
            lims = two_pass(xq, probes, radius, fill=False)[3]
            return float(lims[::probes.shape[1]].diff().float().median().item())

        for nprobe in [int(v) for v in a.nprobe.split(",")]:
            index.nprobe = nprobe
            probes_all = torch.cdist(allq, index.centroids).topk(nprobe, largest=False).indices.contiguous()
            radii = []
            for t in targets:
                kk = min(t, 256)
                Dk = index.scan_device(allq, kk, probes=probes_all)[0][:, kk - 1]
                r = float(Dk[torch.isfinite(Dk)].median().item())
                how = f"median {kk}th distance of scan_device"
                if t > 256:  # the scan's k stops at 256: widen by bisection over the count
                    lo, hi = r, r * 64
                    for _ in range(14):
                        mid = 0.5 * (lo + hi)
                        if median_count(allq, probes_all, mid) < t:
                            lo = mid
                        else:
                            hi = mid
                    r = hi
                    how = "bisection over vidc_ivf_range_count_dev from the median 256th distance"
                radii.append((t, r, how))
            for target, radius, how in radii:
                for nq in nqs:
                    xq, probes = allq[:nq].contiguous(), probes_all[:nq].contiguous()
                    arms = ["range", "torch", "scan"]
                    wall = {arm: [] for arm in arms}
                    scan_ms, got = [], {}
                    for it in range(a.warmup + a.steps):
                        for arm in arms:
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            if arm == "range":
                                out = ivf_range.range_scan_device(index, xq, radius, probes=probes)
                            elif arm == "torch":
                                out = torch_range(index, xq, radius, probes, off, codes)
                            else:
                                out = index.scan_device(xq, 20, probes=probes)
                            torch.cuda.synchronize()
                            ms = 1e3 * (time.perf_counter() - t0)
                            if it >= a.warmup:
                                wall[arm].append(ms)
                                if arm == "scan":
                                    scan_ms.append(ctx.last_kernel_ms())
                            if arm != "scan":
                                got[arm] = out
                            del out
                    cms, fms = [], []
                    for _ in range(a.steps):
                        total, c, f, _ = two_pass(xq, probes, radius)
                        cms.append(c)
                        fms.append(f)
                    lr, Dr, _ = got["range"]
                    lt, Dt, _ = got["torch"]
                    same_counts = int((lr.diff() == lt.diff()).sum().item())
                    same_D = bool(Dr.shape == Dt.shape and torch.isclose(Dr, Dt, rtol=1e-4, atol=0).all().item())
                    per_q = lr.diff().float()
                    lds = rr.plan_lds(kind, nprobe, d, index.M)
                    resident = ir.plan_resident(ctx.num_cu(), lds)
                    ratio = (float(np.median(cms)) + float(np.median(fms))) / float(np.median(scan_ms))
                    row = dict(code="PQ16" if index.M else "Flat", d=d, nprobe=nprobe, nq=nq, target_results=target, radius=radius,
                               radius_from=how, results_per_query=dict(median=float(per_q.median().item()), max=float(per_q.max().item())),
                               total=total, S=ir.plan_pieces(nq, nprobe, resident), lds_bytes=lds, resident_wavefronts=resident,
                               range=dict(wall_ms=spread(wall["range"]), count_kernel_ms=spread(cms), fill_kernel_ms=spread(fms)),
                               torch=dict(wall_ms=spread(wall["torch"])),
                               scan=dict(wall_ms=spread(wall["scan"]), last_kernel_ms=spread(scan_ms)),
                               wall_ratio_torch_over_range=round(float(np.median(wall["torch"]) / np.median(wall["range"])), 2),
                               kernel_ratio_count_plus_fill_over_scan=round(ratio, 2),
                               queries_with_torchs_count=same_counts, D_close_to_torch=same_D)
                    res["rows"].append(row)
                    print(json.dumps(row), flush=True)

                    def cell(v, lose=False):
                        s = f"{v['median']:.3g} ({v['min']:.3g}-{v['max']:.3g})"
                        return f"**{s}**" if lose else s

                    loses = np.median(wall["range"]) > np.median(wall["torch"])
                    kern = spread([c + f for c, f in zip(cms, fms)])
                    table.append(f"| {row['code']} | {nprobe} | {nq} | {row['results_per_query']['median']:.0f} | {row['S']} | "
                                 f"{cell(row['range']['wall_ms'], loses)} | {cell(kern)} | {cell(row['torch']['wall_ms'])} | "
                                 f"{cell(row['scan']['wall_ms'])} | {cell(row['scan']['last_kernel_ms'])} | {ratio:.2f} |")
                    del got
                    torch.cuda.empty_cache()
        del index, codes, data
        torch.cuda.empty_cache()
    res["markdown_table"] = table
    print("\n".join(table))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
