#!/usr/bin/env python3
# Large-k search (k_max) next to the k = 512 search it takes
# over from, in one process.
#
# Shape: a kNN-LM-like point on the "ivfpq_2m_d768_m64" workload of bench.py
# (IVFPQ m=64, d=768, lists of ~1000 rows; --n / --nlist scale it), a batch
# of --nq token queries at --nprobe lists each, k in {512, 1024, 2048}.
# k = 512 is the existing selection path (per-probe top-k in the scan, then
# the candidate merge); above it the scan writes every distance (count +
# fill pass) and k_select_seg picks per query.
#
# Per k it reports
#   * ms per batch (eager: the large-k path synchronizes) and its ratio to
#     k = 512;
#   * the scan / LUT / merge split from dfann_timing; above 512 merge_ms is
#     k_select_seg alone, with its share of the step;
#   * k_select_seg's segment bytes (12 per candidate: fp32 distance + int64
#     id) over its time — the rate at which it would run if it read the
#     segment once — and the bytes it swept, from the number of sweeps a
#     host restatement of the radix select counts on 16 sample queries.
#
# Prints one JSON line.
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FLT_MAX = 3.4028234663852886e38
RES_CAP, RADIX = 4096, 8   # SEG_RES_CAP / SEG_RADIX of kernels.hip


def sweeps(d, ids, k):
    """Sweeps of one segment by k_select_seg: pass 0, one per digit until
    the bucket holding rank k is needed whole, the collect."""
    if d.size <= RES_CAP:
        return 1  # later passes run in LDS
    if d.size <= k:
        return 2
    b = (d + np.float32(0)).view(np.uint32).astype(np.uint64)
    b = np.where(b >> np.uint64(31), ~b & np.uint64(0xFFFFFFFF),
                 b | np.uint64(0x80000000))
    c = (b << np.uint64(32)) | ids.astype(np.uint64)
    shift = int(c.min() ^ c.max()).bit_length()
    need, n = k, 2
    while shift > 0:
        nb = min(RADIX, shift)
        shift -= nb
        n += 1
        digit = ((c >> np.uint64(shift))
                 & np.uint64((1 << nb) - 1)).astype(np.int64)
        hist = np.bincount(digit, minlength=1 << nb)
        cum = np.cumsum(hist)
        bkt = int(np.searchsorted(cum, need))
        need -= int(cum[bkt] - hist[bkt])
        c = c[digit == bkt]
        if hist[bkt] == need:
            break
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--nlist", type=int, default=2048)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import torch

    import bench
    from distributed_faiss_amd.hip_engine import HipEngine

    cfg = dict(bench.WORKLOADS["ivfpq_2m_d768_m64"], n=args.n,
               nlist=args.nlist, nq=args.nq)
    xb, q = bench.gen_shard(cfg, 0, "cuda")
    eng = HipEngine(spec={
        "type": "ivfpq", "dim": cfg["d"], "metric": cfg["metric"],
        "nlist": cfg["nlist"], "m": cfg["m"], "nbits": 8, "seed": 1234,
        "nprobe": args.nprobe, "coarse_bf16": cfg["coarse_bf16"],
        "max_ppc": cfg["max_ppc"], "k_max": 2048})
    eng.train_dev(xb)
    eng.add_dev(xb)
    nq = q.shape[0]

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.steps):
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return round(statistics.median(ts), 4)

    def split(fn, calls=4):
        eng.set_timing(True)
        eng.get_timing()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        t = eng.get_timing()
        eng.set_timing(False)
        return {key: round(t[key] / calls, 4)
                for key in ("scan_ms", "lut_ms", "gemm_ms", "merge_ms")}

    # candidates per query and the select's sweeps on 16 sample queries
    lims, Dall, Iall = eng.range_search_dev(q, FLT_MAX)
    lims = lims.cpu().numpy()
    seg_bytes = 12 * int(lims[-1])
    Dh, Ih = Dall[:lims[16]].cpu().numpy(), Iall[:lims[16]].cpu().numpy()
    del Dall, Iall

    out = {"n": eng.ntotal, "d": cfg["d"], "m": cfg["m"], "nlist": cfg["nlist"],
           "nq": nq, "nprobe": args.nprobe, "steps": args.steps,
           "candidates_per_query": round(int(lims[-1]) / nq, 1), "k": {}}
    for k in (512, 1024, 2048):
        D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        leg = {"ms": timed(lambda: eng.search_dev(q, k, D, I))}
        leg.update(split(lambda: eng.search_dev(q, k, D, I)))
        if k > 512:
            leg["ms_over_k512"] = round(leg["ms"] / out["k"][512]["ms"], 3)
            leg["select_share"] = round(leg["merge_ms"] / leg["ms"], 3)
            n = statistics.mean(sweeps(Dh[lims[i]:lims[i + 1]],
                                       Ih[lims[i]:lims[i + 1]], k)
                                for i in range(16))
            leg["select_sweeps"] = round(n, 2)
            per_s = 1e3 / leg["merge_ms"] / 1e9
            leg["select_segment_gbps"] = round(seg_bytes * per_s, 1)
            leg["select_swept_gbps"] = round(seg_bytes * n * per_s, 1)
        out["k"][k] = leg
        print(f"[large_k_bench] k={k}: {leg}", file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
