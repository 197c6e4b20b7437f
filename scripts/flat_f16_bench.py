#!/usr/bin/env python3
# Flat fp16 store next to the fp32 flat index, same data.
#
# Shapes (N x d, nq, k = 10, L2, seeded Gaussian data on the device):
#   1M x 768, nq = 10000   the bench batch at the headline width
#   1M x 128, nq = 10000   a short K loop: the select's share grows
#   1M x 768, nq = 16      one query tile: the database stream bounds it
# --small swaps in 20k rows (seconds; overheads, not rates).
#
# Per shape both indexes are built once; after a warm-up of each, timed
# steps ALTERNATE between the two engines (device events around one
# search_dev, ended by an event synchronize). Reported per shape:
#   fp32_ms / fp16_ms   median ms of one search call, and the QPS from them
#   speedup             fp32_ms / fp16_ms
#   kernel_ms           k_flat_f16 alone: the engine's own device events
#                       around that launch (set_timing), median over the steps
#   kernel_tflops       2 * nq * N * d / kernel_ms (algorithmic flop)
#   kernel_gbps         2 * ldh * N / kernel_ms: the database bytes read once
#                       (meaningful where one query tile reads it: nq = 16)
#   recall_at_10        share of the fp32 index's ids found in the fp16
#                       index's 10, mean over queries
# Prints one JSON line per shape.
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [(1_000_000, 768, 10_000), (1_000_000, 128, 10_000),
          (1_000_000, 768, 16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--k", type=int, default=10)
    args = ap.parse_args()

    import torch

    from distributed_faiss_amd.hip_engine import HipEngine

    k = args.k
    for n, d, nq in SHAPES:
        if args.small:
            n = 20_000
        gen = torch.Generator(device="cuda").manual_seed(1234)
        xb = torch.randn((n, d), generator=gen, device="cuda")
        q = torch.randn((nq, d), generator=gen, device="cuda")
        engs = {}
        for store in ("fp32", "fp16"):
            e = HipEngine(spec={"type": "flat", "dim": d, "metric": 1,
                                "flat_store": store})
            CH = 250_000
            for s in range(0, n, CH):
                e.add_dev(xb[s:s + CH].contiguous())
            engs[store] = e
        del xb
        torch.cuda.empty_cache()
        out = {s: (torch.empty((nq, k), dtype=torch.float32, device="cuda"),
                   torch.empty((nq, k), dtype=torch.int64, device="cuda"))
               for s in engs}

        def step(store):
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            engs[store].search_dev(q, k, *out[store])
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        for _ in range(args.warmup):
            for store in engs:
                step(store)
        ms = {s: [] for s in engs}
        kern = []
        engs["fp16"].set_timing(True)
        engs["fp16"].get_timing()
        for _ in range(args.steps):
            for store in engs:
                ms[store].append(step(store))
            kern.append(engs["fp16"].get_timing()["gemm_ms"])
        engs["fp16"].set_timing(False)
        m32, m16 = (statistics.median(ms[s]) for s in ("fp32", "fp16"))
        km = statistics.median(kern)
        I32, I16 = out["fp32"][1], out["fp16"][1]
        recall = (I32[:, :, None] == I16[:, None, :]).any(2).float().mean()
        ldh = (d + 7) // 8 * 8
        print(json.dumps({
            "n": n, "d": d, "nq": nq, "k": k, "metric": "l2",
            "steps": args.steps,
            "fp32_ms": round(m32, 3), "fp32_qps": round(nq / (m32 / 1e3)),
            "fp16_ms": round(m16, 3), "fp16_qps": round(nq / (m16 / 1e3)),
            "speedup": round(m32 / m16, 2),
            "kernel_ms": round(km, 3),
            "kernel_tflops": round(2.0 * nq * n * d / (km / 1e3) / 1e12, 1),
            "kernel_gbps": round(2.0 * ldh * n / (km / 1e3) / 1e9, 1),
            "recall_at_10": round(float(recall), 4)}), flush=True)
        del engs, out, q
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
