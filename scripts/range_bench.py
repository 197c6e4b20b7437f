#!/usr/bin/env python3
# Range-search cost next to the top-k search it shares its scans with.
#
# Shapes: BASELINE configs[2] (bench.py "ivfpq_1m_d128_m16": 1M x 128 IVFPQ
# m=16 nlist=1024) and the 1M SQ8 shape ("ivfsq8_1m_d128"), nq=10k,
# nprobe=16; --small swaps in bench.py's 100k smoke workload only.
#
# Three radii per shape, giving roughly 10, 100 and 1000 hits per query:
# the median over 64 sample queries of the rank-10/100/1000 distance among
# ALL rows of their probed lists (one range call with the including radius).
#
# Per shape and radius it reports
#   * ms per batch of range_search_dev (eager: the call synchronizes once
#     to read the result size, so it cannot be a graph replay) next to
#     search_dev at k=10, eager and as a HIP-graph replay;
#   * the scan / LUT split from dfann_timing per call, the count pass alone
#     (a call with an excluding radius runs no fill pass) and the fill pass
#     as the difference, each with its achieved code bytes per second;
#   * hits per query.
#
# Prints one JSON line per shape.
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FLT_MAX = 3.4028234663852886e38


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true",
                    help="100k x 64 smoke shape only (seconds)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nprobe", type=int, default=16)
    args = ap.parse_args()

    import torch

    import bench
    from distributed_faiss_amd.hip_engine import HipEngine

    names = (["ivfpq_100k_d64"] if args.small
             else ["ivfpq_1m_d128_m16", "ivfsq8_1m_d128"])

    def timed(fn, graph=False):
        for _ in range(args.warmup):
            fn()
        step = fn
        if graph:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            g.replay()
            step = g.replay
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.steps):
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            step()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return round(statistics.median(ts), 4)

    for name in names:
        cfg = dict(bench.WORKLOADS[name])
        k = cfg["k"]
        xb, q = bench.gen_shard(cfg, 0, "cuda")
        spec = {"type": cfg["type"], "dim": cfg["d"], "metric": cfg["metric"],
                "nlist": cfg["nlist"], "m": cfg["m"], "nbits": cfg["nbits"],
                "sq_type": cfg.get("sq_type", "fp16"), "nprobe": args.nprobe,
                "seed": 1234, "pq_lut_f16": cfg.get("pq_lut_f16", 0)}
        eng = HipEngine(spec=spec)
        eng.train_dev(xb)
        eng.add_dev(xb)
        eng.nprobe = args.nprobe
        nq = q.shape[0]
        l2 = cfg["metric"] == 1
        out = {"config": name, "n": eng.ntotal, "nq": nq, "k": k,
               "nprobe": args.nprobe, "steps": args.steps, "legs": {}}

        def split(fn, calls=4):
            """dfann_timing per call: scan / LUT ms and scanned bytes."""
            fn()
            eng.set_timing(True)
            eng.get_timing()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            t = eng.get_timing()
            eng.set_timing(False)
            return {"scan_ms": round(t["scan_ms"] / calls, 4),
                    "lut_ms": round(t["lut_ms"] / calls, 4),
                    "merge_ms": round(t["merge_ms"] / calls, 4),
                    "scan_launches": t["scan_launches"] // calls,
                    "scan_gb": round(t["scan_bytes"] / calls / 1e9, 4)}

        def gbps(gb, ms):
            return round(gb / (ms / 1e3), 1) if ms > 0 else None

        D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        top = {"ms_eager": timed(lambda: eng.search_dev(q, k, D, I)),
               "ms_graph": timed(lambda: eng.search_dev(q, k, D, I), True)}
        top.update(split(lambda: eng.search_dev(q, k, D, I)))
        top["scan_gbps"] = gbps(top["scan_gb"], top["scan_ms"])
        out["legs"][f"search_k{k}"] = top

        # radii from the full distance distribution of 64 sample queries
        lims, Dall, _ = eng.range_search_dev(
            q[:64].contiguous(), FLT_MAX if l2 else -FLT_MAX)
        lims, Dall = lims.cpu().numpy(), Dall.cpu().numpy()
        radii = {}
        for hits in (10, 100, 1000):
            vals = []
            for i in range(64):
                d = np.sort(Dall[lims[i]:lims[i + 1]])
                if not l2:
                    d = d[::-1]
                if d.size > hits:
                    vals.append((float(d[hits - 1]) + float(d[hits])) / 2)
            radii[hits] = float(np.median(vals))

        none = 0.0 if l2 else FLT_MAX
        count = split(lambda: eng.range_search_dev(q, none))
        count["ms_eager"] = timed(lambda: eng.range_search_dev(q, none))
        count["scan_gbps"] = gbps(count["scan_gb"], count["scan_ms"])
        out["legs"]["range_count_only"] = count
        for hits, r in radii.items():
            leg = {"radius": r,
                   "ms_eager": timed(lambda r=r: eng.range_search_dev(q, r))}
            leg.update(split(lambda r=r: eng.range_search_dev(q, r)))
            lm, _d, _i = eng.range_search_dev(q, r)
            leg["hits_per_query"] = round(int(lm[-1]) / nq, 2)
            fill_ms = leg["scan_ms"] - count["scan_ms"]
            leg["fill_ms"] = round(fill_ms, 4)
            leg["fill_gbps"] = gbps(leg["scan_gb"] / 2, fill_ms)
            leg["scan_over_topk_scan"] = round(leg["scan_ms"] / top["scan_ms"], 3)
            leg["ms_over_topk_eager"] = round(leg["ms_eager"] / top["ms_eager"], 3)
            out["legs"][f"range_{hits}"] = leg
            print(f"[range_bench] {name} ~{hits} hits: {leg}", file=sys.stderr,
                  flush=True)
        print(json.dumps(out), flush=True)
        del eng, xb, q
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
