#!/usr/bin/env python3
# Filtered-search cost: in-kernel allow-bitmap vs the x3 over-fetch.
#
# Shape: BASELINE configs[2] (bench.py "ivfpq_1m_d128_m16": 1M x 128 IVFPQ
# m=16 nlist=1024, low-rank synthetic generator, nq=10k, k=10, nprobe=16);
# --small swaps in bench.py's 100k smoke workload and runs in seconds.
#
# Reports ms per step (bench.py protocol: warm-up steps, then the timed
# steps as HIP-graph replays of the whole search step; the median and the
# mean of per-step HIP-event times) for
#   1. search_dev at k           — the unfiltered floor
#   2. search_dev at 3k          — what search_with_filter's over-fetch runs
#   3. search_filtered_dev at k with 100 % / 50 % / 1 % of the ids allowed
# plus an upper bound on the id->position translate kernel's share of (3):
# a ONE-query filtered step minus a one-query unfiltered step (the translate
# kernel runs over all ntotal positions whatever nq is).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true",
                    help="100k x 64 smoke shape (seconds)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--graph", type=int, default=1,
                    help="time HIP-graph replays of the step (0: eager)")
    args = ap.parse_args()

    import torch

    import bench
    from distributed_faiss_amd.hip_engine import HipEngine, pack_allow_bits

    name = "ivfpq_100k_d64" if args.small else "ivfpq_1m_d128_m16"
    cfg = dict(bench.WORKLOADS[name])
    k = cfg["k"]
    xb, q = bench.gen_shard(cfg, 0, "cuda")
    spec = {"type": cfg["type"], "dim": cfg["d"], "metric": cfg["metric"],
            "nlist": cfg["nlist"], "m": cfg["m"], "nbits": cfg["nbits"],
            "nprobe": args.nprobe, "seed": 1234,
            "pq_lut_f16": cfg.get("pq_lut_f16", 0)}
    eng = HipEngine(spec=spec)
    eng.train_dev(xb)
    eng.add_dev(xb)
    eng.nprobe = args.nprobe
    n = eng.ntotal
    nq = q.shape[0]

    rng = np.random.default_rng(5)

    def bits(frac):
        allow = np.ones(n, bool) if frac >= 1.0 else rng.random(n) < frac
        return torch.as_tensor(pack_allow_bits(allow)).cuda(), int(allow.sum())

    def timed(fn):
        """bench.py protocol; returns (median_ms, mean_ms) per step."""
        for _ in range(args.warmup):
            fn()
        step = fn
        if args.graph:
            fn()  # no first-use allocation inside the capture
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
        return statistics.median(ts), statistics.fmean(ts)

    out = {"config": name, "n": n, "nq": nq, "k": k, "nprobe": args.nprobe,
           "steps": args.steps, "warmup": args.warmup, "graph": args.graph,
           "ms_per_step": {}}

    def leg(label, fn):
        med, mean = timed(fn)
        out["ms_per_step"][label] = {"median": round(med, 4),
                                     "mean": round(mean, 4)}
        print(f"[filter_bench] {label}: median {med:.3f} ms  mean {mean:.3f} ms",
              file=sys.stderr, flush=True)
        return med

    def buffers(kk):
        return (torch.empty((nq, kk), dtype=torch.float32, device="cuda"),
                torch.empty((nq, kk), dtype=torch.int64, device="cuda"))

    D1, I1 = buffers(k)
    D3, I3 = buffers(3 * k)
    t_k = leg(f"search_k{k}", lambda: eng.search_dev(q, k, D1, I1))
    t_3k = leg(f"search_k{3 * k}", lambda: eng.search_dev(q, 3 * k, D3, I3))
    t_f = {}
    for frac in (1.0, 0.5, 0.01):
        bt, cnt = bits(frac)
        label = f"filtered_k{k}_{int(frac * 100)}pct"
        t_f[frac] = leg(label, lambda bt=bt: eng.search_filtered_dev(
            q, k, bt, n, D1, I1))
        out["ms_per_step"][label]["allowed"] = cnt
        if frac >= 1.0:  # the ALL filter must change nothing
            Dr, Ir = eng.search_dev(q, k)
            assert torch.equal(I1, Ir) and torch.equal(D1, Dr)

    # translate kernel alone: a filtered search of ONE query runs the same
    # k_filter_id2pos over all ntotal positions; an unfiltered search of
    # one query is everything else in that step. Both are launch-latency
    # sized, so the difference is an upper bound on the translate cost.
    q1 = q[:1].contiguous()
    Da, Ia = (torch.empty((1, k), dtype=torch.float32, device="cuda"),
              torch.empty((1, k), dtype=torch.int64, device="cuda"))
    bt, _ = bits(1.0)
    t1 = leg("one_query_search", lambda: eng.search_dev(q1, k, Da, Ia))
    t1f = leg("one_query_filtered", lambda: eng.search_filtered_dev(
        q1, k, bt, n, Da, Ia))
    out["translate_ms_upper_bound"] = round(max(t1f - t1, 0.0), 4)
    out["ratios"] = {
        "filtered_100pct_over_search_k": round(t_f[1.0] / t_k, 4),
        "filtered_100pct_over_overfetch": round(t_f[1.0] / t_3k, 4),
        "filtered_50pct_over_overfetch": round(t_f[0.5] / t_3k, 4),
        "filtered_1pct_over_overfetch": round(t_f[0.01] / t_3k, 4),
        "overfetch_over_search_k": round(t_3k / t_k, 4),
    }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
