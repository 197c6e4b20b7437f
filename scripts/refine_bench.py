#!/usr/bin/env python3
# Refine-stage cost and what it buys: recall against scanned work.
#
# Shape: BASELINE configs[2] (bench.py "ivfpq_1m_d128_m16": 1M x 128 IVFPQ
# m=16 nlist=1024, low-rank synthetic generator, nq=10k, k=10); --small
# swaps in bench.py's 100k smoke workload and runs in seconds.
#
# For refine in {off, fp16, fp32} and k_factor in {1, 1.6, 4, 10} (one row
# for off: k_factor has no meaning there) nprobe is swept over
# 1, 2, 4, ... to the smallest value with recall@10 >= --target-recall
# (faiss convention, as bench.py: the true nearest neighbour, by
# bench.exact_ground_truth, is among the returned 10; 2048 queries). At
# that nprobe the row reports ms per step (bench.py protocol: warm-up
# steps, then the timed steps as HIP-graph replays of the whole search
# step; median and mean of per-step HIP-event times), the recall, the
# nprobe and the HBM in use. A configuration that never reaches the target
# is reported at the largest nprobe tried, with "reached": false. Each row
# is also timed at the refine-off row's nprobe ("ms_median_at_off_nprobe"),
# so the k_factor=1.6 (k'=16) and k_factor=4 (k'=40) rows show at equal
# scanned work what leaving the register top-k path costs.
#
# Every row is compared against the refine-off row of the SAME run: the
# same commit's base path on the same data and trained artifacts (the
# three engines share one training through set_trained).
#
# Prints one JSON line.
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

K_FACTORS = (1, 1.6, 4, 10)
NPROBES = (1, 2, 4, 8, 16, 32, 64, 128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true",
                    help="100k x 64 smoke shape (seconds)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--target-recall", type=float, default=0.95)
    ap.add_argument("--graph", type=int, default=1,
                    help="time HIP-graph replays of the step (0: eager)")
    args = ap.parse_args()

    import torch

    import bench
    from distributed_faiss_amd.hip_engine import HipEngine

    name = "ivfpq_100k_d64" if args.small else "ivfpq_1m_d128_m16"
    cfg = dict(bench.WORKLOADS[name])
    k = cfg["k"]
    xb, q = bench.gen_shard(cfg, 0, "cuda")
    nq = q.shape[0]
    nq_eval = min(2048, nq)
    _gd, gt = bench.exact_ground_truth(xb, q[:nq_eval].contiguous(),
                                       cfg["metric"], k, "cuda")
    gt1 = gt[:, :1]
    spec = {"type": cfg["type"], "dim": cfg["d"], "metric": cfg["metric"],
            "nlist": cfg["nlist"], "m": cfg["m"], "nbits": cfg["nbits"],
            "nprobe": 1, "seed": 1234, "pq_lut_f16": cfg.get("pq_lut_f16", 0)}

    def hbm_gib():
        free_b, total_b = torch.cuda.mem_get_info()
        return round((total_b - free_b) / 2 ** 30, 3)

    hbm0 = hbm_gib()  # data + ground truth, before any engine
    base = HipEngine(spec=spec)
    base.train_dev(xb)
    cent, cb = base.get_centroids(), base.get_codebooks()
    engines, hbm = {}, {}
    for refine in ("off", "fp16", "fp32"):
        before = hbm_gib()
        if refine == "off":
            eng = base
        else:
            eng = HipEngine(spec=dict(spec, refine=refine))
            eng.set_trained(cent, cb)
        eng.add_dev(xb)
        eng.search_dev(q[:16].contiguous(), k)  # finalize the lists
        torch.cuda.synchronize()
        engines[refine] = eng
        hbm[refine] = round(hbm_gib() - before, 3)
        print(f"[refine_bench] built {refine}: +{hbm[refine]} GiB",
              file=sys.stderr, flush=True)

    D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    qe = q[:nq_eval].contiguous()

    def recall(eng):
        _d, got = eng.search_dev(qe, k)
        return float((got == gt1).any(dim=1).float().mean().item())

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

    rows = []
    for refine in ("off", "fp16", "fp32"):
        eng = engines[refine]
        for kf in ((None,) if refine == "off" else K_FACTORS):
            if kf is not None:
                eng.k_factor = kf
            chosen, rec, reached = None, 0.0, False
            for cand in NPROBES:
                if cand > cfg["nlist"]:
                    break
                eng.nprobe = cand
                chosen, rec = cand, recall(eng)
                if rec >= args.target_recall:
                    reached = True
                    break
            eng.nprobe = chosen
            med, mean = timed(lambda: eng.search_dev(q, k, D, I))
            row = {"refine": refine, "k_factor": kf, "nprobe": chosen,
                   "recall_at_10": round(rec, 4), "reached": reached,
                   "ms_median": round(med, 4), "ms_mean": round(mean, 4),
                   "engine_hbm_gib": hbm[refine]}
            # the same step at the refine-off row's nprobe: isolates what
            # k' costs (k' <= 16 keeps the base stage on the register
            # top-k path, k' > 16 moves it to the LDS-selection path)
            nprobe_ref = rows[0]["nprobe"] if rows else chosen
            eng.nprobe = nprobe_ref
            med_r, _mean_r = timed(lambda: eng.search_dev(q, k, D, I))
            row["ms_median_at_off_nprobe"] = round(med_r, 4)
            row["recall_at_off_nprobe"] = round(recall(eng), 4)
            rows.append(row)
            print(f"[refine_bench] {row}", file=sys.stderr, flush=True)

    off_ms = rows[0]["ms_median"]
    for row in rows:
        row["ms_over_refine_off"] = round(row["ms_median"] / off_ms, 4)
    out = {"config": name, "n": int(xb.shape[0]), "nq": nq, "k": k,
           "target_recall": args.target_recall, "steps": args.steps,
           "warmup": args.warmup, "graph": args.graph,
           "hbm_before_engines_gib": hbm0, "hbm_total_gib": hbm_gib(),
           "rows": rows}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
