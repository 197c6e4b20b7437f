#!/usr/bin/env python3
# IVF-RaBitQ (spec "type": "ivfrabitq") against ivfpq at equal
# code stride on the same data, each with and without RFlat on top: build
# time (train + add) and the nprobe -> (recall@10, QPS) sweep.
#
# Shapes: bench.py "ivfpq_1m_d128_m16" (1M x 128; stride 32 = PQ m=32) and
# --workload ivfpq_100m8_d768_m64 (12.5M x 768; RaBitQ stride 112 against
# PQ m=96); --small swaps in bench.py's 100k smoke workload (PQ m=16).
#
# Rows: pq, pq_rflat, rabitq, rabitq_rflat, rabitq_rr (with the rotation).
# Recall is bench.py's: the true nearest neighbour (bench.exact_ground_truth)
# among the returned 10, over 2048 queries. QPS is nq / median step time,
# steps timed with HIP events after warm-up steps (eager: no graph).
#
# Prints one JSON line.
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NPROBES = (1, 2, 4, 8, 16, 32, 64)
PQ_M = {"ivfpq_1m_d128_m16": 32, "ivfpq_100m8_d768_m64": 96,
        "ivfpq_100k_d64": 16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--workload", default="ivfpq_1m_d128_m16",
                    choices=["ivfpq_1m_d128_m16", "ivfpq_100m8_d768_m64"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="", help="comma-separated subset")
    args = ap.parse_args()

    import torch

    import bench
    from distributed_faiss_amd.hip_engine import HipEngine

    name = "ivfpq_100k_d64" if args.small else args.workload
    cfg = dict(bench.WORKLOADS[name])
    k, d = cfg["k"], cfg["d"]
    xb, q = bench.gen_shard(cfg, 0, "cuda")
    nq = q.shape[0]
    qe = q[:min(2048, nq)].contiguous()
    _gd, gt = bench.exact_ground_truth(xb, qe, cfg["metric"], k, "cuda")
    gt1 = gt[:, :1]
    common = {"dim": d, "metric": cfg["metric"], "nlist": cfg["nlist"],
              "nprobe": 1, "seed": 1234}
    for kn in ("coarse_bf16", "max_ppc", "ws_mb"):
        if kn in cfg:
            common[kn] = cfg[kn]
    rf = {"refine": "fp32", "k_factor": 4}
    specs = [
        ("pq", dict(common, type="ivfpq", m=PQ_M[name], nbits=8)),
        ("pq_rflat", dict(common, type="ivfpq", m=PQ_M[name], nbits=8, **rf)),
        ("rabitq", dict(common, type="ivfrabitq")),
        ("rabitq_rflat", dict(common, type="ivfrabitq", **rf)),
        ("rabitq_rr", dict(common, type="ivfrabitq", rr=1)),
    ]
    if args.rows:
        specs = [s for s in specs if s[0] in args.rows.split(",")]

    D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    rows = []
    for label, spec in specs:
        eng = HipEngine(spec=spec)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.train_dev(xb)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        eng.add_dev(xb)
        eng.search_dev(q[:16].contiguous(), k)  # finalize the lists
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        row = {"row": label, "train_s": round(t1 - t0, 3),
               "add_s": round(t2 - t1, 3),
               "code_stride": int(eng.lib.dfann_code_stride(eng.h)),
               "sweep": []}
        for nprobe in NPROBES:
            if nprobe > cfg["nlist"]:
                break
            eng.nprobe = nprobe
            _d, got = eng.search_dev(qe, k)
            rec = float((got == gt1).any(dim=1).float().mean().item())
            for _ in range(args.warmup):
                eng.search_dev(q, k, D, I)
            ts = []
            for _ in range(args.steps):
                a = torch.cuda.Event(enable_timing=True)
                b = torch.cuda.Event(enable_timing=True)
                a.record()
                eng.search_dev(q, k, D, I)
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b))
            ms = statistics.median(ts)
            row["sweep"].append({"nprobe": nprobe, "recall_at_10": round(rec, 4),
                                 "ms_median": round(ms, 4),
                                 "qps": round(nq / ms * 1e3)})
        rows.append(row)
        print(f"[rabitq_bench] {row}", file=sys.stderr, flush=True)
        del eng
    print(json.dumps({"config": name, "n": int(xb.shape[0]), "nq": nq, "k": k,
                      "steps": args.steps, "warmup": args.warmup,
                      "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
