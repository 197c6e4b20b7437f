#!/usr/bin/env python3
# OPQ pre-transform (spec "opq": 1) against plain IVFPQ:
# recall@10 and QPS at equal nprobe, plus train time.
#
# Shape: bench.py "ivfpq_1m_d128_m16" (BASELINE.json configs[2]: 1M x 128,
# m=16, nlist=1024, low-rank synthetic generator, nq=10k, k=10);
# --workload ivfpq_2m_d768_m64 gives the d=768 shape (--n trims the row
# count); --small swaps in bench.py's 100k smoke workload and runs in
# seconds.
#
# Rows, all in one run on the same data, the workload's own knobs:
#   pq      IVFn,PQm              the workload as bench.py builds it
#   opq     OPQm,IVFn,PQm         rotation only (d_out = d)
#   opq_r   OPQm_<d3>,IVFn,PQm    d3 = the largest multiple of m <= d / 3
# Every row trains on the full shard (train_s is the wall time of that
# call, OPQ learning included), then for every nprobe of --nprobes reports
# recall@10 (faiss convention, as bench.py: the true nearest neighbour, by
# bench.exact_ground_truth, is among the returned 10; 2048 queries), the ms
# per step (bench.py protocol: warm-up steps, then the timed steps as
# HIP-graph replays of the whole search step; median of per-step HIP-event
# times) and QPS = nq / that. At --counters-nprobe the engine's own event
# timing of one eager step (gemm_ms includes the transform) is added.
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

KNOBS = ("coarse_bf16", "max_ppc", "ws_mb", "pq_lut_f16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true",
                    help="100k x 64 smoke shape (seconds)")
    ap.add_argument("--workload", default="ivfpq_1m_d128_m16",
                    choices=["ivfpq_1m_d128_m16", "ivfpq_2m_d768_m64"])
    ap.add_argument("--n", type=int, default=0, help="trim the shard to n rows")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nprobes", default="1,4,16,64")
    ap.add_argument("--counters-nprobe", type=int, default=16)
    ap.add_argument("--opq-niter", type=int, default=16)
    ap.add_argument("--graph", type=int, default=1,
                    help="time HIP-graph replays of the step (0: eager)")
    ap.add_argument("--rows", default="",
                    help="comma-separated subset of the rows (for a kernel "
                         "trace of one configuration); default all")
    args = ap.parse_args()

    import torch

    import bench
    from distributed_faiss_amd.hip_engine import HipEngine

    name = "ivfpq_100k_d64" if args.small else args.workload
    cfg = dict(bench.WORKLOADS[name])
    if args.n:
        cfg["n"] = args.n
    k, m, d = cfg["k"], cfg["m"], cfg["d"]
    d3 = max(m, (d // 3) // m * m)
    xb, q = bench.gen_shard(cfg, 0, "cuda")
    nq = q.shape[0]
    nq_eval = min(2048, nq)
    _gd, gt = bench.exact_ground_truth(xb, q[:nq_eval].contiguous(),
                                       cfg["metric"], k, "cuda")
    gt1 = gt[:, :1]
    common = {"type": "ivfpq", "dim": d, "metric": cfg["metric"],
              "nlist": cfg["nlist"], "nprobe": 1, "seed": 1234, "m": m,
              "nbits": 8}
    common.update({kn: cfg[kn] for kn in KNOBS if kn in cfg})
    specs = [
        ("pq", dict(common)),
        ("opq", dict(common, opq=1, opq_niter=args.opq_niter)),
        ("opq_r", dict(common, opq=1, opq_dim=d3, opq_niter=args.opq_niter)),
    ]
    if args.rows:
        want = args.rows.split(",")
        assert all(w in [s[0] for s in specs] for w in want), want
        specs = [s for s in specs if s[0] in want]
    nprobes = [int(v) for v in args.nprobes.split(",")
               if int(v) <= cfg["nlist"]]

    D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    qe = q[:nq_eval].contiguous()

    def recall(eng):
        _d, got = eng.search_dev(qe, k)
        return float((got == gt1).any(dim=1).float().mean().item())

    def timed(fn):
        """bench.py protocol; returns the median ms per step."""
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
        return statistics.median(ts)

    def counters(eng):
        eng.set_timing(True)
        eng.get_timing()  # reset
        eng.search_dev(q, k, D, I)
        torch.cuda.synchronize()
        t = eng.get_timing()
        eng.set_timing(False)
        return {kk: round(t[kk], 4)
                for kk in ("gemm_ms", "lut_ms", "scan_ms", "merge_ms")}

    rows = []
    for label, spec in specs:
        eng = HipEngine(spec=spec)
        torch.cuda.synchronize()
        t0 = time.time()
        eng.train_dev(xb)
        torch.cuda.synchronize()
        train_s = time.time() - t0
        t0 = time.time()
        eng.add_dev(xb)
        eng.search_dev(q[:16].contiguous(), k)  # finalize the lists
        torch.cuda.synchronize()
        add_s = time.time() - t0
        row = {"row": label, "d_in": d, "d_out": eng.transform_info()[2],
               "m": m, "train_s": round(train_s, 2), "add_s": round(add_s, 2),
               "sweep": []}
        for npb in nprobes:
            eng.nprobe = npb
            rec = recall(eng)
            ms = timed(lambda: eng.search_dev(q, k, D, I))
            row["sweep"].append({"nprobe": npb, "recall_at_10": round(rec, 4),
                                 "ms_median": round(ms, 4),
                                 "qps": round(nq / ms * 1e3)})
        eng.nprobe = min(args.counters_nprobe, cfg["nlist"])
        row["counters_nprobe"] = eng.nprobe
        row["counters"] = counters(eng)
        rows.append(row)
        print(f"[opq_bench] {row}", file=sys.stderr, flush=True)
        del eng
        torch.cuda.empty_cache()

    out = {"config": name, "n": int(xb.shape[0]), "nq": nq, "k": k,
           "steps": args.steps, "warmup": args.warmup, "graph": args.graph,
           "opq_niter": args.opq_niter, "rows": rows}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
