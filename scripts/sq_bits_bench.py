#!/usr/bin/env python3
# SQ4 / SQ6 (spec "sq_type": "4bit" | "6bit") against SQ8:
# scan rate, step time and recall, all from the same data in one run.
#
# Shape: bench.py "ivfsq8_10m_d128" (10M x 128, nlist=4096, the
# configs[4]-shaped HBM-bound workload BASELINE.md has an SQ8 row for;
# nq=10k, k=10); --small shrinks it to 200k rows / 256 lists and runs in
# seconds.
#
# Rows: sq8, sq6, sq4, and sq6_rflat / sq4_rflat (refine fp32, k_factor 4).
# sq8 is trained by the engine; the others take its centroids and ranges
# through set_trained (training is the same at every width: the same
# kernels over the same residuals), so all five index the same lists.
#
# Per row, for every nprobe of the sweep: recall@10 against exact ground
# truth (faiss convention, as bench.py: the true nearest neighbour is among
# the returned 10; 2048 queries). At --nprobe (default 32) the row reports,
# as medians over the timed steps: the engine's own scan_ms, rows/s and
# GB/s of algorithmic code bytes (dfann_get_timing of eager steps), and
# ms per step / QPS (bench.py protocol: warm-up, then HIP-graph replays of
# the whole search step timed by HIP events).
#
# The acceptance floor (BASELINE.md "SQ4 / SQ6"): sq4 and sq6 scan at least as
# many rows/s as sq8 in the same run; "floor" reports both ratios.
#
# Prints one JSON line.
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NPROBES = (1, 2, 4, 8, 16, 32, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true",
                    help="200k x 128, nlist=256 (seconds)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nprobe", type=int, default=32,
                    help="nprobe of the timed rows")
    ap.add_argument("--graph", type=int, default=1,
                    help="time HIP-graph replays of the step (0: eager)")
    ap.add_argument("--rows", default="",
                    help="comma-separated subset of the rows; default all")
    args = ap.parse_args()

    import torch

    import bench
    from distributed_faiss_amd.hip_engine import HipEngine

    cfg = dict(bench.WORKLOADS["ivfsq8_10m_d128"])
    if args.small:
        cfg.update(n=200_000, nlist=256, centers=2_000, nq=2_000)
    k, d = cfg["k"], cfg["d"]
    xb, q = bench.gen_shard(cfg, 0, "cuda")
    nq = q.shape[0]
    nq_eval = min(2048, nq)
    qe = q[:nq_eval].contiguous()
    _gd, gt = bench.exact_ground_truth(xb, qe, cfg["metric"], k, "cuda")
    gt1 = gt[:, :1]
    common = {"type": "ivfsq", "dim": d, "metric": cfg["metric"],
              "nlist": cfg["nlist"], "nprobe": 1, "seed": 1234}
    specs = [
        ("sq8", dict(common, sq_type="8bit")),
        ("sq6", dict(common, sq_type="6bit")),
        ("sq4", dict(common, sq_type="4bit")),
        ("sq6_rflat", dict(common, sq_type="6bit", refine="fp32", k_factor=4)),
        ("sq4_rflat", dict(common, sq_type="4bit", refine="fp32", k_factor=4)),
    ]
    if args.rows:
        want = args.rows.split(",")
        assert all(w in [s[0] for s in specs] for w in want), want
        specs = [s for s in specs if s[0] in want or s[0] == "sq8"]

    def hbm_gib():
        free_b, total_b = torch.cuda.mem_get_info()
        return round((total_b - free_b) / 2 ** 30, 3)

    D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    I = torch.empty((nq, k), dtype=torch.int64, device="cuda")

    def recall(eng):
        _d, got = eng.search_dev(qe, k)
        return float((got == gt1).any(dim=1).float().mean().item())

    def timed(fn):
        """bench.py protocol; returns median ms per step."""
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

    def scan_counters(eng):
        """The engine's own event timing, one eager step at a time."""
        eng.set_timing(True)
        ms, rows, nbytes = [], 0, 0
        for i in range(args.warmup + args.steps):
            eng.get_timing()  # reset
            eng.search_dev(q, k, D, I)
            torch.cuda.synchronize()
            t = eng.get_timing()
            if i >= args.warmup:
                ms.append(t["scan_ms"])
                rows, nbytes = int(t["scan_rows"]), int(t["scan_bytes"])
        eng.set_timing(False)
        med = statistics.median(ms)
        return {"scan_ms": round(med, 4), "scan_ms_min": round(min(ms), 4),
                "scan_ms_max": round(max(ms), 4), "scan_rows": rows,
                "scan_rows_per_s": round(rows / med * 1e3, 1),
                "scan_gb_per_s": round(nbytes / med / 1e6, 1)}

    rows, trained = [], None
    for label, spec in specs:
        before = hbm_gib()
        eng = HipEngine(spec=spec)
        if trained is None:
            eng.train_dev(xb)
            trained = (eng.get_centroids(), None) + eng.get_sq_params()
        else:
            eng.set_trained(*trained)
        eng.add_dev(xb)
        eng.search_dev(q[:16].contiguous(), k)  # finalize the lists
        torch.cuda.synchronize()
        row = {"row": label, "sq_type": spec["sq_type"],
               "refine": spec.get("refine"),
               "code_stride": int(eng.lib.dfann_code_stride(eng.h)),
               "engine_hbm_gib": round(hbm_gib() - before, 3), "recall_at_10": {}}
        print(f"[sq_bits_bench] built {label}: +{row['engine_hbm_gib']} GiB",
              file=sys.stderr, flush=True)
        for cand in NPROBES:
            if cand > cfg["nlist"]:
                break
            eng.nprobe = cand
            row["recall_at_10"][str(cand)] = round(recall(eng), 4)
        eng.nprobe = min(args.nprobe, cfg["nlist"])
        row["nprobe"] = eng.nprobe
        row.update(scan_counters(eng))
        med = timed(lambda: eng.search_dev(q, k, D, I))
        row["ms_median"] = round(med, 4)
        row["qps"] = round(nq / med * 1e3, 1)
        rows.append(row)
        print(f"[sq_bits_bench] {row}", file=sys.stderr, flush=True)
        del eng  # one index resident at a time
        torch.cuda.empty_cache()

    by = {r["row"]: r for r in rows}
    floor = {}
    for label in ("sq6", "sq4"):
        if label in by:
            floor[label + "_rows_per_s_over_sq8"] = round(
                by[label]["scan_rows_per_s"] / by["sq8"]["scan_rows_per_s"], 4)
    floor["met"] = bool(floor) and all(v >= 1.0 for v in floor.values())
    out = {"config": "ivfsq8_10m_d128" + ("(small)" if args.small else ""),
           "n": int(xb.shape[0]), "nq": nq, "k": k, "nlist": cfg["nlist"],
           "steps": args.steps, "warmup": args.warmup, "graph": args.graph,
           "floor": floor, "rows": rows}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
