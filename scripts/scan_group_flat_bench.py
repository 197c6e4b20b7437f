#!/usr/bin/env python
# A/B of the grouped (list-major) scan against the pair-major scan on an
# ivf_flat index (spec "scan_group_flat"), k = 10, two shapes
# over the rows of a bench.py workload (default the 1M x 128 of
# ivfflat_1m_d128; --workload ivfpq_2m_d768_m64 --n 200000 --shapes dense is
# the d = 768 slice, only the rows of that workload being used):
#   dense   nlist=1024,  nprobe=16, nq=8192: ~128 pairs per list
#   sparse  nlist=16384, nprobe=1,  nq=1024: most groups hold one pair
# One index per shape, built with scan_group_flat: 1; the grouped side runs
# with DFANN_SCAN_GROUP_FLAT unset, the pair-major side is the same index under
# DFANN_SCAN_GROUP_FLAT=0 (the knob is read per call and leaves every launch
# of the default path as it is). The two sides alternate inside one process,
# warm-up first, eager steps timed with device events; scan_ms is the engine's
# own event timing (grouping + operands + scan on the grouped side).
# Recall@10 is against the exact top-10 of the fp32 rows.
# Prints one JSON line.
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

KNOB = "DFANN_SCAN_GROUP_FLAT"
SHAPES = {
    "dense": dict(nlist=1024, nprobe=16, nq=8192),
    "sparse": dict(nlist=16384, nprobe=1, nq=1024),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true",
                    help="100k rows, nlist / 8 (seconds)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3,
                    help="alternations of the two sides")
    ap.add_argument("--shapes", default="dense,sparse")
    ap.add_argument("--workload", default="ivfflat_1m_d128")
    ap.add_argument("--n", type=int, default=0, help="rows (0: the workload's)")
    ap.add_argument("--metric", type=int, default=-1,
                    help="0 IP, 1 L2 (-1: the workload's)")
    args = ap.parse_args()

    import torch

    import bench
    from distributed_faiss_amd.hip_engine import HipEngine

    cfg = dict(bench.WORKLOADS[args.workload], nq=8192)
    if args.n:
        cfg.update(n=args.n)
    if args.metric >= 0:
        cfg.update(metric=args.metric)
    if args.small:
        cfg.update(n=100_000, centers=1_000)
    k, d = 10, cfg["d"]
    xb, q_all = bench.gen_shard(cfg, 0, "cuda")
    _gd, gt_all = bench.exact_ground_truth(xb, q_all, cfg["metric"], k, "cuda")

    def step_ms(eng, q, D, I):
        ts = []
        for i in range(args.warmup + args.steps):
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            eng.search_dev(q, k, D, I)
            b.record()
            b.synchronize()
            if i >= args.warmup:
                ts.append(a.elapsed_time(b))
        return ts

    def scan_ms(eng, q, D, I):
        eng.set_timing(True)
        ms = []
        for i in range(args.warmup + args.steps):
            eng.get_timing()  # reset
            eng.search_dev(q, k, D, I)
            torch.cuda.synchronize()
            t = eng.get_timing()
            if i >= args.warmup:
                ms.append(t["scan_ms"])
        eng.set_timing(False)
        return ms, int(t["scan_rows"]), int(t["scan_launches"])

    out = {"workload": args.workload, "n": int(xb.shape[0]), "d": d,
           "metric": cfg["metric"], "k": k, "steps": args.steps,
           "warmup": args.warmup, "rounds": args.rounds, "shapes": {}}
    for name in args.shapes.split(","):
        sh = dict(SHAPES[name])
        if args.small:
            sh["nlist"] //= 8
        nq = sh["nq"]
        q, gt = q_all[:nq].contiguous(), gt_all[:nq]
        eng = HipEngine(spec={
            "type": "ivf_flat", "dim": d, "metric": cfg["metric"],
            "nlist": sh["nlist"], "nprobe": sh["nprobe"], "seed": 1234,
            "scan_group_flat": 1, "coarse_bf16": cfg.get("coarse_bf16", 0),
            "max_ppc": cfg.get("max_ppc", 256)})
        eng.train_dev(xb)
        eng.add_dev(xb)
        D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        sides = {"0": {"step": [], "scan": []}, "1": {"step": [], "scan": []}}
        for _ in range(args.rounds):
            for on in ("0", "1"):
                if on == "0":
                    os.environ[KNOB] = "0"
                else:
                    os.environ.pop(KNOB, None)
                s = sides[on]
                s["step"] += step_ms(eng, q, D, I)
                ms, s["scan_rows"], s["scan_launches"] = scan_ms(eng, q, D, I)
                s["scan"] += ms
                hit = (I[:, :, None] == gt[:, None, :]).any(1).float().mean()
                s["recall_at_10"] = round(float(hit.item()), 4)
        row = {"pairs_per_list": round(nq * sh["nprobe"] / sh["nlist"], 3),
               **sh}
        for on, s in sides.items():
            med = statistics.median(s["step"])
            row["scan_group_flat_" + on] = {
                "ms_median": round(med, 4), "ms_min": round(min(s["step"]), 4),
                "ms_max": round(max(s["step"]), 4),
                "qps": round(nq / med * 1e3, 1),
                "scan_ms": round(statistics.median(s["scan"]), 4),
                "scan_rows": s["scan_rows"],
                "scan_launches": s["scan_launches"],
                "recall_at_10": s["recall_at_10"]}
        a, b = row["scan_group_flat_0"], row["scan_group_flat_1"]
        row["step_speedup"] = round(a["ms_median"] / b["ms_median"], 3)
        row["scan_speedup"] = round(a["scan_ms"] / b["scan_ms"], 3)
        out["shapes"][name] = row
        print(f"[scan_group_flat_bench] {name}: {row}", file=sys.stderr,
              flush=True)
        del eng
        torch.cuda.empty_cache()
    os.environ.pop(KNOB, None)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
