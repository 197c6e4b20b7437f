#!/usr/bin/env python3
# 4-bit PQ (spec "nbits": 4) against 8-bit PQ: recall, step
# time and scan throughput at equal code bytes, at half the code bytes, and
# at half the code bytes with a refine stage on top.
#
# Shape: bench.py "ivfpq_1m_d128_m16" (1M x 128, m=16, nlist=1024, low-rank
# synthetic generator, nq=10k, k=10); --workload ivfpq_2m_d768_m64 gives the
# d=768 shape; --small swaps in bench.py's 100k smoke workload and runs in
# seconds.
#
# Rows, all in one run on the same data:
#   pq8_bench   the workload as bench.py runs it (8-bit, its own knobs)
#   pq8_exact   8-bit, exact fp32 LUT built in the scan kernel
#   pq4_2m      PQ(2m)x4: the same code bytes per vector as PQ(m)x8
#   pq4_m       PQ(m)x4: half the code bytes
#   pq4_m_rf16  PQ(m)x4 + refine fp16, k_factor 4
# The two 8-bit rows share one training through set_trained, as do the two
# PQ(m)x4 rows; the 4-bit engines train their own 16-codeword codebooks
# from the same seed, which makes their coarse centroids the 8-bit rows'
# ("coarse_shared" reports the comparison).
#
# For every row nprobe is swept over 1, 2, 4, ... to the smallest value
# with recall@10 >= --target-recall (faiss convention, as bench.py: the
# true nearest neighbour, by bench.exact_ground_truth, is among the
# returned 10; 2048 queries); a row that never reaches the target is
# reported at the largest nprobe tried, with "reached": false. At that
# nprobe the row reports ms per step (bench.py protocol: warm-up steps,
# then the timed steps as HIP-graph replays of the whole search step;
# median and mean of per-step HIP-event times), the engine's own scan_ms
# and scan_bytes / scan_ms of one step, the recall, the code bytes per
# vector and the HBM the engine took. Every row is also timed at the
# pq8_exact row's nprobe, so equal scanned rows can be compared.
#
# The comparison base is the 8-bit rows of the SAME run.
#
# Prints one JSON line.
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NPROBES = (1, 2, 4, 8, 16, 32, 64, 128, 256)
KNOBS = ("coarse_bf16", "max_ppc", "ws_mb", "pq_precomputed", "pq_lut_f16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true",
                    help="100k x 64 smoke shape (seconds)")
    ap.add_argument("--workload", default="ivfpq_1m_d128_m16",
                    choices=["ivfpq_1m_d128_m16", "ivfpq_2m_d768_m64"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--target-recall", type=float, default=0.95)
    ap.add_argument("--graph", type=int, default=1,
                    help="time HIP-graph replays of the step (0: eager)")
    ap.add_argument("--rows", default="",
                    help="comma-separated subset of the rows (for a kernel "
                         "trace of one configuration); default all")
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    from distributed_faiss_amd.hip_engine import HipEngine

    name = "ivfpq_100k_d64" if args.small else args.workload
    cfg = dict(bench.WORKLOADS[name])
    k, m, d = cfg["k"], cfg["m"], cfg["d"]
    assert d % (2 * m) == 0, "PQ(2m)x4 needs dim % 2m == 0"
    xb, q = bench.gen_shard(cfg, 0, "cuda")
    nq = q.shape[0]
    nq_eval = min(2048, nq)
    _gd, gt = bench.exact_ground_truth(xb, q[:nq_eval].contiguous(),
                                       cfg["metric"], k, "cuda")
    gt1 = gt[:, :1]
    common = {"type": "ivfpq", "dim": d, "metric": cfg["metric"],
              "nlist": cfg["nlist"], "nprobe": 1, "seed": 1234}
    for kn in ("coarse_bf16", "max_ppc", "ws_mb"):
        if kn in cfg:
            common[kn] = cfg[kn]
    own = {kn: cfg[kn] for kn in KNOBS if kn in cfg}  # bench.py's knobs
    specs = [
        ("pq8_bench", dict(common, m=m, nbits=8, **own), None),
        ("pq8_exact", dict(common, m=m, nbits=8, pq_lut_f16=0,
                           pq_lut_global=0), "pq8_bench"),
        ("pq4_2m", dict(common, m=2 * m, nbits=4), None),
        ("pq4_m", dict(common, m=m, nbits=4), None),
        ("pq4_m_rf16", dict(common, m=m, nbits=4, refine="fp16",
                            k_factor=4), "pq4_m"),
    ]

    if args.rows:
        want = args.rows.split(",")
        assert all(w in [s[0] for s in specs] for w in want), want
        specs = [s for s in specs if s[0] in want]

    def hbm_gib():
        free_b, total_b = torch.cuda.mem_get_info()
        return round((total_b - free_b) / 2 ** 30, 3)

    hbm0 = hbm_gib()  # data + ground truth, before any engine
    engines, hbm, trained, coarse_shared = {}, {}, {}, True
    for label, spec, share in specs:
        before = hbm_gib()
        eng = HipEngine(spec=spec)
        if share in trained:
            eng.set_trained(*trained[share])
        else:
            eng.train_dev(xb)
            trained[label] = (eng.get_centroids(), eng.get_codebooks())
            first = trained[specs[0][0]][0]
            coarse_shared = coarse_shared and np.array_equal(
                trained[label][0], first)
        eng.add_dev(xb)
        eng.search_dev(q[:16].contiguous(), k)  # finalize the lists
        torch.cuda.synchronize()
        engines[label] = eng
        hbm[label] = round(hbm_gib() - before, 3)
        print(f"[pq4_bench] built {label}: +{hbm[label]} GiB",
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

    def scan_counters(eng):
        """The engine's own event timing of one eager step."""
        eng.set_timing(True)
        eng.get_timing()  # reset
        eng.search_dev(q, k, D, I)
        torch.cuda.synchronize()
        t = eng.get_timing()
        eng.set_timing(False)
        gbs = t["scan_bytes"] / t["scan_ms"] / 1e6 if t["scan_ms"] else 0.0
        return {"scan_ms": round(t["scan_ms"], 4),
                "scan_rows": int(t["scan_rows"]),
                "scan_gb_per_s": round(gbs, 1),
                "lut_ms": round(t["lut_ms"], 4)}

    # nprobe sweeps first: the equal-work column needs pq8_exact's nprobe
    chosen = {}
    for label, _spec, _share in specs:
        eng = engines[label]
        pick, rec, reached = None, 0.0, False
        for cand in NPROBES:
            if cand > cfg["nlist"]:
                break
            eng.nprobe = cand
            pick, rec = cand, recall(eng)
            if rec >= args.target_recall:
                reached = True
                break
        chosen[label] = (pick, rec, reached)
    ref_row = "pq8_exact" if "pq8_exact" in chosen else specs[0][0]
    nprobe_ref = chosen[ref_row][0]

    rows = []
    for label, spec, _share in specs:
        eng = engines[label]
        pick, rec, reached = chosen[label]
        eng.nprobe = pick
        med, mean = timed(lambda: eng.search_dev(q, k, D, I))
        stride = int(eng.lib.dfann_code_stride(eng.h))
        row = {"row": label, "m": spec["m"], "nbits": spec["nbits"],
               "refine": spec.get("refine"), "nprobe": pick,
               "recall_at_10": round(rec, 4), "reached": reached,
               "ms_median": round(med, 4), "ms_mean": round(mean, 4),
               "code_bytes": (spec["m"] * spec["nbits"] + 7) // 8,
               "code_stride": stride, "engine_hbm_gib": hbm[label]}
        row.update(scan_counters(eng))
        # the same step at the pq8_exact row's nprobe: equal scanned rows
        eng.nprobe = nprobe_ref
        med_r, _mean_r = timed(lambda: eng.search_dev(q, k, D, I))
        ref = scan_counters(eng)
        row["ms_median_at_pq8_nprobe"] = round(med_r, 4)
        row["scan_ms_at_pq8_nprobe"] = ref["scan_ms"]
        row["scan_gb_per_s_at_pq8_nprobe"] = ref["scan_gb_per_s"]
        row["recall_at_pq8_nprobe"] = round(recall(eng), 4)
        rows.append(row)
        print(f"[pq4_bench] {row}", file=sys.stderr, flush=True)

    base_ms = next(r for r in rows if r["row"] == ref_row)["ms_median"]
    for row in rows:
        row["ms_over_" + ref_row] = round(row["ms_median"] / base_ms, 4)
    out = {"config": name, "n": int(xb.shape[0]), "nq": nq, "k": k,
           "target_recall": args.target_recall, "steps": args.steps,
           "warmup": args.warmup, "graph": args.graph,
           "nprobe_ref": nprobe_ref, "ref_row": ref_row, "coarse_shared": bool(coarse_shared),
           "hbm_before_engines_gib": hbm0, "hbm_total_gib": hbm_gib(),
           "rows": rows}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
