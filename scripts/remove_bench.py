#!/usr/bin/env python3
# Removal cost, and what a search costs afterwards.
#
# Shapes: the 10M x 128 SQ8 shard (bench.py "ivfsq8_10m_d128", 1.28 GB of
# codes) and the headline-shaped PQ shard ("ivfpq_100m8_d768_m64", 12.5M x
# 64 B codes); --small swaps in bench.py's 100k smoke workload only.
#
# Per shape the index is built once and saved; each removal runs on a fresh
# load of that file, so every fraction starts from the same lists.
#   * remove_ids_dev of a seeded random 1 %, 10 % and 50 % of the ids: wall
#     ms of the whole call (keep bits, scan, compaction, offsets, the syncs
#     between slab windows), the code bytes it moved per second (read +
#     write: 2 * kept rows * stride) and that as a fraction of a plain
#     device-to-device copy of the same bytes measured in the same process —
#     the streaming-copy rate is the compaction's ceiling. The 50 % case also
#     runs with DFANN_REMOVE_LANES=1 (one thread per row instead of one per
#     16-byte unit).
#   * search after the 50 % removal (k and nprobe of the workload, eager,
#     median ms per batch and QPS) next to a FRESH index that got the same
#     trained artifacts and only the surviving rows.
#
# Prints one JSON line per shape.
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true",
                    help="100k x 64 smoke shape only (seconds)")
    ap.add_argument("--configs", default="ivfsq8_10m_d128,ivfpq_100m8_d768_m64")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nprobe", type=int, default=16)
    args = ap.parse_args()

    import torch

    import bench
    from distributed_faiss_amd.hip_engine import HipEngine, HipProvider

    names = ["ivfpq_100k_d64"] if args.small else args.configs.split(",")

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
        return statistics.median(ts)

    def pack_bits(mask):
        """bool cuda tensor over ids -> int32 bitmap words on the device."""
        n = mask.shape[0]
        words = (n + 31) // 32
        m = torch.zeros(words * 32, dtype=torch.int64, device="cuda")
        m[:n] = mask
        w = (m.view(words, 32) << torch.arange(32, device="cuda")).sum(1)
        return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)

    for name in names:
        cfg = dict(bench.WORKLOADS[name])
        k = cfg["k"]
        xb, q = bench.gen_shard(cfg, 0, "cuda")
        spec = {"type": cfg["type"], "dim": cfg["d"], "metric": cfg["metric"],
                "nlist": cfg["nlist"], "m": cfg["m"], "nbits": cfg["nbits"],
                "sq_type": cfg.get("sq_type", "fp16"), "nprobe": args.nprobe,
                "seed": 1234, "pq_lut_f16": cfg.get("pq_lut_f16", 0),
                "coarse_bf16": cfg.get("coarse_bf16", 0),
                "max_ppc": cfg.get("max_ppc", 256),
                "ws_mb": cfg.get("ws_mb", 512)}
        t0 = time.perf_counter()
        eng = HipEngine(spec=spec)
        eng.train_dev(xb)
        eng.add_dev(xb)
        eng.nprobe = args.nprobe
        n, nq = eng.ntotal, q.shape[0]
        D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        eng.search_dev(q, k, D, I)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        eng.lib.dfann_code_stride.argtypes = [ctypes.c_void_p]
        stride = int(eng.lib.dfann_code_stride(eng.h))
        out = {"config": name, "n": n, "nq": nq, "k": k, "nprobe": args.nprobe,
               "stride": stride, "build_s": round(build_s, 1), "remove": {}}
        print(f"[remove_bench] {name}: built in {build_s:.1f} s",
              file=sys.stderr, flush=True)

        # the artifacts, for the fresh index of the survivors
        cent = eng.get_centroids()
        cb = eng.get_codebooks() if cfg["type"] == "ivfpq" else None
        vmin, vdiff = (eng.get_sq_params()
                       if cfg.get("sq_type", "fp16") != "fp16"
                       and cfg["type"] == "ivfsq" else (None, None))

        tmp = tempfile.mkdtemp(prefix="remove_bench_")
        path = os.path.join(tmp, "shard.dfann")
        eng.save(path)
        del eng
        torch.cuda.empty_cache()

        gen = torch.Generator(device="cuda").manual_seed(77)
        u = torch.rand(n, generator=gen, device="cuda")
        cases = [(0.01, None), (0.10, None), (0.50, "1"), (0.50, None)]
        for frac, lanes in cases:
            e = HipProvider().load(path)
            e.nprobe = args.nprobe
            mask = u < frac
            bits = pack_bits(mask)
            nrem = int(mask.sum())
            moved = 2 * (n - nrem) * stride
            # ceiling: a plain copy of the bytes the compaction writes
            src = torch.empty((n - nrem) * stride, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            copy_ms = timed(lambda: dst.copy_(src))
            del src, dst
            torch.cuda.empty_cache()
            if lanes:
                os.environ["DFANN_REMOVE_LANES"] = lanes
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = e.remove_ids_dev(bits, n)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            os.environ.pop("DFANN_REMOVE_LANES", None)
            assert got == nrem and e.nlive == n - nrem
            leg = {"removed": nrem, "ms": round(ms, 2),
                   "moved_gb": round(moved / 1e9, 3),
                   "moved_gbps": round(moved / 1e9 / (ms / 1e3), 1),
                   "copy_ms": round(copy_ms, 3),
                   "copy_gbps": round(moved / 1e9 / (copy_ms / 1e3), 1),
                   "fraction_of_copy": round(copy_ms / ms, 3)}
            key = f"{int(frac * 100)}pct" + ("_thread_per_row" if lanes else "")
            out["remove"][key] = leg
            print(f"[remove_bench] {name} {key}: {leg}", file=sys.stderr,
                  flush=True)
            if frac == 0.50 and not lanes:
                ms_rm = timed(lambda: e.search_dev(q, k, D, I))
                I_rm = I.clone()
                fresh = HipEngine(spec=spec)
                fresh.set_trained(cent, cb, vmin, vdiff)
                keep = torch.nonzero(~mask).squeeze(1)
                CH = 1_000_000
                for s in range(0, keep.shape[0], CH):
                    fresh.add_dev(xb[keep[s:s + CH]].contiguous())
                fresh.nprobe = args.nprobe
                ms_fr = timed(lambda: fresh.search_dev(q, k, D, I))
                # same rows, same quantizer: the same answers, renumbered
                same = bool((keep[I.clamp(min=0)] == I_rm)[I >= 0].all())
                out["search_after_50pct"] = {
                    "removed_ms": round(ms_rm, 3),
                    "removed_qps": round(nq / (ms_rm / 1e3)),
                    "fresh_ms": round(ms_fr, 3),
                    "fresh_qps": round(nq / (ms_fr / 1e3)),
                    "removed_over_fresh": round(ms_rm / ms_fr, 3),
                    "same_neighbours": same}
                del fresh
            del e
            torch.cuda.empty_cache()
        os.remove(path)
        os.rmdir(tmp)
        print(json.dumps(out), flush=True)
        del xb, q
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
