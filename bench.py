#!/usr/bin/env python3
# bench.py — BASELINE.json metric on MI355X: QPS at recall@10 >= 0.95 for
# the sharded IVFPQ search path (driver contract: one JSON line from rank 0).
#
# A "step" = one pass of the hot path over one batch of synthetic queries:
# local shard search (coarse MFMA GEMM -> LDS-LUT list scan -> top-k merge)
# + RCCL all-gather of per-shard (distance,id) top-k + on-GPU k-way merge.
# Inputs are resident in HBM when the timed region starts.
#
# Default workload (N=1): "ivfpq_100m8_d768_m64" — the BASELINE.json
# configs[3] HEADLINE per-shard slice (12.5M x 768 IVFPQ m=64,
# nlist=65536/shard; at --gpus 8 the sharded DB is exactly the 100M x 768
# configuration the metric is quoted on). It builds in ~40 s and benches
# within the driver budget. "ivfpq_1m_d128_m16" (configs[2]) stays as the
# secondary regression line.
# Multi-GPU (--gpus N via torchrun): weak scaling — each rank holds its own
# shard (disjoint partitions, as the reference's per-server round-robin
# placement), value = whole-job QPS against the N-shard DB.
#
# recall@10 follows the faiss convention (recall at rank 10): the fraction
# of queries whose TRUE nearest neighbor appears in the returned top-10;
# ground truth by exact brute force on GPU. nprobe is swept to the smallest
# value reaching 0.95.
#
# A plain run does only what the headline figure needs: build, operating
# point, warm-up, the timed steps, the result line. --full adds the legs
# that take runs of their own (served-path / graph-replay agreement checks,
# scan-kernel roofline, CPU baseline); without it the result line carries
# "roofline": null and "cpu_baseline": null. --dump-outputs DIR writes the
# arrays the last timed step returned (seeded inputs: same arguments, same
# queries and shard data on every run).
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0  # gfx950 spec peak (MI355X_MICROARCH.md)


def log(msg):
    if int(os.environ.get("RANK", "0")) == 0:
        print(f"[bench] {msg}", file=sys.stderr, flush=True)


WORKLOADS = {
    # BASELINE.json configs[2] (SIFT1M-shaped IVFPQ). sigma 0.5 gives
    # SIFT-like cluster overlap so the nprobe/recall trade-off is
    # non-degenerate (sigma 0.15 was solved at nprobe=1).
    "ivfpq_1m_d128_m16": dict(
        type="ivfpq", d=128, n=1_000_000, nlist=1024, m=16, nbits=8,
        metric=1, nq=10_000, k=10, centers=10_000, sigma=0.45, latent=12,
        pq_lut_f16=1,
    ),
    # BASELINE.json configs[1] (ivf_simple 1M, dot) — parity/regression
    "ivfflat_1m_d128": dict(
        type="ivf_flat", d=128, n=1_000_000, nlist=1024, m=0, nbits=8,
        metric=0, nq=10_000, k=10, centers=10_000, sigma=0.15,
        fixed_nprobe=16,
    ),
    # BASELINE.json configs[4]-shaped at single-GPU scale (8-bit SQ,
    # HBM-stress flavor: 128 code bytes/vector)
    "ivfsq8_1m_d128": dict(
        type="ivfsq", d=128, n=1_000_000, nlist=1024, m=0, nbits=8,
        metric=1, nq=10_000, k=10, centers=10_000, sigma=0.5,
        sq_type="8bit",
    ),
    # 10M single-GPU stress (toward configs[3] scale; 160 MB codes)
    "ivfpq_10m_d128_m16": dict(
        type="ivfpq", d=128, n=10_000_000, nlist=4096, m=16, nbits=8,
        metric=1, nq=10_000, k=10, centers=200_000, sigma=0.5, latent=12,
    ),
    # true HBM-bound scan: 10M x 128B SQ8 codes = 1.28 GB >> 256 MB L3
    "ivfsq8_10m_d128": dict(
        type="ivfsq", d=128, n=10_000_000, nlist=4096, m=0, nbits=8,
        metric=1, nq=10_000, k=10, centers=50_000, sigma=0.5,
        sq_type="8bit",
    ),
    # BASELINE configs[3]-SHAPED at single-GPU-buildable scale: d=768,
    # m=64 (64 KB LUT in LDS), bf16-MFMA assign/coarse build path
    "ivfpq_2m_d768_m64": dict(
        type="ivfpq", d=768, n=2_000_000, nlist=2048, m=64, nbits=8,
        metric=1, nq=10_000, k=10, centers=20_000, sigma=0.5, latent=32,
        coarse_bf16=1, max_ppc=64,
    ),
    # THE HEADLINE: BASELINE.json configs[3] per-shard slice — 12.5M x 768
    # IVFPQ m=64, at --gpus 8 the sharded DB is exactly the 100M x 768
    # configuration. bf16-MFMA assign/coarse for the build; k-means capped
    # at 64 pts/centroid. nlist=16384/shard (engine tuning, round-2 sweep
    # gpurun_out/r2s_nl*.json: same scanned rows/query as 65536@nprobe=8
    # but 4x less coarse GEMM / top-k / ADC-table overhead — 1.34M ->
    # 3.94M QPS at recall 0.978; override with --nlist).
    "ivfpq_100m8_d768_m64": dict(
        type="ivfpq", d=768, n=12_500_000, nlist=16384, m=64, nbits=8,
        metric=1, nq=10_000, k=10, centers=12_500, sigma=0.5, latent=32,
        coarse_bf16=1, max_ppc=64, ws_mb=2048, pq_lut_f16=1,
    ),
    # BASELINE configs[4] per-shard slice: 1B x 128 SIFT1B-shaped 8-bit SQ
    # sharded over 8 GPUs = 125M/shard (the HBM-stress config: 16 GB of
    # packed codes per shard, far beyond the 256 MB LLC). Slab-arena
    # memory plan keeps peak code memory ~1x + merge_mb.
    "ivfsq8_125m_d128": dict(
        type="ivfsq", d=128, n=125_000_000, nlist=16384, m=0, nbits=8,
        metric=1, nq=10_000, k=10, centers=125_000, sigma=0.5, latent=12,
        sq_type="8bit", coarse_bf16=1, max_ppc=64, ws_mb=2048,
    ),
    # scaled-down smoke workload
    "ivfpq_100k_d64": dict(
        type="ivfpq", d=64, n=100_000, nlist=256, m=8, nbits=8,
        metric=1, nq=2_000, k=10, centers=1_000, sigma=0.15,
    ),
}


def gen_shard(cfg, rank, device):
    """Synthetic shard data + HELD-OUT queries, generated on GPU.

    SURVEY.md §8d protocol (Gaussian mixture, held-out queries) with one
    measured refinement: the configs name SIFT- / BERT-embedding-shaped
    data, whose INTRINSIC dimension is far below d — and PQ recall
    depends on exactly that (an isotropic full-rank mixture caps
    recall@10 near 0.5 for m=16 regardless of nprobe, measured; SIFT-like
    low-rank data sweeps to >0.95 like the real datasets do). So points
    live on a latent subspace of dim cfg["latent"] (16 for d=128 SIFT
    shapes, 32 for d=768 BERT shapes) plus small ambient noise:
        x = (center_z + sigma*noise_z) @ P + 0.02*ambient
    Queries are fresh mixture samples (never stored), identical across
    ranks via the shared seed.
    """
    import torch

    d, n = cfg["d"], cfg["n"]
    dl = cfg.get("latent", 16)
    gp = torch.Generator(device=device).manual_seed(4321)  # shared projection
    P = torch.randn(dl, d, generator=gp, device=device) / (dl ** 0.5)
    g = torch.Generator(device=device).manual_seed(1234 + rank)
    centers_z = torch.randn(cfg["centers"], dl, generator=g, device=device)
    lbl = torch.randint(0, cfg["centers"], (n,), generator=g, device=device)
    z = centers_z[lbl] + cfg["sigma"] * torch.randn(n, dl, generator=g,
                                                    device=device)
    xb = z @ P + 0.02 * torch.randn(n, d, generator=g, device=device)
    gq = torch.Generator(device=device).manual_seed(9999)  # same on all ranks
    qlbl = torch.randint(0, cfg["centers"], (cfg["nq"],), generator=gq,
                         device=device)
    qz = centers_z[qlbl] + cfg["sigma"] * torch.randn(
        cfg["nq"], dl, generator=gq, device=device)
    q = qz @ P + 0.02 * torch.randn(cfg["nq"], d, generator=gq, device=device)
    return xb.float().contiguous(), q.float().contiguous()


def exact_ground_truth(xb, q, metric, k, device):
    """Exact top-k of the LOCAL shard by brute force (chunked GPU GEMM)."""
    import torch

    n = xb.shape[0]
    nq = q.shape[0]
    Dbest = torch.full((nq, k), float("inf"), device=device)
    Ibest = torch.full((nq, k), -1, dtype=torch.int64, device=device)
    xn = (xb * xb).sum(1)
    CH = 250_000
    for b0 in range(0, n, CH):
        blk = xb[b0:b0 + CH]
        ip = q @ blk.T
        sc = xn[b0:b0 + CH][None, :] - 2.0 * ip if metric == 1 else -ip
        d2, i2 = torch.topk(sc, min(k, sc.shape[1]), dim=1, largest=False)
        Dcat = torch.cat([Dbest, d2], dim=1)
        Icat = torch.cat([Ibest, i2 + b0], dim=1)
        Dbest, sel = torch.topk(Dcat, k, dim=1, largest=False)
        Ibest = torch.gather(Icat, 1, sel)
    return Dbest, Ibest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="ivfpq_100m8_d768_m64",
                    choices=sorted(WORKLOADS))
    ap.add_argument("--target-recall", type=float, default=0.95)
    ap.add_argument("--full", action="store_true",
                    help="also run the legs the headline figure does not "
                         "need: served-path and graph-replay agreement "
                         "checks, scan-kernel roofline, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last timed "
                         "step returned as DIR/distances.npy (float32) and "
                         "DIR/ids.npy (float64 global ids)")
    ap.add_argument("--cpu-baseline", type=int, default=1,
                    help="with --full: 0 skips the CPU-baseline leg")
    ap.add_argument("--cpu-sample-queries", type=int, default=256)
    ap.add_argument("--pq-precomputed", type=int, default=-1,
                    help="-1: workload default; 0/1 override")
    ap.add_argument("--pq-lut-global", type=int, default=-1,
                    help="-1: auto (on at m>=32); 0/1 override")
    ap.add_argument("--pq-lut-mb", type=int, default=2048,
                    help="LUT chunk budget (bigger chunks win)")
    ap.add_argument("--pq-lut-f16", type=int, default=-1,
                    help="-1: workload default; 0/1 override")
    ap.add_argument("--graph", type=int, default=1,
                    help="HIP-graph the serving step at N=1 (0: eager)")
    ap.add_argument("--nlist", type=int, default=0,
                    help="override the workload's nlist (0: default); the "
                         "BASELINE configs fix N/d/m — nlist is engine "
                         "tuning (printed in config.nlist)")
    args = ap.parse_args()

    import torch

    from distributed_faiss_amd.client import IndexClient
    from distributed_faiss_amd.dist import (
        allgather_shard_topk,
        init_from_env,
        merge_gathered,
    )
    from distributed_faiss_amd.hip_engine import HipEngine, HipProvider
    from distributed_faiss_amd.index import Index
    from distributed_faiss_amd.index_cfg import IndexCfg
    from distributed_faiss_amd.index_state import IndexState
    from distributed_faiss_amd.server import IndexServer

    rank, world = init_from_env()
    assert world == args.gpus or world == 1, (world, args.gpus)
    device = "cuda"
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    cfg = dict(WORKLOADS[args.config])
    if args.nlist:
        cfg["nlist"] = args.nlist
    metric = cfg["metric"]
    maximize = metric == 0
    k = cfg["k"]

    # ---- build phase (untimed) ----
    t0 = time.time()
    xb, q = gen_shard(cfg, rank, device)
    # NB queries are seeded identically on every rank (gen_shard), but the
    # CENTERS differ per rank (each shard its own mixture) — queries come
    # from rank 0's centers, so broadcast to keep them truly identical
    if world > 1:
        import torch.distributed as dist

        dist.broadcast(q, src=0)
    log(f"data generated in {time.time()-t0:.1f}s")

    spec = {"type": cfg["type"], "dim": cfg["d"], "metric": metric,
            "nlist": cfg["nlist"], "m": cfg["m"], "nbits": cfg["nbits"],
            "sq_type": cfg.get("sq_type", "fp16"), "nprobe": 1, "seed": 1234,
            "coarse_bf16": cfg.get("coarse_bf16", 0),
            "max_ppc": cfg.get("max_ppc", 256),
            "ws_mb": cfg.get("ws_mb", 512),
            "pq_precomputed": (cfg.get("pq_precomputed", 0)
                               if args.pq_precomputed < 0
                               else args.pq_precomputed),
            "pq_lut_global": args.pq_lut_global,
            "pq_lut_mb": args.pq_lut_mb,
            "pq_lut_f16": (cfg.get("pq_lut_f16", 0)
                           if args.pq_lut_f16 < 0 else args.pq_lut_f16)}
    eng = HipEngine(spec=spec)
    t0 = time.time()
    eng.train_dev(xb)
    log(f"trained in {time.time()-t0:.1f}s")
    t0 = time.time()
    eng.add_dev(xb)
    torch.cuda.synchronize()
    free_b, total_b = torch.cuda.mem_get_info()
    log(f"added {eng.ntotal} in {time.time()-t0:.1f}s "
        f"(HBM in use {(total_b-free_b)/2**30:.1f} GiB of {total_b/2**30:.0f})")

    # ---- serve through the reference surface (IndexClient) ----
    # The timed step routes through IndexClient.search_dev — the SAME
    # pipeline IndexClient.search uses in distributed mode (local shard
    # search -> RCCL all-gather -> on-GPU k-way merge), minus the host
    # metadata epilogue. The shard engine was built above from
    # device-resident synthetic data (the Index.add_batch path would
    # bounce the 38 GB shard through host numpy), then adopted into the
    # server, exactly what Index.from_storage_dir does on load.
    class _NoMeta:  # bench shards carry no metadata; every id maps to None
        def __getitem__(self, i):
            return None

        def __len__(self):
            return 1 << 62

    icfg = IndexCfg(faiss_factory="Flat", dim=cfg["d"],
                    metric=("l2" if metric == 1 else "dot"), nprobe=1)
    shard_index = Index(icfg, provider=HipProvider())
    shard_index.engine = eng
    shard_index.state = IndexState.TRAINED
    shard_index.id_to_metadata = _NoMeta()
    server = IndexServer(rank, os.path.join("/tmp", "dfann_bench"))
    server.adopt_index("bench", shard_index)
    client = IndexClient(servers=[server])
    client.cfg = icfg
    assert client.dist_mode == (world > 1)

    # ---- ground truth + nprobe operating point ----
    t0 = time.time()
    Dgt, Igt = exact_ground_truth(xb, q, metric, k, device)
    Dall, Iall = allgather_shard_topk(Dgt, Igt)
    _, s_idx, local = merge_gathered(Dall, Iall, k, maximize=False)
    gt_global = s_idx * cfg["n"] + local  # (nq, k) true top-k global ids
    log(f"ground truth in {time.time()-t0:.1f}s")

    def run_search(nprobe, qt):
        # serving step THROUGH the client surface: results stay in HBM
        # (no per-step D2H sync; IndexClient.search wraps this same
        # pipeline and adds the host metadata epilogue)
        eng.nprobe = nprobe
        Dm, s_i, loc = client.search_dev(qt, k, "bench")
        return Dm, s_i * cfg["n"] + loc

    def recall_at(nprobe, nq_eval=2048):
        qt = q[:nq_eval].contiguous()
        _, got = run_search(nprobe, qt)
        # faiss convention: true NN within returned top-k
        got = got.cpu().numpy()
        hits = (got == gt_global[:nq_eval, :1]).any(axis=1)
        return float(hits.mean())

    if "fixed_nprobe" in cfg:
        nprobe, recall = cfg["fixed_nprobe"], recall_at(cfg["fixed_nprobe"])
    else:
        nprobe, recall = None, 0.0
        for cand in (1, 2, 4, 8, 16, 32, 64, 128):
            if cand > cfg["nlist"]:
                break
            r = recall_at(cand)
            log(f"nprobe={cand}: recall@{k}={r:.4f}")
            if r >= args.target_recall:
                nprobe, recall = cand, r
                break
            nprobe, recall = cand, r
    eng.nprobe = nprobe
    log(f"operating point: nprobe={nprobe} recall={recall:.4f}")

    # --full: one untimed pass through the FULL reference API (host arrays
    # + metadata epilogue) to prove the served path and the timed path
    # agree — client.search wraps the same pipeline as search_dev
    if args.full:
        q4 = q[:4].cpu().numpy()
        Dh, _meta_h = (client.search(q4, k, "bench")[:2])
        Dd, _gid = run_search(nprobe, q[:4].contiguous())
        # both carry the reference merge conventions (incl. quirk-2 negation)
        assert np.allclose(np.asarray(Dh), Dd.cpu().numpy(),
                           rtol=1e-6, atol=1e-6), \
            "client.search diverged from the device serving step"

    # ---- timed region ----
    import torch.distributed as tdist

    def barrier():
        if world > 1:
            tdist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        run_search(nprobe, q)
    # Serving-style step: capture the whole search step (coarse -> scan ->
    # merge) in a HIP graph and replay it — identical kernels and work,
    # zero host launch gaps (the 1M step is otherwise launch-bound).
    # Verified under --full: one replay must reproduce the eager step
    # bitwise. Multi-rank keeps the eager path (RCCL collectives stay
    # outside graphs), so SCALE numbers are conservative.
    use_graph = world == 1 and args.graph
    if use_graph:
        try:
            # one eager step right before capture, so no lazy allocation
            # or first-use setup lands inside the captured region
            Dref, gref = run_search(nprobe, q)
            gobj = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gobj):
                Dcap, gcap = run_search(nprobe, q)
            gobj.replay()  # first replay uploads the graph: keep it untimed
            torch.cuda.synchronize()
            if args.full:
                assert torch.equal(gcap, gref) and torch.equal(Dcap, Dref), \
                    "graph replay diverged from eager step"
            del Dref, gref
        except Exception as e:  # never let capture kill the bench
            log(f"graph capture unavailable ({e}); eager steps")
            use_graph = False
    last = [None]  # what the most recent timed step returned (D, global ids)
    if use_graph:
        last[0] = (Dcap, gcap)  # static graph outputs, rewritten per replay

        def step():
            gobj.replay()
    else:
        def step():
            last[0] = run_search(nprobe, q)
    barrier()
    t0 = time.time()
    for _ in range(args.steps):
        step()
    barrier()
    elapsed = time.time() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=device)
        tdist.all_reduce(t, op=tdist.ReduceOp.MAX)
        elapsed = float(t.item())
    ms_per_step = elapsed * 1000.0 / args.steps
    qps = cfg["nq"] * args.steps / elapsed

    # ---- --dump-outputs: what the last timed step handed its caller ----
    # (merged distances + global ids of the whole query batch: nq x k each,
    # far below any size worth sampling). ids go out as float64, exact for
    # every id below 2^53.
    if args.dump_outputs and rank == 0 and last[0] is not None:
        os.makedirs(args.dump_outputs, exist_ok=True)
        D_last, gid_last = last[0]
        np.save(os.path.join(args.dump_outputs, "distances.npy"),
                D_last.detach().cpu().numpy().astype(np.float32))
        np.save(os.path.join(args.dump_outputs, "ids.npy"),
                gid_last.detach().cpu().numpy().astype(np.float64))
        log(f"outputs of the last timed step written to {args.dump_outputs}")

    roofline = None
    cpu_baseline = None
    if args.full:
        roofline = roofline_leg(args, cfg, eng, nprobe,
                                lambda: run_search(nprobe, q))
        cpu_baseline = cpu_baseline_leg(args, cfg, spec, eng, nprobe, q, k,
                                        rank, world)

    if rank == 0:
        out = {
            "metric": "QPS at recall@10>=0.95 (IVFPQ sharded search)",
            "value": qps,
            "unit": "queries/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": args.config,
                "n_per_shard": cfg["n"],
                "dim": cfg["d"],
                "nlist": cfg["nlist"],
                "m": cfg["m"],
                "k": k,
                "nprobe": nprobe,
                "recall_at_10": recall,
                "batch": cfg["nq"],
                "metric_space": "l2" if metric == 1 else "dot",
                "coarse_dtype": "bf16" if cfg.get("coarse_bf16") else "f32",
                "pq_lut": ("f16" if (cfg.get("pq_lut_f16", 0)
                                     if args.pq_lut_f16 < 0
                                     else args.pq_lut_f16)
                           else "f32"),
                "step_graph": bool(use_graph),
                "serving_path": "IndexClient.search_dev",
            },
            # both legs run under --full only (null on a plain run)
            "roofline": roofline,
            "cpu_baseline": cpu_baseline,
        }
        print(json.dumps(out), flush=True)


def roofline_leg(args, cfg, eng, nprobe, search_step):
    """--full: scan-kernel HIP-event timing on the same workload."""
    import torch

    eng.set_timing(True)
    eng.get_timing()  # reset
    for _ in range(3):
        search_step()
    torch.cuda.synchronize()
    t = eng.get_timing()
    eng.set_timing(False)
    # algorithmic bytes: packed code bytes per scanned row (stride ==
    # code_bytes for m=16 / d%16==0; ids are read only for winners)
    scan_gbs = (t["scan_bytes"] / 1e9) / (t["scan_ms"] / 1e3) if t["scan_ms"] else 0.0
    per_launch_bytes = t["scan_bytes"] / max(t["scan_launches"], 1)
    per_launch_ms = t["scan_ms"] / max(t["scan_launches"], 1)
    # honesty about the cache level that actually bounds the scan: if the
    # whole code arena fits the 256 MiB Infinity Cache, re-reads are
    # absorbed on-die and the 8 TB/s HBM peak is not the binding roof
    # (MI355X_MICROARCH.md §Infinity Cache)
    code_bytes = {"ivfpq": cfg["m"], "ivfsq": cfg["d"],
                  "ivf_flat": 4 * cfg["d"]}[cfg["type"]]
    codes_total = eng.ntotal * ((code_bytes + 15) // 16 * 16)
    hbm_bound = codes_total > 256 * 1024 * 1024
    # measured HBM traffic (rocprofv3 --pmc FETCH_SIZE/WRITE_SIZE, with the
    # gfx950 x2 wide-read correction — MI355X_MICROARCH.md §HBM): PMC
    # cannot run inside this bench process, so the per-launch counter
    # bytes are read from the committed calibration measured on the SAME
    # workload at the SAME operating point (profiles/traffic_calibration.
    # json, generating rocprofv3 runs cited inside). Entries whose
    # operating point (nprobe / lut mode) differs from this run's are
    # skipped -> traffic stays null.
    traffic = None
    traffic_src = None
    cal_path = os.path.join(REPO, "profiles", "traffic_calibration.json")
    lut_mode = ("f16" if (cfg.get("pq_lut_f16", 0) if args.pq_lut_f16 < 0
                          else args.pq_lut_f16) else "f32")
    if os.path.exists(cal_path):
        try:
            cal = json.load(open(cal_path)).get(args.config)
            if (cal and cal.get("nprobe") == nprobe
                    and cal.get("lut") in (None, lut_mode)):
                traffic = cal["bytes_per_launch"]
                traffic_src = cal.get("source")
        except Exception as e:
            log(f"traffic calibration unreadable: {e}")
    roofline = {
        "bound": "hbm" if hbm_bound else "l3-resident (codes fit 256MiB LLC)",
        "achieved": scan_gbs,
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": scan_gbs / HBM_PEAK_GBS,
        "traffic": traffic,  # measured counter bytes/launch (see above)
        "traffic_source": traffic_src,
        "kernel": {"ivfpq": "k_scan_pq", "ivfsq": "k_scan_sq8",
                   "ivf_flat": "k_scan_ivfflat"}[cfg["type"]],
        "per_launch_bytes": per_launch_bytes,
        "per_launch_ms": per_launch_ms,
        # per-3-search phase split (ms): ADC-table build is timed apart
        # from the scan proper, so `achieved` is the scan kernel alone
        "lut_ms": t["lut_ms"],
        "gemm_ms": t["gemm_ms"],
        "merge_ms": t["merge_ms"],
        "scan_ms": t["scan_ms"],
        "gemm_ms_frac": t["gemm_ms"] / max(t["scan_ms"] + t["gemm_ms"]
                                           + t["merge_ms"] + t["lut_ms"],
                                           1e-9),
    }
    return roofline


def cpu_baseline_leg(args, cfg, spec, eng, nprobe, q, k, rank, world):
    """--full: the CPU oracle scanning the engine's own lists (None when
    the leg does not apply or --cpu-baseline 0)."""
    # ---- CPU baseline (rank 0, N=1): oracle scanning the SAME index ----
    cpu_baseline = None
    if rank == 0 and world == 1 and args.cpu_baseline:
        sys.path.insert(0, REPO)
        from oracle import make_oracle_engine

        t0 = time.time()
        orc = make_oracle_engine(spec)
        orc.centroids = eng.get_centroids()
        if cfg["type"] == "ivfpq":
            orc.codebooks = eng.get_codebooks()
        if cfg["type"] == "ivfsq" and cfg.get("sq_type") == "8bit":
            vmin, vdiff = eng.get_sq_params()
            orc.vmin, orc.vdiff = vmin, vdiff
            orc.scale = (vdiff / np.float32(255.0)).astype(np.float32)
        orc.is_trained = True
        off, ids, codes = eng.get_lists()
        for L in range(cfg["nlist"]):
            s0, s1 = int(off[L]), int(off[L + 1])
            orc.list_ids[L] = ids[s0:s1]
            if cfg["type"] == "ivfpq":
                orc.list_codes[L] = codes[s0:s1, :cfg["m"]]
            elif cfg["type"] == "ivfsq":
                nb = cfg["d"] if cfg.get("sq_type") == "8bit" else 2 * cfg["d"]
                orc.list_codes[L] = codes[s0:s1, :nb]
            else:
                orc.list_data[L] = (
                    codes[s0:s1].reshape(s1 - s0, -1)[:, :cfg["d"] * 4]
                    .copy().view(np.float32))
        orc.ntotal = eng.ntotal
        orc.nprobe = nprobe
        log(f"cpu baseline index shared in {time.time()-t0:.1f}s")
        # bounded sample: repeat query slices until >= ~10 s of CPU work
        nq_s = args.cpu_sample_queries
        q_np = q[:nq_s].cpu().numpy()
        done = 0
        t0 = time.time()
        while True:
            orc.search(q_np, k)
            done += nq_s
            cpu_elapsed = time.time() - t0
            if cpu_elapsed >= 10.0 or done >= cfg["nq"]:
                break
        cpu_baseline = {
            "value": done / cpu_elapsed,
            "unit": "QPS",
            # numpy fancy-indexing scan is single-threaded; the BLAS coarse
            # GEMM uses all cores but is a small fraction of oracle time
            "cores": 1,
            "kind": "port",
            "sample": f"{done} queries ({nq_s}-query batches of the same "
                      f"workload batch), same index content (engine lists), "
                      f"{cpu_elapsed:.1f}s on host cores "
                      f"(os.cpu_count={os.cpu_count()})",
        }
    return cpu_baseline


if __name__ == "__main__":
    main()
