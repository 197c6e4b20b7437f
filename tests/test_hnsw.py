# hnswsq engine (reference index.py:51-60 builder): GPU build + search.
#
# Parity tiers:
#  * search: BIT-EXACT vs the oracle restatement over the engine's own
#    dumped graph (OracleHNSWSearch mirrors k_hnsw_search op-for-op).
#  * build: deterministic (same data + seed -> identical graph dump) and
#    recall-gated here (the batched wave insertion is a documented
#    deviation from faiss's sequential insertion); the graph itself is
#    pinned bit for bit against the oracle's build restatement in
#    tests/test_gpu_hnsw_build.py.
#  * persistence: save/load -> identical graph + results.
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from distributed_faiss_amd.hip_engine import HipEngine, HipProvider  # noqa: E402
from oracle.core import OracleHNSWSearch  # noqa: E402


def _clustered(n, d, seed=0, centers=64, sigma=0.3):
    # centers SHARED across calls (queries must come from the same
    # mixture as the database, as the bench's gen_shard does)
    crng = np.random.default_rng(1000)
    cent = crng.standard_normal((centers, d)).astype(np.float32) * 3.0
    rng = np.random.default_rng(seed)
    lbl = rng.integers(0, centers, n)
    x = cent[lbl] + sigma * rng.standard_normal((n, d)).astype(np.float32)
    return x.astype(np.float32)


def _build(n=4000, d=32, m=16, efc=60, seed=7, chunks=1):
    xb = _clustered(n, d, seed=seed)
    spec = {"type": "hnswsq", "dim": d, "metric": 1, "m": m,
            "ef_construction": efc, "nprobe": 32, "seed": 11}
    eng = HipEngine(spec=spec)
    eng.train(xb[: max(1000, n // 4)])
    ch = (n + chunks - 1) // chunks
    for s in range(0, n, ch):
        eng.add(xb[s:s + ch])
    return eng, xb


def test_hnsw_build_deterministic():
    e1, xb = _build()
    e2, _ = _build()
    d1, d2 = e1.hnsw_dump(), e2.hnsw_dump()
    for k in ("levels", "cnt0", "nbr0", "upslot", "cntU", "nbrU"):
        np.testing.assert_array_equal(d1[k], d2[k])
    assert d1["entry"] == d2["entry"] and d1["maxlevel"] == d2["maxlevel"]
    q = _clustered(50, 32, seed=99)
    D1, I1 = e1.search(q, 10)
    D2, I2 = e2.search(q, 10)
    np.testing.assert_array_equal(I1, I2)
    np.testing.assert_array_equal(D1, D2)


def test_hnsw_search_matches_oracle_on_shared_graph():
    eng, xb = _build(n=3000, d=32, m=16, efc=50)
    g = eng.hnsw_dump()
    vmin, vdiff = eng.get_sq_params()
    codes = OracleHNSWSearch.encode(xb, vmin, vdiff)
    orc = OracleHNSWSearch(32, g, vmin, vdiff, codes)
    q = _clustered(12, 32, seed=5)
    for ef in (10, 40):
        eng.nprobe = ef
        D, I = eng.search(q, 10)
        Do, Io = orc.search(q, 10, ef)
        np.testing.assert_array_equal(I, Io)
        np.testing.assert_array_equal(D, Do)  # bitwise


def test_hnsw_recall_property():
    # graph quality gate on clustered data: recall@10 of the SQ8-decoded
    # ground truth (the codec's own nearest neighbors) at ef=64
    n, d = 50_000, 64
    eng, xb = _build(n=n, d=d, m=32, efc=100, chunks=3)
    vmin, vdiff = eng.get_sq_params()
    codes = OracleHNSWSearch.encode(xb, vmin, vdiff)
    scale = vdiff.astype(np.float32) / np.float32(255.0)
    dec = (vmin[None, :] + (codes.astype(np.float32) + 0.5) * scale[None, :])
    q = _clustered(200, d, seed=42)
    # decoded-space GT (what the HNSW distance actually minimizes)
    dec_t = torch.as_tensor(dec).cuda()
    q_t = torch.as_tensor(q).cuda()
    d2 = (torch.cdist(q_t, dec_t) ** 2)
    gt = torch.topk(d2, 10, largest=False).indices.cpu().numpy()
    eng.nprobe = 64
    D, I = eng.search(q, 10)
    hits = np.mean([len(set(I[i]) & set(gt[i])) / 10.0 for i in range(len(q))])
    assert hits >= 0.85, f"recall@10 {hits}"
    # results are sorted and valid
    assert (np.diff(D, axis=1) >= 0).all()
    assert (I >= 0).all() and (I < n).all()


def test_hnsw_persistence_roundtrip(tmp_path):
    eng, xb = _build(n=2500, d=32, m=16)
    p = str(tmp_path / "h.dfann")
    eng.save(p)
    prov = HipProvider()
    e2 = prov.load(p)
    d1, d2 = eng.hnsw_dump(), e2.hnsw_dump()
    for k in ("levels", "cnt0", "nbr0", "cntU", "nbrU"):
        np.testing.assert_array_equal(d1[k], d2[k])
    q = _clustered(20, 32, seed=3)
    e2.nprobe = 32
    D1, I1 = eng.search(q, 5)
    D2, I2 = e2.search(q, 5)
    np.testing.assert_array_equal(I1, I2)
    np.testing.assert_array_equal(D1, D2)


def test_hnsw_reconstruct_and_builder_flow(tmp_path):
    # through the reference surface: builder "hnswsq" via Index/Client
    from distributed_faiss_amd import IndexCfg, IndexClient, IndexServer

    prov = HipProvider()
    srv = IndexServer(0, str(tmp_path), provider=prov)
    cli = IndexClient(servers=[srv])
    cfg = IndexCfg(index_builder_type="hnswsq", dim=32, metric="l2",
                   train_num=500, nprobe=40, store_n=16, ef_construction=50)
    cli.create_index("h", cfg)
    cli.cfg = cfg
    xb = _clustered(2000, 32, seed=1)
    cli.add_index_data("h", xb, [("m", i) for i in range(2000)],
                       train_async_if_triggered=False)
    import time

    from distributed_faiss_amd import IndexState

    for _ in range(200):
        if (cli.get_state("h") == IndexState.TRAINED
                and cli.get_ntotal("h") == 2000):
            break
        time.sleep(0.05)
    q = _clustered(6, 32, seed=2)
    D, meta = cli.search(q, 5, "h")
    assert D.shape == (6, 5)
    assert all(m[0][0] == "m" for m in meta)
    # search_and_reconstruct decodes SQ8 rows (no centroid term)
    eng = srv._get_index("h").engine
    Dr, Ir, R = eng.search_and_reconstruct(q, 3)
    vmin, vdiff = eng.get_sq_params()
    codes = OracleHNSWSearch.encode(xb, vmin, vdiff)
    scale = vdiff.astype(np.float32) / np.float32(255.0)
    for i in range(3):
        for j in range(3):
            rid = Ir[i, j]
            dec = vmin + (codes[rid].astype(np.float32) + 0.5) * scale
            np.testing.assert_allclose(R[i, j], dec, rtol=1e-6, atol=1e-6)
