# Exact filtered search, the layers above the engine (no GPU): Index bitmap
# construction and caching, server / client plumbing, dist-mode fan-out and
# the TCP transport. The engine is the CPU oracle wrapped by a test-local
# provider whose search_filtered is DEFINED as: oracle search at k = ntotal,
# masked to the allowed ids, truncated / padded to k.
import os
import sys
import time

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from distributed_faiss_amd import (  # noqa: E402
    IndexCfg,
    IndexClient,
    IndexServer,
    IndexState,
)
from distributed_faiss_amd.index import Index  # noqa: E402
from oracle import OracleProvider  # noqa: E402

FLT_MAX = np.float32(3.4028235e38)


class FilteredOracleEngine:
    """Oracle engine + search_filtered(q, k, allow). Counts its calls."""

    def __init__(self, inner):
        self.__dict__["inner"] = inner
        self.__dict__["filtered_calls"] = []

    def __getattr__(self, name):
        return getattr(self.__dict__["inner"], name)

    def __setattr__(self, name, value):
        setattr(self.__dict__["inner"], name, value)

    def search_filtered(self, q, k, allow):
        inner = self.inner
        allow = np.asarray(allow, dtype=bool)
        assert allow.shape[0] >= inner.ntotal
        self.filtered_calls.append(allow.copy())
        nq = q.shape[0]
        pad = FLT_MAX if inner.metric == 1 else -FLT_MAX
        D = np.full((nq, k), pad, np.float32)
        I = np.full((nq, k), -1, np.int64)
        if inner.ntotal == 0:
            return D, I
        Df, If = inner.search(q, inner.ntotal)
        for i in range(nq):
            valid = If[i] >= 0
            keep = np.zeros(If.shape[1], bool)
            keep[valid] = allow[If[i][valid]]
            n = min(k, int(keep.sum()))
            D[i, :n] = Df[i][keep][:n]
            I[i, :n] = If[i][keep][:n]
        return D, I


class FilteredOracleProvider:
    def __init__(self):
        self.inner = OracleProvider()

    def create(self, spec):
        return FilteredOracleEngine(self.inner.create(spec))

    def load(self, path):
        return FilteredOracleEngine(self.inner.load(path))


def _ref_allows(m, pos, val):
    # the reference predicate, spelled as client._do_filter spells it
    if not m:
        return False
    return len(m) > pos and m[pos] != val


def _wait(pred, timeout=30):
    t0 = time.time()
    while time.time() - t0 < timeout:
        if pred():
            return True
        time.sleep(0.02)
    return False


def _flat_index(tmp_path, metas, d=8, metric="l2", seed=0, provider=None):
    n = len(metas)
    xb = np.random.default_rng(seed).standard_normal((n, d), dtype=np.float32)
    cfg = IndexCfg(faiss_factory="Flat", dim=d, metric=metric, train_num=1,
                   index_storage_dir=str(tmp_path))
    idx = Index(cfg, provider=provider or FilteredOracleProvider())
    idx.add_batch(xb, metas, train_async_if_triggered=False)
    assert _wait(lambda: idx.get_state() == IndexState.TRAINED
                 and idx.engine.ntotal == n)
    return idx, xb


# ---------------------------------------------------------------------------
# Index: bitmap construction, cache
# ---------------------------------------------------------------------------

ODD_METAS = [("a", 1), None, ("a",), (), ("b", 2), ["a", 2], "x", ("a", 2, 3),
             ("c", None), 0, ("a", [1])]


@pytest.mark.parametrize("pos,val", [(1, 2), (0, "a"), (1, None), (1, [1]),
                                     (2, 3), (5, "zz")])
def test_bitmap_matches_reference_predicate(tmp_path, pos, val):
    metas = ODD_METAS * 3
    idx, xb = _flat_index(tmp_path, metas)
    n = len(metas)
    scores, ids, meta, embs = idx.search_filtered(xb[:4], n, pos, val)
    assert embs is None
    assert scores.shape == (4, n) and ids.shape == (4, n)
    want = np.array([_ref_allows(m, pos, val) for m in metas])
    (allow,) = idx.engine.filtered_calls
    np.testing.assert_array_equal(allow[:n], want)
    # k = ntotal on a flat index: exactly the allowed ids come back
    for i in range(4):
        got = ids[i][ids[i] >= 0]
        assert sorted(got.tolist()) == np.nonzero(want)[0].tolist()
        assert (ids[i][len(got):] == -1).all()
        assert meta[i][:len(got)] == [metas[j] for j in got]
        assert all(m is None for m in meta[i][len(got):])
    # an unhashable filter value works but is not cached
    hashable = not isinstance(val, list)
    assert len(idx._filter_cache) == (1 if hashable else 0)


class _CountingMeta(tuple):
    """Metadata row that counts predicate evaluations (len() calls)."""
    calls = 0

    def __len__(self):
        type(self).calls += 1
        return super().__len__()


def test_cache_lru_and_tail_extension(tmp_path):
    _CountingMeta.calls = 0
    metas = [_CountingMeta(("doc", i % 4)) for i in range(40)]
    idx, xb = _flat_index(tmp_path, metas)
    base = _CountingMeta.calls  # bool(m) during add_batch etc.
    idx.search_filtered(xb[:2], 3, 1, 2)
    first = _CountingMeta.calls - base
    assert first >= 40  # O(ntotal) on first use
    idx.search_filtered(xb[:2], 3, 1, 2)
    assert _CountingMeta.calls - base == first  # cached: nothing re-evaluated
    # grow: only the tail is evaluated, and the mask is extended
    more = [_CountingMeta(("doc", i % 4)) for i in range(40, 50)]
    xb2 = np.random.default_rng(5).standard_normal((10, 8), dtype=np.float32)
    idx.add_batch(xb2, more)
    assert _wait(lambda: idx.get_state() == IndexState.TRAINED
                 and idx.engine.ntotal == 50)
    mid = _CountingMeta.calls
    idx.search_filtered(xb[:2], 3, 1, 2)
    per_row = first // 40
    assert _CountingMeta.calls - mid == 10 * per_row
    allow = idx.engine.filtered_calls[-1]
    np.testing.assert_array_equal(
        allow[:50], np.array([i % 4 != 2 for i in range(50)]))
    # LRU of FILTER_CACHE_SIZE entries, most recently used kept
    assert Index.FILTER_CACHE_SIZE == 8
    for v in range(100, 107):
        idx.search_filtered(xb[:1], 1, 1, v)
    assert len(idx._filter_cache) == 8 and (1, 2) in idx._filter_cache
    idx.search_filtered(xb[:1], 1, 1, 2)      # touch (1, 2)
    idx.search_filtered(xb[:1], 1, 1, 999)    # evicts the oldest: (1, 100)
    assert len(idx._filter_cache) == 8
    assert (1, 2) in idx._filter_cache and (1, 100) not in idx._filter_cache


def test_drop_index_clears_cache(tmp_path):
    idx, xb = _flat_index(tmp_path, [("doc", i % 4) for i in range(20)])
    idx.search_filtered(xb[:1], 2, 1, 2)
    assert len(idx._filter_cache) == 1
    idx.drop_index()
    assert len(idx._filter_cache) == 0


def test_engine_without_search_filtered_raises(tmp_path):
    idx, xb = _flat_index(tmp_path, [("doc", i) for i in range(10)],
                          provider=OracleProvider())
    with pytest.raises(NotImplementedError, match="search_filtered"):
        idx.search_filtered(xb[:1], 2, 1, 2)


# ---------------------------------------------------------------------------
# client: four in-process servers vs brute-force filtering of one server
# ---------------------------------------------------------------------------


def _fill(client, servers, index_id, cfg_kwargs, batches, metas):
    client.create_index(index_id, IndexCfg(**cfg_kwargs))
    client.cur_server_ids[index_id] = 0
    for b, m in zip(batches, metas):
        client.add_index_data(index_id, b, m, train_async_if_triggered=False)
    total = sum(b.shape[0] for b in batches)
    assert _wait(lambda: all(s.get_state(index_id) == IndexState.TRAINED
                             for s in servers)
                 and sum(s.get_ntotal(index_id) for s in servers) == total)


def _data(d=16, nb=12, per=25, seed=7):
    rng = np.random.default_rng(seed)
    batches = [rng.standard_normal((per, d), dtype=np.float32)
               for _ in range(nb)]
    # unique rows; field 1 cycles 0..3 (filter value 2 rejects 25 %),
    # field 3 is "common" on 75 % of the rows
    metas = [[("b%d" % bi, i % 4, bi * per + i,
               "common" if i % 4 else "rare") for i in range(per)]
             for bi in range(nb)]
    q = np.random.default_rng(99).standard_normal((9, d), dtype=np.float32)
    return batches, metas, q


def _cfg(metric):
    if metric == "dot":
        return dict(index_builder_type="flat", dim=16, train_num=10,
                    metric="dot")
    return dict(faiss_factory="Flat", dim=16, train_num=10, metric="l2")


def _brute_force(tmp_path, metric, batches, metas, q, top_k, pos, val):
    """Single server, plain search at k = ntotal, filtered on the host."""
    srv = IndexServer(0, str(tmp_path / "single"), provider=OracleProvider())
    cli = IndexClient(servers=[srv], distributed=False)
    _fill(cli, [srv], "one", _cfg(metric), batches, metas)
    n = sum(b.shape[0] for b in batches)
    D, M = cli.search(q, n, "one")
    outD = np.zeros((q.shape[0], top_k), np.float32)
    outM = []
    for i in range(q.shape[0]):
        keep = [j for j, m in enumerate(M[i]) if _ref_allows(m, pos, val)]
        assert len(keep) >= top_k
        outD[i] = D[i][keep[:top_k]]
        outM.append([M[i][j] for j in keep[:top_k]])
    return outD, outM


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_client_four_servers_equals_brute_force(tmp_path, metric):
    batches, metas, q = _data()
    prov = FilteredOracleProvider()
    servers = [IndexServer(r, str(tmp_path / "four"), provider=prov)
               for r in range(4)]
    cli = IndexClient(servers=servers, distributed=False)
    _fill(cli, servers, "idx", _cfg(metric), batches, metas)
    top_k = 7
    D, M = cli.search_filtered(q, top_k, "idx", 1, 2)
    assert D.shape == (9, top_k)
    Dr, Mr = _brute_force(tmp_path, metric, batches, metas, q, top_k, 1, 2)
    np.testing.assert_array_equal(D, Dr)
    assert M == Mr
    if metric == "dot":
        # the merged dot scores come back negated, exactly like search()
        Ds, _ = cli.search(q, top_k, "idx")
        assert (Ds <= D).all() and (D != 0).all()
        xb = np.concatenate(batches)
        row = M[0][0][2]
        np.testing.assert_allclose(D[0, 0], -float(q[0] @ xb[row]),
                                   rtol=1e-4, atol=1e-4)


def test_selective_filter_fills_top_k_where_overfetch_does_not(tmp_path):
    # 75 % of the rows rejected: the x3 over-fetch cannot fill top_k, the
    # exact path does — the gap this feature closes
    batches, metas, q = _data()
    prov = FilteredOracleProvider()
    servers = [IndexServer(r, str(tmp_path / "sel"), provider=prov)
               for r in range(4)]
    cli = IndexClient(servers=servers, distributed=False)
    _fill(cli, servers, "idx", _cfg("l2"), batches, metas)
    top_k = 20
    _s, old = cli.search_with_filter(q, top_k, "idx", 3, "common")
    assert any(len(r) < top_k for r in old), "over-fetch happened to fill"
    assert sum(len(r) for r in old) < q.shape[0] * top_k
    D, M = cli.search_filtered(q, top_k, "idx", 3, "common")
    assert D.shape == (9, top_k)
    for r in M:
        assert len(r) == top_k
        for m in r:
            assert m is not None and m[3] == "rare"
    assert (np.abs(D) < FLT_MAX).all()
    # where the over-fetch found rows they are a prefix of the exact answer
    for r_old, r_new in zip(old, M):
        assert r_new[:len(r_old)] == r_old


# ---------------------------------------------------------------------------
# TCP transport
# ---------------------------------------------------------------------------


def test_search_filtered_over_tcp(tmp_path):
    from distributed_faiss_amd.rpc import TcpClient, TcpServer

    srv = IndexServer(0, str(tmp_path), provider=FilteredOracleProvider())
    tcp = TcpServer(srv, port=0)
    tcp.start_background()
    try:
        cli = TcpClient("127.0.0.1", tcp.port)
        cfg = IndexCfg(index_builder_type="flat", dim=16, train_num=4)
        assert cli.create_index("t", cfg) is True
        emb = np.random.default_rng(0).random((12, 16), dtype=np.float32)
        metas = [("m", i % 3) for i in range(12)]
        cli.add_index_data("t", emb, metas, False)
        assert _wait(lambda: cli.get_state("t") == IndexState.TRAINED
                     and cli.get_ntotal("t") == 12)
        D, I, M, E = cli.search_filtered("t", emb[:2], 5, 1, 0)
        assert D.shape == (2, 5) and I.shape == (2, 5) and E is None
        assert (I >= 0).all() and (I % 3 != 0).all()
        assert M == [[metas[j] for j in row] for row in I]
        cli.close()
    finally:
        tcp.stop()


# ---------------------------------------------------------------------------
# dist mode (gloo world 2) equals the classic topology
# ---------------------------------------------------------------------------


def _dist_worker(rank, world, tmpdir, metric):
    import torch.distributed as dist

    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = "29587" if metric == "dot" else "29588"
    dist.init_process_group("gloo", rank=rank, world_size=world)

    batches, metas, q = _data()
    top_k = 6
    srv = IndexServer(rank, os.path.join(tmpdir, f"dist{rank}"),
                      provider=FilteredOracleProvider())
    client = IndexClient(servers=[srv], distributed=None)
    assert client.dist_mode and client.get_num_servers() == world
    client.create_index("idx", IndexCfg(**_cfg(metric)))
    for b, m in zip(batches, metas):
        client.add_index_data("idx", b, m, train_async_if_triggered=False)
    local = sum(b.shape[0] for bi, b in enumerate(batches) if bi % world == rank)
    assert _wait(lambda: srv.get_state("idx") == IndexState.TRAINED
                 and srv.get_ntotal("idx") == local)
    dist.barrier()

    D, M = client.search_filtered(q, top_k, "idx", 1, 2)
    assert D.shape == (9, top_k)
    # each shard searched top_k rows, not 3 * top_k
    (allow,) = srv.indexes["idx"].engine.filtered_calls
    assert allow.shape[0] == local
    from distributed_faiss_amd.dist import all_gather_object

    Ds = all_gather_object(D.tolist())
    Ms = all_gather_object(M)
    assert Ds[0] == Ds[1] and Ms[0] == Ms[1]

    if rank == 0:
        prov = FilteredOracleProvider()
        servers = [IndexServer(r, os.path.join(tmpdir, "classic"), provider=prov)
                   for r in range(world)]
        classic = IndexClient(servers=servers, distributed=False)
        _fill(classic, servers, "idx", _cfg(metric), batches, metas)
        Dc, Mc = classic.search_filtered(q, top_k, "idx", 1, 2)
        np.testing.assert_array_equal(D, Dc)
        assert M == Mc
        for r in M:
            for m in r:
                assert m[1] != 2
        if metric == "dot":
            assert (D <= 0).any()  # negated dot scores, like search()
    dist.destroy_process_group()


@pytest.mark.parametrize("metric", ["dot", "l2"])
def test_client_dist_world2_equals_classic(tmp_path, metric):
    pytest.importorskip("torch")
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_dist_worker, args=(r, 2, str(tmp_path), metric))
             for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=240)
    for p in procs:
        assert p.exitcode == 0
