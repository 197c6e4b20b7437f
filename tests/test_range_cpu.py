# Range search, the layers above the engine (no GPU): Index state check,
# filter bitmap cache and growth retry, server, client shard concatenation
# and score sign, the dist-mode gather and the TCP transport. The engine is
# the CPU oracle wrapped by a test-local provider whose range_search is
# DEFINED as: oracle search at k = ntotal (the full ranking), thresholded
# with the strict radius test and masked to the allowed ids, kept in
# ranking order.
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


class RangeOracleEngine:
    """Oracle engine + range_search(q, radius, allow=None). Records the
    allow masks it was called with."""

    def __init__(self, inner):
        self.__dict__["inner"] = inner
        self.__dict__["range_calls"] = []
        self.__dict__["before_range"] = None

    def __getattr__(self, name):
        return getattr(self.__dict__["inner"], name)

    def __setattr__(self, name, value):
        setattr(self.__dict__["inner"], name, value)

    def range_search(self, q, radius, allow=None):
        inner = self.inner
        self.range_calls.append(None if allow is None
                                else np.asarray(allow, bool).copy())
        nq = q.shape[0]
        lims = np.zeros(nq + 1, np.int64)
        Ds, Is = [], []
        if inner.ntotal:
            Df, If = inner.search(q, inner.ntotal)
            for i in range(nq):
                keep = If[i] >= 0
                keep &= (Df[i] < radius) if inner.metric == 1 else (Df[i] > radius)
                if allow is not None:
                    assert len(allow) >= inner.ntotal
                    keep[keep] = np.asarray(allow, bool)[If[i][keep]]
                Ds.append(Df[i][keep])
                Is.append(If[i][keep])
                lims[i + 1] = lims[i] + int(keep.sum())
        D = np.concatenate(Ds) if Ds else np.empty(0, np.float32)
        I = np.concatenate(Is) if Is else np.empty(0, np.int64)
        return lims, D.astype(np.float32), I.astype(np.int64)


class RangeOracleProvider:
    def __init__(self):
        self.inner = OracleProvider()

    def create(self, spec):
        return RangeOracleEngine(self.inner.create(spec))

    def load(self, path):
        return RangeOracleEngine(self.inner.load(path))


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
    idx = Index(cfg, provider=provider or RangeOracleProvider())
    idx.add_batch(xb, metas, train_async_if_triggered=False)
    assert _wait(lambda: idx.get_state() == IndexState.TRAINED
                 and idx.engine.ntotal == n)
    return idx, xb


def _brute(xb, q, radius, metric, allow=None):
    """Per query: the set of (id) passing the strict test, and the values."""
    out = []
    for qi in q.astype(np.float64):
        x = xb.astype(np.float64)
        v = ((x - qi) ** 2).sum(1) if metric == "l2" else x @ qi
        hit = v < radius if metric == "l2" else v > radius
        if allow is not None:
            hit &= allow
        out.append((set(np.flatnonzero(hit).tolist()), v))
    return out


# ---------------------------------------------------------------------------
# Index
# ---------------------------------------------------------------------------


def test_index_range_search_and_state_check(tmp_path):
    metas = [("doc", i % 4) for i in range(60)]
    cfg = IndexCfg(faiss_factory="Flat", dim=8, metric="l2", train_num=1000,
                   index_storage_dir=str(tmp_path / "u"))
    untrained = Index(cfg, provider=RangeOracleProvider())
    with pytest.raises(RuntimeError, match="not trained"):
        untrained.range_search(np.zeros((1, 8), np.float32), 1.0)

    idx, xb = _flat_index(tmp_path / "t", metas)
    q = xb[:5] + 0.05
    radius = 9.0
    lims, scores, ids, meta = idx.range_search(q, radius)
    assert lims.shape == (6,) and lims[0] == 0 and lims[-1] == len(scores)
    assert len(ids) == len(meta) == len(scores) > 5
    assert meta == [metas[j] for j in ids]
    for i, (want, v) in enumerate(_brute(xb, q, radius, "l2")):
        got = ids[lims[i]:lims[i + 1]]
        assert set(got.tolist()) == want and len(got) == len(want)
        np.testing.assert_allclose(scores[lims[i]:lims[i + 1]], v[got],
                                   rtol=1e-4, atol=1e-4)
    assert idx.engine.range_calls == [None]  # no filter: no bitmap built
    assert len(idx._filter_cache) == 0


def test_index_filter_cache_reuse_and_growth(tmp_path):
    metas = [("doc", i % 4) for i in range(40)]
    idx, xb = _flat_index(tmp_path, metas)
    q = xb[:3]
    radius = 12.0
    allow = np.array([m[1] != 2 for m in metas])
    lims, scores, ids, meta = idx.range_search(q, radius, 1, 2)
    np.testing.assert_array_equal(idx.engine.range_calls[-1][:40], allow)
    for i, (want, _v) in enumerate(_brute(xb, q, radius, "l2", allow)):
        assert set(ids[lims[i]:lims[i + 1]].tolist()) == want
    assert all(m[1] != 2 for m in meta) and len(meta) > 0
    # the cache entry of search_filtered is shared and reused
    assert len(idx._filter_cache) == 1
    (entry,) = idx._filter_cache.values()
    packed = entry["packed"]
    idx.range_search(q, radius, 1, 2)
    (entry,) = idx._filter_cache.values()
    assert entry["packed"] is packed
    # growth: the bitmap is extended by the tail
    more = [("doc", i % 4) for i in range(40, 52)]
    xb2 = np.random.default_rng(5).standard_normal((12, 8), dtype=np.float32)
    idx.add_batch(xb2, more)
    assert _wait(lambda: idx.get_state() == IndexState.TRAINED
                 and idx.engine.ntotal == 52)
    lims, scores, ids, meta = idx.range_search(q, radius, 1, 2)
    assert idx.engine.range_calls[-1].shape[0] == 52
    allow2 = np.array([m[1] != 2 for m in metas + more])
    xall = np.concatenate([xb, xb2])
    for i, (want, _v) in enumerate(_brute(xall, q, radius, "l2", allow2)):
        assert set(ids[lims[i]:lims[i + 1]].tolist()) == want


def test_index_retries_when_rows_arrive_while_the_bitmap_is_built(tmp_path):
    metas = [("doc", i % 4) for i in range(30)]
    idx, xb = _flat_index(tmp_path, metas)
    xb2 = np.random.default_rng(6).standard_normal((6, 8), dtype=np.float32)
    more = [("doc", 2)] * 6
    inner_filter_for = idx._filter_for
    grown = []

    def racing(engine, ntotal, pos, val):
        flt = inner_filter_for(engine, ntotal, pos, val)
        if not grown:  # rows arrive after the bitmap was built
            grown.append(True)
            idx.add_batch(xb2, more)
            assert _wait(lambda: idx.engine.ntotal == 36
                         and idx.get_state() == IndexState.TRAINED)
        return flt

    idx._filter_for = racing
    lims, scores, ids, meta = idx.range_search(xb[:2], 1e9, 1, 2)
    # one engine call only, with a bitmap that covers the grown index
    assert len(idx.engine.range_calls) == 1
    assert idx.engine.range_calls[0].shape[0] == 36
    assert all(m[1] != 2 for m in meta)
    assert np.diff(lims).tolist() == [sum(m[1] != 2 for m in metas)] * 2


def test_engine_without_range_search_raises(tmp_path):
    idx, xb = _flat_index(tmp_path, [("doc", i) for i in range(10)],
                          provider=OracleProvider())
    with pytest.raises(NotImplementedError, match="HIP engine"):
        idx.range_search(xb[:1], 1.0)


# ---------------------------------------------------------------------------
# server and client
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
    metas = [[("b%d" % bi, i % 4, bi * per + i) for i in range(per)]
             for bi in range(nb)]
    q = np.random.default_rng(99).standard_normal((9, d), dtype=np.float32)
    return batches, metas, q


def _cfg(metric):
    if metric == "dot":
        return dict(index_builder_type="flat", dim=16, train_num=10,
                    metric="dot")
    return dict(faiss_factory="Flat", dim=16, train_num=10, metric="l2")


RADIUS = {"l2": 22.0, "dot": 4.0}


def _check_client_result(res, parts, q, metric, batches, filtered):
    lims, scores, meta = res
    nq = q.shape[0]
    assert lims.dtype == np.int64 and lims.shape == (nq + 1,) and lims[0] == 0
    assert lims[-1] == len(scores) == len(meta) > nq
    for i in range(nq):
        want_s = np.concatenate([p[1][p[0][i]:p[0][i + 1]] for p in parts])
        want_m = sum((list(p[3][p[0][i]:p[0][i + 1]]) for p in parts), [])
        np.testing.assert_array_equal(scores[lims[i]:lims[i + 1]], want_s)
        assert meta[lims[i]:lims[i + 1]] == want_m
    xb = np.concatenate(batches)
    allow = np.array([(j % 25) % 4 != 2 for j in range(xb.shape[0])]) \
        if filtered else None
    for i, (want, v) in enumerate(_brute(xb, q, RADIUS[metric], metric, allow)):
        rows = [m[2] for m in meta[lims[i]:lims[i + 1]]]
        assert set(rows) == want and len(rows) == len(want)
        # the score is the true value: squared l2, or the dot product
        # itself — NOT negated
        np.testing.assert_allclose(scores[lims[i]:lims[i + 1]], v[rows],
                                   rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_client_concatenates_shards_in_order(tmp_path, metric, filtered):
    batches, metas, q = _data()
    prov = RangeOracleProvider()
    servers = [IndexServer(r, str(tmp_path / "four"), provider=prov)
               for r in range(4)]
    cli = IndexClient(servers=servers, distributed=False)
    _fill(cli, servers, "idx", _cfg(metric), batches, metas)
    fp, fv = (1, 2) if filtered else (None, None)
    parts = [s.range_search("idx", q, RADIUS[metric], fp, fv) for s in servers]
    assert all(len(p) == 4 and len(p[3]) == len(p[1]) == p[0][-1] for p in parts)
    res = cli.range_search(q, RADIUS[metric], "idx", fp, fv)
    _check_client_result(res, parts, q, metric, batches, filtered)
    if metric == "dot":
        assert (res[1] > RADIUS["dot"]).all()


def test_range_search_over_tcp(tmp_path):
    from distributed_faiss_amd.rpc import TcpClient, TcpServer

    srv = IndexServer(0, str(tmp_path), provider=RangeOracleProvider())
    tcp = TcpServer(srv, port=0)
    tcp.start_background()
    try:
        cli = TcpClient("127.0.0.1", tcp.port)
        cfg = IndexCfg(faiss_factory="Flat", dim=16, train_num=4, metric="l2")
        assert cli.create_index("t", cfg) is True
        emb = np.random.default_rng(0).random((12, 16), dtype=np.float32)
        metas = [("m", i % 3) for i in range(12)]
        cli.add_index_data("t", emb, metas, False)
        assert _wait(lambda: cli.get_state("t") == IndexState.TRAINED
                     and cli.get_ntotal("t") == 12)
        lims, D, I, M = cli.range_search("t", emb[:2], 2.5, 1, 0)
        assert lims.shape == (3,) and lims[-1] == len(D) == len(I) == len(M) > 2
        assert (I % 3 != 0).all() and (D < 2.5).all()
        assert M == [metas[j] for j in I]
        want = srv.range_search("t", emb[:2], 2.5, 1, 0)
        np.testing.assert_array_equal(I, want[2])
        np.testing.assert_array_equal(D, want[1])
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
    os.environ["MASTER_PORT"] = "29591" if metric == "dot" else "29592"
    dist.init_process_group("gloo", rank=rank, world_size=world)

    batches, metas, q = _data()
    srv = IndexServer(rank, os.path.join(tmpdir, f"dist{rank}"),
                      provider=RangeOracleProvider())
    client = IndexClient(servers=[srv], distributed=None)
    assert client.dist_mode and client.get_num_servers() == world
    client.create_index("idx", IndexCfg(**_cfg(metric)))
    for b, m in zip(batches, metas):
        client.add_index_data("idx", b, m, train_async_if_triggered=False)
    local = sum(b.shape[0] for bi, b in enumerate(batches) if bi % world == rank)
    assert _wait(lambda: srv.get_state("idx") == IndexState.TRAINED
                 and srv.get_ntotal("idx") == local)
    dist.barrier()

    lims, scores, meta = client.range_search(q, RADIUS[metric], "idx", 1, 2)
    from distributed_faiss_amd.dist import all_gather_object

    seen = all_gather_object((lims.tolist(), scores.tolist(), meta))
    assert seen[0] == seen[1]  # every rank holds the same answer

    if rank == 0:
        prov = RangeOracleProvider()
        servers = [IndexServer(r, os.path.join(tmpdir, "classic"), provider=prov)
                   for r in range(world)]
        classic = IndexClient(servers=servers, distributed=False)
        _fill(classic, servers, "idx", _cfg(metric), batches, metas)
        lc, sc, mc = classic.range_search(q, RADIUS[metric], "idx", 1, 2)
        np.testing.assert_array_equal(lims, lc)
        np.testing.assert_array_equal(scores, sc)
        assert meta == mc and len(meta) > 9
        assert all(m[1] != 2 for m in meta)
        if metric == "dot":
            assert (scores > RADIUS["dot"]).all()  # un-negated
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
