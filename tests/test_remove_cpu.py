# remove_ids, the layers above the engine (no GPU): Index bookkeeping and
# saving, server / client plumbing. The engine is the CPU oracle wrapped by a
# test-local stub that records remove_ids calls, tracks ntotal / nlive and
# hides removed ids from search (oracle search at k = ntotal, masked).
import os
import pickle

import numpy as np
import pytest

from distributed_faiss_amd import (
    IndexCfg,
    IndexClient,
    IndexServer,
    IndexState,
)
from distributed_faiss_amd.index import Index, get_index_files
from oracle import OracleProvider

FLT_MAX = np.float32(3.4028235e38)


class RemovingEngine:
    """Oracle engine + remove_ids(ids) / nlive. Ids are never reused."""

    def __init__(self, inner, removed=()):
        self.__dict__["inner"] = inner
        self.__dict__["removed"] = set(int(i) for i in removed)
        self.__dict__["remove_calls"] = []

    def __getattr__(self, name):
        return getattr(self.__dict__["inner"], name)

    def __setattr__(self, name, value):
        setattr(self.__dict__["inner"], name, value)

    @property
    def nlive(self):
        return self.inner.ntotal - len(self.removed)

    def remove_ids(self, ids):
        ids = [int(i) for i in np.asarray(ids).reshape(-1)]
        assert all(0 <= i < self.inner.ntotal for i in ids)
        self.remove_calls.append(ids)
        new = set(ids) - self.removed
        self.removed.update(new)
        return len(new)

    def search(self, q, k):
        inner = self.inner
        nq = q.shape[0]
        pad = FLT_MAX if inner.metric == 1 else -FLT_MAX
        D = np.full((nq, k), pad, np.float32)
        I = np.full((nq, k), -1, np.int64)
        if inner.ntotal == 0:
            return D, I
        Df, If = inner.search(q, inner.ntotal)
        for i in range(nq):
            keep = np.array([j >= 0 and j not in self.removed for j in If[i]])
            n = min(k, int(keep.sum()))
            D[i, :n] = Df[i][keep][:n]
            I[i, :n] = If[i][keep][:n]
        return D, I

    def save(self, path):
        self.inner.save(path)
        with open(path + ".removed", "wb") as f:
            pickle.dump(sorted(self.removed), f)


class RemovingProvider:
    def __init__(self):
        self.inner = OracleProvider()

    def create(self, spec):
        return RemovingEngine(self.inner.create(spec))

    def load(self, path):
        removed = ()
        if os.path.exists(path + ".removed"):
            with open(path + ".removed", "rb") as f:
                removed = pickle.load(f)
        return RemovingEngine(self.inner.load(path), removed)


def _metas(n, base=0):
    return [(base + i, f"doc{base + i}") for i in range(n)]


def _index(tmp_path, n=40, d=8, provider=None, base=0):
    xb = np.random.default_rng(base).standard_normal((n, d), dtype=np.float32)
    cfg = IndexCfg(faiss_factory="Flat", dim=d, metric="l2", train_num=1,
                   index_storage_dir=str(tmp_path))
    idx = Index(cfg, provider=provider or RemovingProvider())
    idx.add_batch(xb, _metas(n, base), train_async_if_triggered=False)
    _wait_trained(idx, n)
    return idx, xb


def _wait_trained(idx, ntotal):
    import time

    t0 = time.time()
    while time.time() - t0 < 30:
        if idx.get_state() == IndexState.TRAINED and idx.engine.ntotal == ntotal:
            return
        time.sleep(0.01)
    raise AssertionError("index did not reach TRAINED")


# ---------------------------------------------------------------------------
# Index
# ---------------------------------------------------------------------------


def test_index_remove_ids(tmp_path):
    idx, xb = _index(tmp_path)
    assert idx.get_idx_data_num() == (0, 40)
    assert idx.remove_ids([3, 5, 5, 39]) == 3
    assert idx.engine.remove_calls == [[3, 5, 39]]
    assert [i for i, m in enumerate(idx.id_to_metadata) if m is None] == [3, 5, 39]
    assert idx.get_ids() == set(range(40)) - {3, 5, 39}
    assert idx.metadata_for(np.array([[3, 4, -1]])) == [[None, (4, "doc4"), None]]
    # live rows are what the index reports; ids stay arrival positions
    assert idx.get_idx_data_num() == (0, 37)
    assert idx.engine.ntotal == 40
    _, ids, meta, _ = idx.search_full(xb[[3, 4]], 1)
    assert ids[1, 0] == 4 and meta[1][0] == (4, "doc4")
    assert ids[0, 0] not in (3, 5, 39) and meta[0][0] is not None
    # removing them again removes nothing
    assert idx.remove_ids([3, 39]) == 0
    assert idx.remove_ids([]) == 0
    assert idx.get_idx_data_num() == (0, 37)


def test_index_remove_by_meta_ids(tmp_path):
    idx, xb = _index(tmp_path, base=100)  # meta ids 100..139 on rows 0..39
    assert idx.remove_by_meta_ids([100, 117, 999]) == 2
    assert idx.engine.remove_calls == [[0, 17]]
    assert idx.get_ids() == set(range(100, 140)) - {100, 117}
    assert idx.metadata_for(np.array([[0, 17, 1]])) == [[None, None, (101, "doc101")]]
    assert idx.remove_by_meta_ids({100, 117}) == 0  # already gone
    assert len(idx.engine.remove_calls) == 1
    # rows added later get new ids
    idx.add_batch(xb[:2], _metas(2, 500), train_async_if_triggered=False)
    _wait_trained(idx, 42)
    assert idx.get_idx_data_num() == (0, 40)
    assert idx.remove_by_meta_ids([501]) == 1
    assert idx.engine.remove_calls[-1] == [41]


def test_filter_predicate_stops_seeing_removed_rows(tmp_path):
    idx, _ = _index(tmp_path)
    idx.remove_ids([0, 1])
    with idx.buffer_lock:
        allowed = [Index._filter_allows(m, 1, "doc2") for m in idx.id_to_metadata]
    assert allowed[:4] == [False, False, False, True]


def test_engine_without_remove_ids(tmp_path):
    idx, _ = _index(tmp_path, provider=OracleProvider())
    with pytest.raises(NotImplementedError, match="has no remove_ids"):
        idx.remove_ids([1])
    with pytest.raises(NotImplementedError, match="has no remove_ids"):
        idx.remove_by_meta_ids([1])
    assert idx.get_ids() == set(range(40))
    assert idx.get_idx_data_num() == (0, 40)  # an engine without nlive


def test_not_trained_is_refused(tmp_path):
    cfg = IndexCfg(faiss_factory="Flat", dim=8, metric="l2", train_num=100,
                   index_storage_dir=str(tmp_path))
    idx = Index(cfg, provider=RemovingProvider())
    idx.add_batch(np.zeros((4, 8), np.float32), _metas(4))
    assert idx.get_state() == IndexState.NOT_TRAINED
    with pytest.raises(RuntimeError, match="not trained"):
        idx.remove_ids([0])
    with pytest.raises(RuntimeError, match="not trained"):
        idx.remove_by_meta_ids([0])
    assert idx.get_ids() == {0, 1, 2, 3}


# ---------------------------------------------------------------------------
# saving
# ---------------------------------------------------------------------------


def test_maybe_save_writes_after_a_removal(tmp_path):
    idx, _ = _index(tmp_path)
    index_file, meta_file, _, _ = get_index_files(str(tmp_path))
    assert idx.save() is True
    assert idx.save() is False  # nothing changed
    stamp = os.path.getmtime(meta_file)
    os.utime(meta_file, (stamp - 10, stamp - 10))
    assert idx.remove_ids([7]) == 1
    assert idx.engine.ntotal == 40  # unchanged: the old check would skip
    assert idx.save() is True
    assert os.path.getmtime(meta_file) > stamp - 10
    with open(meta_file, "rb") as f:
        assert pickle.load(f)[7] is None
    assert idx.save() is False


def test_from_storage_dir_keeps_the_holes(tmp_path):
    idx, xb = _index(tmp_path)
    idx.remove_ids([2, 3])
    assert idx.save() is True
    got = Index.from_storage_dir(str(tmp_path), provider=RemovingProvider())
    assert got is not None and got.get_state() == IndexState.TRAINED
    assert len(got.id_to_metadata) == 40
    assert got.id_to_metadata[2] is None and got.id_to_metadata[3] is None
    assert got.get_ids() == set(range(40)) - {2, 3}
    assert got.get_idx_data_num() == (0, 38)
    _, ids, meta, _ = got.search_full(xb[[2, 4]], 1)
    assert ids[0, 0] not in (2, 3) and ids[1, 0] == 4
    assert meta[1][0] == (4, "doc4")


# ---------------------------------------------------------------------------
# server / client
# ---------------------------------------------------------------------------


def _two_shards(tmp_path):
    servers = [IndexServer(r, str(tmp_path), provider=RemovingProvider())
               for r in range(2)]
    client = IndexClient(servers=servers)
    cfg = IndexCfg(faiss_factory="Flat", dim=8, metric="l2", train_num=1)
    client.create_index("t", cfg)
    rng = np.random.default_rng(5)
    for b in range(4):  # round-robin: two batches of 10 rows per shard
        client.add_index_data(
            "t", rng.standard_normal((10, 8), dtype=np.float32),
            _metas(10, 10 * b), train_async_if_triggered=False)
    for s in servers:
        _wait_trained(s.indexes["t"], 20)
    return servers, client


def test_client_remove_ids_over_two_shards(tmp_path):
    servers, client = _two_shards(tmp_path)
    assert client.get_ids("t") == set(range(40))
    assert client.get_ntotal("t") == 40
    gone = [0, 9, 10, 25, 39, 1234]
    assert client.remove_ids("t", gone) == 5
    assert client.get_ids("t") == set(range(40)) - set(gone)
    assert client.get_ntotal("t") == 35
    per_shard = [s.get_nlive("t") for s in servers]
    assert sum(per_shard) == 35 and all(n < 20 for n in per_shard)
    assert client.remove_ids("t", gone) == 0
    # no search returns a removed document
    q = np.random.default_rng(6).standard_normal((3, 8), dtype=np.float32)
    _, meta = client.search(q, 35, "t")
    for row in meta:
        assert {m[0] for m in row} == set(range(40)) - set(gone)


def test_server_remove_ids(tmp_path):
    servers, _ = _two_shards(tmp_path)
    s = servers[0]
    before = s.get_ids("t")
    victim = s.indexes["t"].id_to_metadata[4][0]
    assert s.remove_ids("t", [4]) == 1
    assert s.get_ids("t") == before - {victim}
    assert s.get_nlive("t") == s.get_ntotal("t") == 19
    assert s.remove_by_meta_ids("t", [victim]) == 0
    with pytest.raises(RuntimeError, match="no index"):
        s.remove_ids("nope", [0])
