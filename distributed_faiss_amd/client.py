# IndexClient: shard fan-out + top-k merge.
#
# Keeps the reference's client surface (distributed_faiss/client.py:57-345):
# create/load/save/drop index, add_index_data round-robin placement
# (client.py:174-192), search fan-out + merge (client.py:200-210,265-310),
# search_with_filter (client.py:213-263), get_state aggregation, get_ntotal
# sum, get_centroids, set_nprobe, get_ids. Differences from the reference:
#   * shards are in-process IndexServer objects (or, multi-GPU, one rank per
#     GPU via distributed_faiss_amd.dist) instead of pickle-TCP rpc.Client
#     proxies — the RPC layer is retired for the intra-node path
#     (BASELINE.json north_star; reference rpc.py out of scope per
#     SURVEY.md §2).
#   * the merge is a numpy restatement of ResultHeap
#     (faiss.float_maxheap_array_t, client.py:29-54) pinned by the
#     reference's own merge KAT (tests/test_integration.py:181-203, ported
#     into tests/test_merge.py).
#
# Merge semantics mirrored EXACTLY, including reference quirk 2
# (SURVEY.md §2): for metric "dot" the client pushes -D into the
# min-oriented merge and NEVER flips the sign back — returned scores for
# dot are negated. Unfilled shard slots arrive as D=+FLT_MAX (L2) /
# -FLT_MAX (dot) with id -1 and meta None, and lose the merge naturally.

import itertools
import logging
import os
import random
import time
from multiprocessing.dummy import Pool as ThreadPool
from typing import List, Optional, Tuple

import numpy as np

from .index_cfg import IndexCfg
from .index_state import IndexState
from .server import IndexServer, resolve_inproc_server

logger = logging.getLogger()


class ResultHeap:
    """Merge accumulator, numpy restatement of reference client.py:29-54.

    Keeps the k SMALLEST values per query (the caller negates for
    maximize). Ties break toward the earlier-added synthetic id, which is
    deterministic (faiss's heap order on ties is unspecified; the KAT has
    no ties).
    """

    def __init__(self, nq, k):
        self.nq, self.k = nq, k
        self._vals = []   # list of (nq, k) fp32
        self._ids = []    # list of (nq, k) int64
        self.D = None
        self.I = None

    def add_result(self, D, I):
        assert D.shape == (self.nq, self.k)
        assert I.shape == (self.nq, self.k)
        self._vals.append(np.asarray(D, dtype=np.float32))
        self._ids.append(np.asarray(I, dtype=np.int64))

    def finalize(self):
        allD = np.concatenate(self._vals, axis=1)
        allI = np.concatenate(self._ids, axis=1)
        # row-wise lexsort, vectorized (the per-row Python loop dominated
        # the in-process serving path at 10k-query batches — VERDICT r1);
        # same (value, synthetic id) order as the loop it replaces
        order = np.lexsort((allI, allD), axis=-1)[:, : self.k]
        self.D = np.take_along_axis(allD, order, axis=1).astype(np.float32)
        self.I = np.take_along_axis(allI, order, axis=1)


def _dist_ctx():
    """(rank, world) of the active torch.distributed group, (0, 1) when
    none. Import is lazy — the in-process client path works without
    torch."""
    try:
        import torch.distributed as td

        if td.is_available() and td.is_initialized():
            return td.get_rank(), td.get_world_size()
    except ImportError:
        pass
    return 0, 1


class IndexClient:
    """Manages a set of shard sub-indexes; searches merge client-side.

    Two topologies behind the SAME surface:
      * in-process (reference-shaped): N IndexServer objects, thread-pool
        fan-out, numpy ResultHeap merge.
      * distributed (MI355X-native, BASELINE.json north_star): one rank
        per GPU shard under torch.distributed, auto-detected when the
        process group is initialized with world > 1 and the client was
        handed exactly its LOCAL server. search() then runs: local shard
        search -> all-gather of per-shard (distance, id) top-k (RCCL
        over xGMI on GPU, gloo on CPU) -> k-way merge (on-GPU
        dfann_merge_topk / numpy) -> metadata mapped from (shard, slot)
        exactly as the reference maps synthetic ids
        (ref client.py:290,297-298). Merge semantics (incl. quirk-2 dot
        negation) are identical to the in-process path, and search_dev()
        exposes the same pipeline with device-resident results — the
        bench's timed step IS this client path.
    """

    def __init__(self, server_list_path=None, cfg_path: Optional[str] = None,
                 servers=None, distributed: Optional[bool] = None):
        """Either pass `servers` (list of in-process IndexServer) or
        `server_list_path` (reference format: first line = count, then
        host,port lines — resolved against the in-process port registry).
        `distributed` overrides the auto-detection described above."""
        self._dist_rank, self._dist_world = _dist_ctx()
        if servers is not None:
            self.sub_indexes: List[IndexServer] = list(servers)
        else:
            machine_ports = IndexClient.read_server_list(server_list_path)
            self.sub_indexes = []
            for host, port in machine_ports:
                try:
                    self.sub_indexes.append(resolve_inproc_server(port))
                except ConnectionError:
                    # multi-node: fall back to the TCP transport (rpc.py)
                    from .rpc import TcpClient

                    self.sub_indexes.append(TcpClient(host, port))
        self.num_indexes = len(self.sub_indexes)
        if distributed is None:
            distributed = self._dist_world > 1 and self.num_indexes == 1
        self.dist_mode = bool(distributed)
        # logical shard count: ranks in dist mode, local servers otherwise
        self.num_shards = self._dist_world if self.dist_mode else self.num_indexes

        index_ranks = [idx.get_rank() for idx in self.sub_indexes]
        self.index_rank_to_id = {
            index_rank: index_id for index_id, index_rank in enumerate(index_ranks)
        }

        self.pool = ThreadPool(self.num_indexes)
        self.verbose = False
        self.cur_server_ids = {}
        random.seed(time.time())
        self.cfg = IndexCfg.from_json(cfg_path) if cfg_path is not None else None

    @staticmethod
    def read_server_list(
        server_list_path,
        initial_timeout=0.1,
        backoff_factor=1.5,
        total_max_timeout=7200,
    ) -> List[Tuple[str, int]]:
        # reference client.py:87-120 restated, including the no-success-break
        # spin (quirk 8): loop until the timeout accumulator trips, then
        # assert the count.
        time_waited = 0
        while True:
            with open(server_list_path) as f:
                res = []
                num_servers = 0
                for idx, line in enumerate(f):
                    if idx == 0:
                        num_servers = int(line)
                        continue
                    res.append((str(line.split(",")[0]), int(line.split(",")[1])))

            msg = f"{num_servers} != {len(res)} in server list {server_list_path}."
            if num_servers != len(res):
                time.sleep(initial_timeout)
            if time_waited + initial_timeout >= total_max_timeout:
                break
            time_waited += initial_timeout
            initial_timeout *= backoff_factor

        assert num_servers == len(res), (
            msg + f" Timed out after waiting {round(time_waited * 100) / 100} seconds"
        )
        return res

    # -- index management --------------------------------------------------

    def create_index(self, index_id: str, cfg: Optional[IndexCfg] = None):
        if cfg is not None:
            self.cfg = cfg
        if self.cfg is None:
            self.cfg = IndexCfg()
        return self.pool.map(lambda idx: idx.create_index(index_id, self.cfg), self.sub_indexes)

    def load_index(
        self, index_id: str, cfg: Optional[IndexCfg] = None, force_reload: bool = True
    ) -> bool:
        def setup_cfg(cfg):
            if cfg is None:
                config_paths = self.pool.map(
                    lambda idx: idx.get_config_path(index_id), self.sub_indexes
                )
                if len(config_paths) > 0 and os.path.isfile(config_paths[0]):
                    cfg = IndexCfg.from_json(config_paths[0])
                else:
                    cfg = IndexCfg()
            return cfg

        if force_reload:
            self.pool.map(lambda idx: idx.drop_index(index_id), self.sub_indexes)
        all_loaded = self.pool.map(lambda idx: idx.load_index(index_id, cfg), self.sub_indexes)
        if self.dist_mode:
            from .dist import all_gather_object

            all_loaded = all_gather_object(all_loaded[0])
        self.cfg = setup_cfg(cfg)
        if all(all_loaded):
            return True
        if any(all_loaded):
            logger.warning(f"Some server nodes can't load index: {all_loaded}")
        return False

    def save_index(self, index_id: str):
        self.pool.map(lambda idx: idx.save_index(index_id), self.sub_indexes)

    def drop_index(self, index_id: str):
        self.pool.map(lambda idx: idx.drop_index(index_id), self.sub_indexes)

    # -- data path ---------------------------------------------------------

    def add_index_data(
        self,
        index_id: str,
        embeddings: np.ndarray,
        metadata: Optional[List[object]] = None,
        train_async_if_triggered: bool = True,
    ) -> None:
        # round-robin placement, random start (reference client.py:174-192)
        if self.dist_mode:
            # SPMD: every rank sees the same batch stream; batch i lands
            # on shard i % world. Deterministic start 0 (deviation from
            # the reference's random start — ranks must agree).
            if index_id not in self.cur_server_ids:
                self.cur_server_ids[index_id] = 0
            if self.cur_server_ids[index_id] == self._dist_rank:
                self.sub_indexes[0].add_index_data(
                    index_id, embeddings, metadata, train_async_if_triggered
                )
            self.cur_server_ids[index_id] = (
                self.cur_server_ids[index_id] + 1) % self.num_shards
            return
        if index_id not in self.cur_server_ids:
            self.cur_server_ids[index_id] = random.randint(0, self.num_indexes - 1)
        cur_server_id = self.cur_server_ids[index_id]
        self.sub_indexes[cur_server_id].add_index_data(
            index_id, embeddings, metadata, train_async_if_triggered
        )
        self.cur_server_ids[index_id] = (self.cur_server_ids[index_id] + 1) % self.num_indexes

    def sync_train(self, index_id: str) -> None:
        self.pool.map(lambda idx: idx.sync_train(index_id), self.sub_indexes)

    def async_train(self, index_id: str):
        # reference quirk 4: client.async_train == sync_train (client.py:197-198)
        self.pool.map(lambda idx: idx.sync_train(index_id), self.sub_indexes)

    def search(
        self, query, topk: int, index_id: str, return_embeddings: bool = False
    ) -> Tuple[np.ndarray, List]:
        q_size = query.shape[0]
        maximize_metric: bool = self.cfg.metric == "dot"
        if self.dist_mode:
            return self._dist_search(query, topk, index_id, maximize_metric,
                                     return_embeddings)
        results = self.pool.imap(
            lambda idx: idx.search(index_id, query, topk, return_embeddings), self.sub_indexes
        )
        return self._aggregate_results(results, topk, q_size, maximize_metric, return_embeddings)

    def search_filtered(
        self, query: np.ndarray, top_k: int, index_id: str,
        filter_pos: int, filter_value
    ) -> Tuple[np.ndarray, List[List[object]]]:
        """Exact filtered search: the top_k nearest rows among those the
        filter keeps (metadata m truthy, len(m) > filter_pos and
        m[filter_pos] != filter_value — the predicate of
        search_with_filter). Each shard applies the filter as an
        allow-bitmap inside its scan kernels, so every query gets top_k
        rows whenever that many allowed rows exist in the probed lists, at
        any selectivity, and shards search (and gather) top_k rows, not
        3 * top_k. Return format of search(): (nq, top_k) scores (negated
        for dot, like search) and metadata with None at pads."""
        q_size = query.shape[0]
        maximize_metric: bool = self.cfg.metric == "dot"
        if self.dist_mode:
            return self._dist_search(
                query, top_k, index_id, maximize_metric, False,
                local_search=lambda: self.sub_indexes[0].search_filtered(
                    index_id, query, top_k, filter_pos, filter_value))

        def one(idx):
            scores, _ids, meta, embs = idx.search_filtered(
                index_id, query, top_k, filter_pos, filter_value)
            return scores, meta, embs

        results = self.pool.imap(one, self.sub_indexes)
        return self._aggregate_results(results, top_k, q_size, maximize_metric, False)

    def range_search(
        self, query: np.ndarray, radius: float, index_id: str,
        filter_pos=None, filter_value=None
    ) -> Tuple[np.ndarray, np.ndarray, List[object]]:
        """faiss Index.range_search over all shards: every row of the probed
        lists with squared l2 distance < radius, or dot product > radius
        (both strict), optionally among the rows the search_filtered
        predicate keeps. Returns (lims, scores, meta): query i owns
        scores/meta[lims[i]:lims[i+1]]; inside a query the shards' results
        follow each other in shard order, each in its own order (probe
        slot, then arrival id) — not sorted by distance.

        Dot scores are the TRUE dot products, NOT negated: the negation of
        search() (quirk 2) is a kept behaviour of the reference, and this
        method has no reference behaviour to keep.

        Dist mode (one rank per shard) gathers each rank's (lims, scores,
        meta) with all_gather_object, a host path."""
        if self.dist_mode:
            from .dist import all_gather_object

            lims, scores, _ids, meta = self.sub_indexes[0].range_search(
                index_id, query, radius, filter_pos, filter_value)
            parts = all_gather_object(
                (np.asarray(lims), np.asarray(scores), list(meta)))
        else:
            def one(idx):
                lims, scores, _ids, meta = idx.range_search(
                    index_id, query, radius, filter_pos, filter_value)
                return np.asarray(lims), np.asarray(scores), list(meta)

            parts = list(self.pool.imap(one, self.sub_indexes))
        nq = query.shape[0]
        lims = np.zeros(nq + 1, dtype=np.int64)
        for pl, _s, _m in parts:
            lims[1:] += pl[1:]
        scores = np.empty(lims[nq], dtype=np.float32)
        meta: List[object] = [None] * int(lims[nq])
        for i in range(nq):
            o = int(lims[i])
            for pl, ps, pm in parts:
                a, b = int(pl[i]), int(pl[i + 1])
                scores[o:o + b - a] = ps[a:b]
                meta[o:o + b - a] = pm[a:b]
                o += b - a
        return lims, scores, meta

    def _dist_search(self, query, topk, index_id, maximize_metric,
                     return_embeddings, local_search=None):
        """One-rank-per-shard fan-out: local search -> all-gather of
        (D, I) top-k over RCCL/gloo -> k-way merge (dfann_merge_topk on
        GPU) -> metadata mapped host-side from (shard, slot). Merge
        semantics identical to _aggregate_results (incl. quirk-2 dot
        negation and FLT_MAX pads that can win); metadata rides a
        collective object gather (the reference ships it in the RPC
        responses, ref client.py:277-281). local_search: callable giving
        this rank's (scores, ids, meta, embs) in place of search_full
        (search_filtered)."""
        import torch

        from .dist import (
            all_gather_object,
            allgather_shard_topk,
            merge_gathered_full,
        )

        if local_search is not None:
            scores, ids, meta, embs = local_search()
        else:
            scores, ids, meta, embs = self.sub_indexes[0].search_full(
                index_id, query, topk, return_embeddings)
        dev = "cuda" if torch.cuda.is_available() else "cpu"
        D = torch.as_tensor(np.ascontiguousarray(scores, dtype=np.float32),
                            device=dev)
        I = torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int64),
                            device=dev)
        Dall, Iall = allgather_shard_topk(D, I)
        Dm, s_idx, j_idx, _local = merge_gathered_full(
            Dall, Iall, topk, maximize_metric)
        meta_all = all_gather_object(meta)
        nq = Dm.shape[0]
        merged_meta = [
            [meta_all[s_idx[i, j]][i][j_idx[i, j]] for j in range(topk)]
            for i in range(nq)
        ]
        if return_embeddings:
            embs_all = all_gather_object(
                np.asarray(embs, dtype=np.float32) if embs is not None else None)
            merged_embs = np.stack([
                np.stack([embs_all[s_idx[i, j]][i][j_idx[i, j]]
                          for j in range(topk)])
                for i in range(nq)
            ])
            return Dm, merged_meta, merged_embs
        return Dm, merged_meta

    def search_dev(self, qt, topk: int, index_id: str):
        """Device-resident serving step — the SAME pipeline search() uses
        in dist mode, minus the host metadata epilogue: local shard
        search -> RCCL all-gather -> on-GPU merge. Returns cuda tensors
        (D (nq,k) f32 with reference sign conventions incl. quirk-2
        negation, shard_idx (nq,k) i64, local_ids (nq,k) i64). This is
        the bench's timed region (HIP-graph capturable)."""
        from .dist import allgather_shard_topk, merge_gathered_full

        maximize_metric: bool = self.cfg.metric == "dot"
        D, I = self.sub_indexes[0].search_ids_dev(index_id, qt, topk)
        Dall, Iall = allgather_shard_topk(D, I)
        Dm, s_idx, _j, local = merge_gathered_full(
            Dall, Iall, topk, maximize_metric, device_out=True)
        return Dm, s_idx, local

    def search_with_filter(
        self,
        query: np.ndarray,
        top_k: int,
        index_id: str,
        filter_pos: int = -1,
        filter_value=None,
    ) -> Tuple[np.ndarray, List[List[object]]]:
        # reference client.py:213-263: over-fetch x3, host-side post-filter.
        # (search_filtered is the exact path: same predicate, applied inside
        # the scan kernels, full top_k at any selectivity.)
        # The over-fetch is clamped to the engine's k cap (512, see
        # include/dfann.h Limits) so a filtered search with top_k >= 171
        # degrades to a smaller candidate pool instead of raising where the
        # faiss-backed reference would succeed.
        filter_top_factor = 3
        actual_top_k = filter_top_factor * top_k if filter_pos >= 0 else top_k
        if filter_pos >= 0 and actual_top_k > 512:
            actual_top_k = max(top_k, 512)
        (scores, meta) = self.search(query, actual_top_k, index_id)
        if filter_pos < 0:
            return scores, meta

        def _do_filter(scores, results_meta):
            re_query_ids = []
            new_results = []
            new_scores = []
            for i, meta_list in enumerate(results_meta):
                sample_filtered_meta = []
                sample_filtered_scores = []
                for j, m in enumerate(meta_list):
                    if not m:
                        continue
                    if len(m) > filter_pos and m[filter_pos] != filter_value:
                        sample_filtered_meta.append(m)
                        sample_filtered_scores.append(scores[i, j])
                    if len(sample_filtered_meta) >= top_k:
                        break
                if len(sample_filtered_meta) < top_k:
                    re_query_ids.append(i)
                new_results.append(sample_filtered_meta)
                new_scores.append(
                    np.concatenate([s.reshape(-1, 1) for s in sample_filtered_scores], axis=0)
                    if sample_filtered_scores
                    else np.empty((0, 1), dtype=np.float32)
                )
            return new_scores, new_results, re_query_ids

        new_scores, new_results_meta, _re_query_ids = _do_filter(scores, meta)
        return new_scores, new_results_meta

    @staticmethod
    def _aggregate_results(
        results,
        topk: int,
        q_size: int,
        maximize_metric: bool,
        return_embeddings: bool,
    ):
        # reference client.py:265-310 restated: extend a flat metadata list,
        # re-index candidates with synthetic ids, push (-D for dot) into the
        # min-merge, map winning synthetic ids back to metadata.
        meta = []
        embs = []
        cur_idx = 0

        def to_matrix(l, n):
            return [l[i : i + n] for i in range(0, len(l), n)]

        res_heap = ResultHeap(q_size, topk)
        for DI, MetaI, e in results:
            merged_meta = list(itertools.chain(*MetaI))
            meta.extend(merged_meta)
            if return_embeddings:
                merged_embs = list(itertools.chain(*e))
                embs.extend(merged_embs)
            Ii = np.reshape(np.arange(cur_idx, cur_idx + q_size * topk), (q_size, topk))
            if maximize_metric:
                res_heap.add_result(-DI, Ii)
            else:
                res_heap.add_result(DI, Ii)
            cur_idx += q_size * topk
        res_heap.finalize()
        ids = np.reshape(res_heap.I, (-1,)).tolist()
        selected_meta = [meta[i] for i in ids]
        if return_embeddings:
            selected_embs = [embs[i] for i in ids]
        return (
            (
                res_heap.D,
                to_matrix(selected_meta, res_heap.D.shape[1]),
                to_matrix(selected_embs, res_heap.D.shape[1]),
            )
            if return_embeddings
            else (res_heap.D, to_matrix(selected_meta, res_heap.D.shape[1]))
        )

    # -- introspection / knobs --------------------------------------------

    def get_centroids(self, index_id: str):
        if self.dist_mode:
            from .dist import all_gather_object

            return all_gather_object(
                self.sub_indexes[0].get_centroids(index_id))
        return self.pool.map(lambda idx: idx.get_centroids(index_id), self.sub_indexes)

    def set_nprobe(self, index_id: str, nprobe: int):
        return self.pool.map(lambda idx: idx.set_nprobe(index_id, nprobe), self.sub_indexes)

    def set_k_factor(self, index_id: str, k_factor: float):
        return self.pool.map(
            lambda idx: idx.set_k_factor(index_id, k_factor), self.sub_indexes)

    def get_state(self, index_id: str) -> IndexState:
        if self.dist_mode:
            from .dist import all_gather_object

            states = all_gather_object(self.sub_indexes[0].get_state(index_id))
        else:
            states = self.pool.map(lambda idx: idx.get_state(index_id), self.sub_indexes)
        return IndexState.get_aggregated_states(states)

    def add_buffer_to_index(self, index_id: str):
        self.pool.map(lambda idx: idx.add_buffer_to_index(index_id), self.sub_indexes)

    def get_ntotal(self, index_id: str) -> int:
        if self.dist_mode:
            from .dist import all_gather_object

            return sum(all_gather_object(
                self.sub_indexes[0].get_ntotal(index_id)))
        return sum(self.pool.map(lambda idx: idx.get_ntotal(index_id), self.sub_indexes))

    def remove_ids(self, index_id: str, meta_ids) -> int:
        """Remove the rows whose metadata id (the key get_ids reports) is in
        `meta_ids` from every shard; returns the number of rows removed over
        all shards. The rows stop being searchable at once and their ids are
        never reused. Dist mode (one rank per shard): each rank removes from
        its own shard and the counts are combined with all_gather_object."""
        meta_ids = list(meta_ids)
        if self.dist_mode:
            from .dist import all_gather_object

            return sum(all_gather_object(
                self.sub_indexes[0].remove_by_meta_ids(index_id, meta_ids)))
        return sum(self.pool.map(
            lambda idx: idx.remove_by_meta_ids(index_id, meta_ids),
            self.sub_indexes))

    def get_ids(self, index_id: str) -> set:
        if self.dist_mode:
            from .dist import all_gather_object

            id_set_list = all_gather_object(
                self.sub_indexes[0].get_ids(index_id))
        else:
            id_set_list = self.pool.map(lambda idx: idx.get_ids(index_id), self.sub_indexes)
        return set().union(*id_set_list)

    def set_omp_num_threads(self, num_threads: int) -> None:
        self.pool.map(lambda idx: idx.set_omp_num_threads(num_threads), self.sub_indexes)

    def close(self):
        # TCP proxies own sockets; in-process servers have no close()
        for idx in self.sub_indexes:
            close_fn = idx.__dict__.get("sock") and getattr(idx, "close", None)
            if close_fn:
                close_fn()

    def get_num_servers(self):
        return self.num_shards
