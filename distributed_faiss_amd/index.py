# Shard-local index state machine.
#
# Re-implements the reference's distributed_faiss/index.py Index class
# (buffer -> train -> add -> search -> save lifecycle) on top of a pluggable
# compute engine. Behavior mirrored line-for-line where observable:
#   * add_batch buffering, fp32 cast, metadata length check, train trigger
#     at cfg.train_num              (reference index.py:138-176, quirk 10)
#   * training-data selection: first train_num rows in arrival order,
#     shuffled in place after slicing (reference index.py:194-211, quirk 6
#     — the reference shuffle uses the UNSEEDED global numpy RNG; kept)
#   * buffer drained through engine.add in cfg.buffer_bsz chunks with
#     _maybe_save after each chunk   (reference index.py:403-433)
#   * search under index_lock + metadata gather with -1 -> None
#     (reference index.py:241-270, quirk 9: ids are arrival positions)
#   * persistence layout {storage}/{index_id}/{rank}/: engine payload
#     ("index.dfann" — our own format, NOT a faiss file), meta.pkl,
#     buffer.pkl, cfg.json          (reference index.py:103-108,435-474)
#   * from_storage_dir: meta file REQUIRED and must cover ntotal; buffer
#     replay optional               (reference index.py:284-344)
#
# The engine is injected via `provider` (create(spec) / load(path)); the
# product default is the HIP/gfx950 engine (hip_engine.HipProvider), which
# raises immediately if the native library is unavailable — there is no
# silent CPU fallback. Tests inject the oracle provider.

import _thread
import logging
import os
import pickle
import threading
import time
from typing import List, Optional, Tuple, Union

import numpy as np

from .engine_spec import resolve_engine_spec
from .index_cfg import IndexCfg
from .index_state import IndexState

logger = logging.getLogger()


def get_index_files(index_storage_dir: str) -> Tuple[str, str, str, str]:
    # reference index.py:103-108 layout; engine payload renamed (our format)
    index_file = os.path.join(index_storage_dir, "index.dfann")
    meta_file = os.path.join(index_storage_dir, "meta.pkl")
    buffer_file = os.path.join(index_storage_dir, "buffer.pkl")
    cfg_file = os.path.join(index_storage_dir, "cfg.json")
    return index_file, meta_file, buffer_file, cfg_file


def _default_provider():
    from .hip_engine import HipProvider  # fails loudly if libdfann.so is absent

    return HipProvider()


class Index:
    FILTER_CACHE_SIZE = 8  # cached search_filtered bitmaps (LRU)

    def __init__(self, cfg: IndexCfg, provider=None):
        self.cfg = cfg
        self.provider = provider if provider is not None else _default_provider()
        self.embeddings_buffer = []
        self.total_data = 0
        self.id_to_metadata = []
        self.buffer_lock = threading.Lock()
        self.index_lock = threading.Lock()
        self.state = IndexState.NOT_TRAINED
        self.engine = None
        # search_filtered: (filter_pos, filter_value) -> allow-mask entry,
        # insertion-ordered LRU (guarded by _filter_lock, which is never
        # held together with index_lock)
        self._filter_cache = {}
        self._filter_lock = threading.Lock()

        self.index_save_time = time.time()
        # (ntotal, nlive) of the engine at the last save: a removal changes
        # the second and leaves the first
        self.index_saved_size = (0, 0)

        if cfg.save_interval_sec > 0:
            self._run_save_watcher()

    # -- lifecycle ---------------------------------------------------------

    def drop_index(self):
        with self.buffer_lock:
            self.embeddings_buffer = []
            self.total_data = 0
            self.id_to_metadata = []
        with self.index_lock:
            self.engine = None
            self.state = IndexState.NOT_TRAINED
        with self._filter_lock:
            self._filter_cache.clear()

    def add_batch(
        self,
        embeddings: np.ndarray,
        metadata: Optional[List[object]],
        train_async_if_triggered: bool = True,
    ):
        embeddings_num = embeddings.shape[0]
        if not metadata:
            metadata = [None] * embeddings_num
        if embeddings_num != len(metadata):
            raise RuntimeError("metadata length should match the batch size of the embeddings")

        embeddings = embeddings.astype(np.float32)  # reference index.py:151

        with self.buffer_lock:
            self.embeddings_buffer.append(embeddings)
            self.id_to_metadata.extend(metadata)
            self.total_data += embeddings_num
            total_data = self.total_data

        state = self.get_state()
        if state == IndexState.TRAINED and total_data >= 0:
            self.add_buffer_to_index()
        elif state == IndexState.NOT_TRAINED and 0 < self.cfg.train_num <= total_data:
            if train_async_if_triggered:
                _thread.start_new_thread(self.train, ())
            else:
                self.train()

    def get_idx_data_num(self) -> Tuple[int, int]:
        with self.buffer_lock:
            buf_total = self.total_data
        index_total = 0
        with self.index_lock:
            if self.engine is not None:
                # live rows: ntotal until something is removed
                index_total = self._engine_counts()[1]
        return buf_total, index_total

    def train(self) -> None:
        with self.index_lock:
            if self.state in [IndexState.TRAINING, IndexState.TRAINED, IndexState.ADD]:
                return
            self.state = IndexState.TRAINING
        cfg = self.cfg

        with self.buffer_lock:
            embeddings = self.embeddings_buffer
            dim = cfg.dim
            if dim == 0:  # guess from data (reference index.py:196-198)
                dim = embeddings[0].shape[1]
                cfg.dim = dim
            if cfg.train_num > 0:
                train_num = cfg.train_num
            elif cfg.train_ratio >= 1.0:
                train_num = self.total_data
            else:
                train_num = int(cfg.train_ratio * self.total_data)
            all_data_as_np_array = np.concatenate(embeddings, axis=0)

        train_data = all_data_as_np_array[:train_num]
        np.random.shuffle(train_data)  # unseeded, as the reference (index.py:211)
        total_data_size = all_data_as_np_array.shape[0]

        spec = resolve_engine_spec(cfg, total_data_size)
        engine = self.provider.create(spec)
        logger.info(f"Training index with array shaped {train_data.shape}")
        engine.train(train_data)

        with self.index_lock:
            self.engine = engine
            self.state = IndexState.TRAINED
        self.add_buffer_to_index()

    def add_buffer_to_index(self) -> None:
        add_to_index = False
        with self.index_lock:
            if self.state == IndexState.TRAINED:
                add_to_index = True
                self.state = IndexState.ADD
        if add_to_index:
            _thread.start_new_thread(self._add_buffer_to_idx, ())

    def search(
        self, query_batch: np.ndarray, top_k: int = 100, return_embeddings: bool = False
    ) -> Tuple[np.ndarray, List[List[object]], Optional[np.ndarray]]:
        scores, _indexes, results_meta, embs = self.search_full(
            query_batch, top_k, return_embeddings)
        return scores, results_meta, embs

    def search_full(
        self, query_batch: np.ndarray, top_k: int = 100, return_embeddings: bool = False
    ) -> Tuple[np.ndarray, np.ndarray, List[List[object]], Optional[np.ndarray]]:
        """search() plus the shard-local ids — the distributed client's
        fan-out needs ids alongside metadata so the RCCL-gathered merge
        can map winners back (ref client.py:290,297-298 does this with
        synthetic ids; here the (shard, slot) pair does it)."""
        query_batch = np.ascontiguousarray(query_batch, dtype=np.float32)
        with self.index_lock:
            if self.state != IndexState.TRAINED:
                raise RuntimeError(f"Server index is not trained. state: {self.state}")
            if return_embeddings:
                scores, indexes, embs = self.engine.search_and_reconstruct(query_batch, top_k)
            else:
                scores, indexes = self.engine.search(query_batch, top_k)
                embs = None

        return scores, indexes, self.metadata_for(indexes), embs

    def metadata_for(self, indexes: np.ndarray) -> List[List[object]]:
        """Map an (nq, k) id matrix to metadata (-1 -> None), the gather
        the reference does inline at index.py:182-191."""
        nq, n = indexes.shape
        with self.buffer_lock:
            return [
                [
                    self.id_to_metadata[indexes[i, j]] if indexes[i, j] != -1 else None
                    for j in range(n)
                ]
                for i in range(nq)
            ]

    def search_filtered(
        self, query_batch: np.ndarray, top_k: int, filter_pos: int, filter_value
    ) -> Tuple[np.ndarray, np.ndarray, List[List[object]], None]:
        """Exact top-k over the rows the reference's filter predicate keeps
        (ref client.py:213-263 `_do_filter`): metadata `m` is truthy,
        len(m) > filter_pos and m[filter_pos] != filter_value. The
        predicate becomes an allow-bitmap over arrival ids that the engine
        applies inside its scan kernels, so results are exact at any
        selectivity and `top_k` stays the engine's k. Returns
        (scores, indexes, meta, None), shaped like search_full.

        The first use of a (filter_pos, filter_value) pair evaluates the
        predicate over all ntotal metadata rows in Python — O(ntotal);
        later calls reuse the cached bitmap and only evaluate rows added
        since (ids are append-only). The cache holds the 8 most recently
        used filters; unhashable filter values are not cached."""
        query_batch = np.ascontiguousarray(query_batch, dtype=np.float32)
        while True:
            with self.index_lock:
                if self.state != IndexState.TRAINED:
                    raise RuntimeError(f"Server index is not trained. state: {self.state}")
                engine = self.engine
                if not hasattr(engine, "search_filtered"):
                    raise NotImplementedError(
                        f"engine {type(engine).__name__} has no search_filtered: "
                        "exact filtered search needs the HIP engine "
                        "(use search_with_filter for the over-fetch path)")
                ntotal = engine.ntotal
            # the bitmap is built OUTSIDE index_lock: it takes buffer_lock,
            # and _maybe_save orders buffer_lock before index_lock
            flt = self._filter_for(engine, ntotal, filter_pos, filter_value)
            with self.index_lock:
                if self.state != IndexState.TRAINED:
                    raise RuntimeError(f"Server index is not trained. state: {self.state}")
                if self.engine is engine and engine.ntotal == ntotal:
                    scores, indexes = engine.search_filtered(query_batch, top_k, flt)
                    break
            # rows were added in between: extend the bitmap and retry
        return scores, indexes, self.metadata_for(indexes), None

    def range_search(
        self, query_batch: np.ndarray, radius: float, filter_pos=None,
        filter_value=None
    ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, List[object]]:
        """faiss Index.range_search: every row of the probed lists closer
        than `radius` (l2: squared distance < radius; dot: dot product >
        radius, both strict), optionally among the rows the filter predicate
        of search_filtered keeps (filter_pos not None). Returns (lims,
        scores, indexes, meta): query i owns scores/indexes/meta
        [lims[i]:lims[i+1]], ordered by probe slot, then arrival id — not by
        distance; `meta` is a flat list aligned with `scores`."""
        query_batch = np.ascontiguousarray(query_batch, dtype=np.float32)
        while True:
            with self.index_lock:
                if self.state != IndexState.TRAINED:
                    raise RuntimeError(f"Server index is not trained. state: {self.state}")
                engine = self.engine
                if not hasattr(engine, "range_search"):
                    raise NotImplementedError(
                        f"engine {type(engine).__name__} has no range_search: "
                        "range search needs the HIP engine")
                ntotal = engine.ntotal
                if filter_pos is None:
                    lims, scores, indexes = engine.range_search(query_batch, radius)
                    break
            # as search_filtered: the bitmap is built outside index_lock
            flt = self._filter_for(engine, ntotal, filter_pos, filter_value)
            with self.index_lock:
                if self.state != IndexState.TRAINED:
                    raise RuntimeError(f"Server index is not trained. state: {self.state}")
                if self.engine is engine and engine.ntotal == ntotal:
                    lims, scores, indexes = engine.range_search(
                        query_batch, radius, flt)
                    break
            # rows were added in between: extend the bitmap and retry
        with self.buffer_lock:
            meta = [self.id_to_metadata[i] for i in indexes]
        return lims, scores, indexes, meta

    # -- removal -----------------------------------------------------------

    def remove_ids(self, ids) -> int:
        """faiss Index.remove_ids over shard-local arrival ids (the ids
        search_full returns). The rows leave the engine and their metadata
        entries become None, so get_ids, metadata_for and the filter
        predicate stop seeing them; ids are never reused. Returns the number
        of rows removed by this call."""
        ids = np.unique(np.asarray(ids, dtype=np.int64).reshape(-1))
        with self.buffer_lock, self.index_lock:
            engine = self._removable_engine()
            return self._remove_locked(engine, ids)

    def remove_by_meta_ids(self, meta_ids) -> int:
        """Remove the rows whose metadata id — meta[cfg.custom_meta_id_idx],
        the key get_ids reports — is in `meta_ids`. Rows still waiting in
        the add buffer are not in the engine yet and are left alone."""
        wanted = set(meta_ids)
        id_idx = self.cfg.custom_meta_id_idx
        with self.buffer_lock, self.index_lock:
            engine = self._removable_engine()
            ids = np.fromiter(
                (i for i, m in enumerate(self.id_to_metadata[:engine.ntotal])
                 if m and m[id_idx] in wanted), dtype=np.int64)
            return self._remove_locked(engine, ids)

    def _removable_engine(self):
        # caller holds index_lock
        if self.state != IndexState.TRAINED:
            raise RuntimeError(f"Server index is not trained. state: {self.state}")
        if not hasattr(self.engine, "remove_ids"):
            raise NotImplementedError(
                f"engine {type(self.engine).__name__} has no remove_ids: "
                "removal needs the HIP engine")
        return self.engine

    def _remove_locked(self, engine, ids) -> int:
        # caller holds buffer_lock and index_lock
        if ids.size == 0:
            return 0
        removed = int(engine.remove_ids(ids))
        for i in ids:
            self.id_to_metadata[i] = None
        return removed

    def _engine_counts(self) -> Tuple[int, int]:
        # (ntotal, nlive); an engine without removal stores all it issued
        ntotal = self.engine.ntotal
        return ntotal, getattr(self.engine, "nlive", ntotal)

    @staticmethod
    def _filter_allows(m, filter_pos, filter_value) -> bool:
        # the reference predicate, ref client.py:236-240
        return bool(m) and len(m) > filter_pos and m[filter_pos] != filter_value

    def _filter_for(self, engine, ntotal, filter_pos, filter_value):
        """Allow-mask over ids [0, ntotal): cached per (filter_pos,
        filter_value), extended by the tail when ntotal has grown, and
        uploaded once per change when the engine can keep it
        device-resident (pack_filter)."""
        with self._filter_lock:
            return self._filter_for_locked(engine, ntotal, filter_pos, filter_value)

    def _filter_for_locked(self, engine, ntotal, filter_pos, filter_value):
        try:
            key = (filter_pos, filter_value)
            hash(key)
        except TypeError:
            key = None
        entry = self._filter_cache.pop(key, None) if key is not None else None
        if entry is None or entry["n"] > ntotal or entry["engine"] is not engine:
            entry = {"n": 0, "allow": np.zeros(0, dtype=bool), "packed": None,
                     "engine": engine}
        if entry["n"] < ntotal:
            with self.buffer_lock:
                tail = np.fromiter(
                    (self._filter_allows(m, filter_pos, filter_value)
                     for m in self.id_to_metadata[entry["n"]:ntotal]),
                    dtype=bool, count=ntotal - entry["n"])
            entry["allow"] = np.concatenate([entry["allow"], tail])
            entry["n"] = ntotal
            entry["packed"] = None
        if entry["packed"] is None:
            pack = getattr(engine, "pack_filter", None)
            entry["packed"] = pack(entry["allow"]) if pack else entry["allow"]
        if key is not None:
            self._filter_cache[key] = entry  # most recently used last
            while len(self._filter_cache) > self.FILTER_CACHE_SIZE:
                self._filter_cache.pop(next(iter(self._filter_cache)))
        return entry["packed"]

    def search_ids_dev(self, qt, top_k: int):
        """Device-resident search: (D, I) stay in HBM (torch cuda
        tensors). Serving-step hot path for the distributed client — no
        metadata epilogue, no D2H. HIP engine only."""
        with self.index_lock:
            if self.state != IndexState.TRAINED:
                raise RuntimeError(f"Server index is not trained. state: {self.state}")
            return self.engine.search_dev(qt, top_k)

    # -- persistence -------------------------------------------------------

    def save(self) -> bool:
        state = self.get_state()
        if state == IndexState.TRAINED:
            return self._maybe_save(ignore_time=True)
        elif state == IndexState.ADD:
            self.index_save_time = 0  # trigger save when the add drain finishes
        else:
            return False

    @classmethod
    def from_storage_dir(
        cls,
        index_storage_dir: str,
        cfg: IndexCfg = None,
        ignore_buffer: bool = True,
        provider=None,
    ) -> Union[None, "Index"]:
        index_file, meta_file, buffer_file, cfg_file = get_index_files(index_storage_dir)
        if not os.path.exists(index_file):
            return None

        if provider is None:
            provider = _default_provider()
        engine = provider.load(index_file)

        if os.path.exists(meta_file):
            with open(meta_file, "rb") as reader:
                meta = pickle.load(reader)
            assert (
                len(meta) >= engine.ntotal
            ), "Deserialized meta list should be at least of index size"
        else:
            raise RuntimeError("no meta file found. Can't use index.")

        buffer = []
        if (not ignore_buffer) and buffer_file and os.path.exists(buffer_file):
            with open(buffer_file, "rb") as reader:
                buffer = pickle.load(reader)

        if cfg is None:
            if os.path.isfile(cfg_file):
                cfg = IndexCfg.from_json(cfg_file)
            else:
                cfg = IndexCfg()

        buffer_size = sum(v.shape[0] for v in buffer)
        result = cls(cfg, provider=provider)
        result.engine = engine
        result.state = IndexState.TRAINED
        result.upd_cfg(cfg)

        if len(meta) == engine.ntotal + buffer_size:
            result.id_to_metadata = meta
            result.embeddings_buffer = buffer
            result.total_data = buffer_size
            if buffer_size > 0:
                result.add_buffer_to_index()
        else:
            logger.warning(
                "Metadata size doesn't match combined index+buffer size: "
                "ignoring buffer, reducing metadata to index size"
            )
            result.id_to_metadata = meta[: engine.ntotal]
        return result

    # -- knobs / introspection --------------------------------------------

    def get_centroids(self):
        with self.index_lock:
            if self.state != IndexState.TRAINED:
                raise RuntimeError("Server index is not trained")
            return self.engine.get_centroids()

    def set_nprobe(self, nprobe: int):
        self.cfg.nprobe = nprobe
        with self.index_lock:
            if self.engine is not None:
                self.engine.nprobe = nprobe

    def set_k_factor(self, k_factor: float):
        """Refine stage: re-rank ceil(top_k * k_factor) base candidates
        (faiss IndexRefine.k_factor). The engine raises RuntimeError when
        the index has no refine stage."""
        with self.index_lock:
            if self.engine is None:
                raise RuntimeError("set_k_factor: index is not built yet")
            self.engine.k_factor = k_factor
        self.cfg.extra["k_factor"] = float(k_factor)

    def get_state(self):
        with self.index_lock:
            return self.state

    def get_ids(self):
        id_idx = self.cfg.custom_meta_id_idx
        r = {meta[id_idx] for meta in self.id_to_metadata if meta}
        return r

    def upd_cfg(self, cfg: IndexCfg):
        self.cfg = cfg
        self._override_nprobe(cfg)

    # -- internals ---------------------------------------------------------

    def _add_buffer_to_idx(self):
        while True:
            bsz = self.cfg.buffer_bsz
            embeddings_to_add = []
            embeddings_to_add_total = 0
            with self.buffer_lock:
                for e in self.embeddings_buffer:
                    embeddings_to_add.append(e)
                    embeddings_to_add_total += e.shape[0]
                    if embeddings_to_add_total >= bsz:
                        break
                if embeddings_to_add_total > 0:
                    # (the reference mutates the buffer OUTSIDE the lock,
                    #  index.py:417-419; we keep it inside — same observable
                    #  behavior, fewer races)
                    self.embeddings_buffer = self.embeddings_buffer[len(embeddings_to_add):]
                    self.total_data -= embeddings_to_add_total

            if embeddings_to_add_total == 0:
                break
            add_data_as_np = np.concatenate(embeddings_to_add, axis=0)
            self.engine.add(add_data_as_np)
            self._maybe_save(ignore_time=False)

        with self.index_lock:
            self.state = IndexState.TRAINED

    def _maybe_save(self, ignore_time: bool = False) -> bool:
        if not ignore_time:
            if self.cfg.save_interval_sec <= 0:
                return False
            if time.time() - self.index_save_time < self.cfg.save_interval_sec:
                return False

        with self.buffer_lock, self.index_lock:
            if self._engine_counts() == self.index_saved_size:
                return False
            index_storage_dir = self.cfg.index_storage_dir
            index_file, meta_file, buffer_file, cfg_file = get_index_files(index_storage_dir)
            os.makedirs(index_storage_dir, exist_ok=True)
            self.engine.save(index_file)
            with open(meta_file, mode="wb") as f:
                pickle.dump(self.id_to_metadata, f)
            with open(buffer_file, mode="wb") as f:
                pickle.dump(self.embeddings_buffer, f)
            with open(cfg_file, mode="w") as f:
                f.write(self.cfg.to_json_string() + "\n")
            self.index_saved_size = self._engine_counts()
            self.index_save_time = time.time()
            return True

    def _run_save_watcher(self):
        def _save(idx: "Index"):
            while True:
                time.sleep(idx.cfg.save_interval_sec)
                idx._maybe_save(ignore_time=False)

        _thread.start_new_thread(_save, (self,))

    def _override_nprobe(self, cfg: IndexCfg):
        if self.engine is not None:
            self.engine.nprobe = cfg.nprobe

    @staticmethod
    def infer_n_centroids(total_data_size):
        from .engine_spec import infer_n_centroids

        return infer_n_centroids(total_data_size)
