# ORACLE — hnswsq tier: numpy restatement of csrc/hnsw.hip and of the host
# orchestration in csrc/dfann.hip (hnsw_draw_level, hnsw_add,
# hnsw_apply_reqs). TEST INFRASTRUCTURE ONLY (oracle/__init__.py).
#
# Both sides are restated op-for-op:
#   * SEARCH (OracleHNSWSearch): k_hnsw_search over any graph dict of the
#     hnsw_dump() layout — the 8-lane partial sums + fixed butterfly of the
#     distance, the 16384-slot visited hash with probe cap 64, the Sel
#     frontier (threshold-filtered append, compaction to the top-ef, the
#     headroom compaction of sel_guard) and the greedy argmin ties.
#   * BUILD (OracleHNSWBuild): level draws, the wave schedule, k_hnsw_insert
#     over the frozen snapshot, the (dst, level, src)-sorted reverse-link
#     merge of k_hnsw_apply with its fast path, its over-cap prune and its
#     truncation of a run to 1024 candidates, the entry update and the
#     refine pass. The graph it produces equals the engine's dump bit for
#     bit (tests/test_gpu_hnsw_build.py), stale slots past the live counts
#     included, because the in-place writes are mimicked.
#
# The scalar _dist_q / _dist_cc are the DEFINITION of the two distances;
# the row-batched forms compute the same bits (tests/test_oracle_hnsw.py)
# and are what the traversals call.

import math

import numpy as np

HNSW_HASH = 16384
HNSW_PROBES = 64
HNSW_MAXL = 8
HNSW_WMAX = 4096      # widest insertion / refine wave
HNSW_APPLY_CAP = 1024  # candidates one k_hnsw_apply run can hold
SEL_CAP = 1024
_NG = 32              # 256 threads / 8 lanes: neighbours per pass
_FLAG = 0x80000000
_PAD_POS = 0xFFFFFFFF
_FLT_MAX = np.float32(3.402823466e+38)
_MASK64 = (1 << 64) - 1
_LANE = np.arange(8)


# ---------------------------------------------------------------------------
# host arithmetic of the build
# ---------------------------------------------------------------------------


def _splitmix64_next(x):
    x = (x + 0x9E3779B97F4A7C15) & _MASK64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def hnsw_level_real(seed, ident, M):
    """-log(u)/log(M) before floor and clamp (hnsw_draw_level restated).

    seed ^ (id*0x9E3779B97F4A7C15 + 0x51ED2701) in wrapping 64-bit
    arithmetic seeds splitmix64; one draw gives u in (0, 1].
    """
    s = (seed ^ ((ident * 0x9E3779B97F4A7C15 + 0x51ED2701) & _MASK64)) & _MASK64
    z = _splitmix64_next(s)
    u = (float(z >> 11) + 1.0) * (1.0 / 9007199254740992.0)
    mL = 1.0 / math.log(float(M))
    return -math.log(u) * mL


def hnsw_draw_level(seed, ident, M):
    l = int(math.floor(hnsw_level_real(seed, ident, M)))
    return max(0, min(HNSW_MAXL, l))


def hnsw_wave_schedule(n0, n):
    """Insertion wave sizes of one add of n rows onto n0 existing rows."""
    ntot = n0 + n
    out = []
    w0 = n0
    while w0 < ntot:
        W = 1 if w0 == 0 else min(HNSW_WMAX, max(256, w0 // 8), ntot - w0)
        out.append(W)
        w0 += W
    return out


def _empty_graph(M, efc):
    return {
        "levels": np.zeros(0, dtype=np.int32),
        "cnt0": np.zeros(0, dtype=np.int32),
        "nbr0": np.full((0, 2 * M), -1, dtype=np.int32),
        "upslot": np.zeros(0, dtype=np.int32),
        "cntU": np.zeros((1, HNSW_MAXL), dtype=np.int32),
        "nbrU": np.full((1, HNSW_MAXL, M), -1, dtype=np.int32),
        "M": M, "deg0": 2 * M, "nslots": 0, "entry": -1, "maxlevel": -1,
        "efc": efc,
    }


# ---------------------------------------------------------------------------
# distances
# ---------------------------------------------------------------------------


class _HNSWDist:
    """hnsw_dist_q / hnsw_dist_cc over (n, d) uint8 codes and scale (d,).

    Lane g8 covers bytes [16*g8, 16*g8+16) and then strides by 128; within
    a lane the sum is sequential (separate multiply and add); the 8
    partials combine by the xor-butterfly 4, 2, 1.
    """

    def _set_codes(self, codes):
        self.codes = np.ascontiguousarray(codes, dtype=np.uint8)
        n = self.codes.shape[0]
        self._npass = max(1, (self.d + 127) // 128)
        dp = 128 * self._npass
        # zero padding: a padded term is (0 - 0*0)^2 = +0, and part + (+0)
        # leaves a non-negative part unchanged — the same bits as the
        # kernel's `t0 + b < d` guard skipping the term
        self._cf = np.zeros((n, dp), dtype=np.float32)
        self._cf[:, : self.d] = self.codes
        self._sp = np.zeros(dp, dtype=np.float32)
        self._sp[: self.d] = self.scale
        self._cc_rows_memo = {}

    # -- scalar definitions ------------------------------------------------

    @staticmethod
    def _butterfly(parts):
        b1 = np.array([np.float32(parts[i] + parts[i ^ 4]) for i in range(8)],
                      dtype=np.float32)
        b2 = np.array([np.float32(b1[i] + b1[i ^ 2]) for i in range(8)],
                      dtype=np.float32)
        return np.float32(b2[0] + b2[1])

    def _dist_q(self, u, cid):
        d = self.d
        s = self.scale
        row = self.codes[cid]
        parts = np.zeros(8, dtype=np.float32)
        for g8 in range(8):
            acc = np.float32(0.0)
            t0 = g8 * 16
            while t0 < d:
                for b in range(16):
                    t = t0 + b
                    if t < d:
                        diff = np.float32(u[t] - np.float32(row[t]) * s[t])
                        acc = np.float32(acc + np.float32(diff * diff))
                t0 += 128
            parts[g8] = acc
        return self._butterfly(parts)

    def _dist_cc(self, id1, id2):
        d = self.d
        s = self.scale
        r1 = self.codes[id1]
        r2 = self.codes[id2]
        parts = np.zeros(8, dtype=np.float32)
        for g8 in range(8):
            acc = np.float32(0.0)
            t0 = g8 * 16
            while t0 < d:
                for b in range(16):
                    t = t0 + b
                    if t < d:
                        diff = np.float32(
                            np.float32(np.float32(r1[t]) - np.float32(r2[t])) * s[t])
                        acc = np.float32(acc + np.float32(diff * diff))
                t0 += 128
            parts[g8] = acc
        return self._butterfly(parts)

    # -- row-batched forms (same bits) ---------------------------------------

    def _lanes_reduce(self, sq):
        # sq: (rows, 128*npass) per-dim squared terms, t = 128*pass + 16*g8 + b
        rows = sq.shape[0]
        sq = sq.reshape(rows, self._npass, 8, 16)
        part = np.zeros((rows, 8), dtype=np.float32)
        for ps in range(self._npass):
            for b in range(16):
                part = part + sq[:, ps, :, b]
        part = part + part[:, _LANE ^ 4]
        part = part + part[:, _LANE ^ 2]
        part = part + part[:, _LANE ^ 1]
        return part[:, 0]

    def _dist_q_rows(self, u, ids):
        ids = np.asarray(ids, dtype=np.int64)
        up = np.zeros(self._sp.shape[0], dtype=np.float32)
        up[: self.d] = u
        diff = up[None, :] - self._cf[ids] * self._sp[None, :]
        return self._lanes_reduce(diff * diff)

    def _dist_cc_rows(self, ident, ids):
        ids = np.asarray(ids, dtype=np.int64)
        diff = (self._cf[ident][None, :] - self._cf[ids]) * self._sp[None, :]
        return self._lanes_reduce(diff * diff)

    def _cc_all(self, ident):
        """dist_cc(ident, every stored row), computed once per code set."""
        r = self._cc_rows_memo.get(ident)
        if r is None:
            r = self._dist_cc_rows(ident, np.arange(self._cf.shape[0]))
            self._cc_rows_memo[ident] = r
        return r


class _QDist:
    """dist_q(u, id) memo for one query / inserted point: every traversal
    evaluates the same pure function of (u, id), so each id is computed
    once, in row batches."""

    def __init__(self, owner, u):
        self.o = owner
        self.u = u
        n = owner._cf.shape[0]
        self.val = np.zeros(n, dtype=np.float32)
        self.have = np.zeros(n, dtype=bool)

    def get(self, ids):
        ids = np.asarray(ids, dtype=np.int64)
        miss = ids[~self.have[ids]]
        if miss.size:
            miss = np.unique(miss)
            self.val[miss] = self.o._dist_q_rows(self.u, miss)
            self.have[miss] = True
        return self.val[ids]

    def one(self, ident):
        return self.get(np.array([ident]))[0]


# ---------------------------------------------------------------------------
# Sel frontier + visited hash
# ---------------------------------------------------------------------------


class _Sel:
    """kernels.hip Sel as used by hnsw_beam: an append is kept only if it
    sorts before the threshold (dist, id|flag) recorded by the last
    compaction that filled k entries; a compaction sorts by (dist,
    id|flag) and truncates to k."""

    def __init__(self, counters):
        self.d = np.zeros(0, dtype=np.float32)
        self.p = np.zeros(0, dtype=np.int64)
        self.thrD = _FLT_MAX
        self.thrP = _PAD_POS
        self.c = counters

    @property
    def cnt(self):
        return self.d.shape[0]

    def try_many(self, dist, ids):
        dist = np.asarray(dist, dtype=np.float32)
        ids = np.asarray(ids, dtype=np.int64)
        keep = (dist < self.thrD) | ((dist == self.thrD) & (ids < self.thrP))
        if keep.any():
            self.d = np.concatenate([self.d, dist[keep]])
            self.p = np.concatenate([self.p, ids[keep]])
        assert self.cnt <= SEL_CAP

    def compact(self, k):
        order = np.lexsort((self.p, self.d))
        if order.shape[0] > k:
            self.c["sel_truncations"] += 1
            order = order[:k]
        self.d = self.d[order]
        self.p = self.p[order]
        if self.cnt >= k:
            self.thrD = self.d[k - 1]
            self.thrP = int(self.p[k - 1])


class _Visited:
    """The LDS visited table: open addressing, id+1 stored, 0 = empty; an
    id whose 64-slot probe window is full counts as visited."""

    def __init__(self):
        self.tab = {}

    @staticmethod
    def _hash(ident):
        x = (ident * 0x9E3779B9) & 0xFFFFFFFF
        x ^= x >> 16
        return x & (HNSW_HASH - 1)

    def insert(self, ident):
        h = self._hash(ident)
        tab = self.tab
        for p in range(HNSW_PROBES):
            slot = (h + p) & (HNSW_HASH - 1)
            v = tab.get(slot, 0)
            if v == ident + 1:
                return True
            if v == 0:
                tab[slot] = ident + 1
                return False
        return True


class _HNSWTraverse(_HNSWDist):
    """hnsw_greedy + hnsw_beam over a graph dict (hnsw_dump layout)."""

    @staticmethod
    def _nbrs(g, node, level):
        if level == 0:
            c = int(g["cnt0"][node])
            return g["nbr0"][node, :c]
        slot = int(g["upslot"][node])
        c = int(g["cntU"][slot, level - 1])
        return g["nbrU"][slot, level - 1, :c]

    def _greedy(self, g, qd, cur, cur_d, level, self_id=-1):
        # per-group minima over passes, then over groups, both with the
        # (dist, lower id) order: the lexicographic minimum
        while True:
            nb = self._nbrs(g, cur, level).astype(np.int64)
            nb = nb[nb != self_id]
            if nb.size == 0:
                return cur, cur_d
            dd = qd.get(nb)
            j = np.lexsort((nb, dd))[0]
            if dd[j] < cur_d:
                cur, cur_d = int(nb[j]), dd[j]
            else:
                return cur, cur_d

    def _beam(self, g, qd, entry, entry_d, level, ef, self_id=-1):
        """Returns the compacted Sel: (dist, id) arrays sorted by
        (dist, id|flag), at most ef entries, flags stripped."""
        c = self.counters
        vis = _Visited()
        sel = _Sel(c)
        vis.insert(entry)
        sel.try_many([entry_d], [entry])
        sel.compact(ef)
        while True:
            free = np.flatnonzero(sel.p < _FLAG)
            if free.size == 0:
                break
            pick = int(free[0])
            cur = int(sel.p[pick])
            sel.p[pick] |= _FLAG
            nb = self._nbrs(g, cur, level).astype(np.int64)
            cnt = nb.shape[0]
            if cnt == 0:
                sel.compact(ef)
                continue
            c["max_frontier_plus_degree"] = max(
                c["max_frontier_plus_degree"], sel.cnt + cnt)
            dd = qd.get(nb)
            # sel_guard compacts before a pass when fewer than 32 slots are
            # left; while that cannot happen the passes of one expansion
            # are order-invariant and are appended at once
            last0 = ((cnt - 1) // _NG) * _NG
            step = cnt if sel.cnt + last0 <= SEL_CAP - _NG else _NG
            for c0 in range(0, cnt, step):
                if sel.cnt > SEL_CAP - _NG:
                    c["sel_guard_compacts"] += 1
                    sel.compact(ef)
                ids = nb[c0:c0 + step]
                fresh = np.fromiter(
                    (i != self_id and not vis.insert(i) for i in ids.tolist()),
                    dtype=bool, count=ids.shape[0])
                if fresh.any():
                    sel.try_many(dd[c0:c0 + step][fresh], ids[fresh])
            sel.compact(ef)
        return sel.d, sel.p & (_FLAG - 1)


# ---------------------------------------------------------------------------
# search
# ---------------------------------------------------------------------------


class OracleHNSWSearch(_HNSWTraverse):
    def __init__(self, d, graph, vmin, vdiff, codes):
        self.d = d
        self.g = graph  # dict of the hnsw_dump layout
        self.vmin = vmin.astype(np.float32)
        self.vdiff = vdiff.astype(np.float32)
        self.scale = (self.vdiff / np.float32(255.0)).astype(np.float32)
        self._set_codes(codes)
        self.counters = {"sel_truncations": 0, "sel_guard_compacts": 0,
                         "max_frontier_plus_degree": 0}

    @staticmethod
    def encode(x, vmin, vdiff):
        """k_sq_encode restated (trunc toward zero, f32 ops)."""
        x = x.astype(np.float32)
        xi = (x - vmin[None, :].astype(np.float32)) / vdiff[None, :].astype(np.float32)
        c = (np.float32(255.0) * xi).astype(np.int32)  # trunc toward zero
        return np.clip(c, 0, 255).astype(np.uint8)

    def search(self, q, k, ef):
        """ef is the engine's nprobe: clamped to [k, 512] as hnsw_search does."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        nq = q.shape[0]
        ef = min(max(ef, k), 512)
        g = self.g
        D = np.full((nq, k), _FLT_MAX, dtype=np.float32)
        I = np.full((nq, k), -1, dtype=np.int64)
        for qi in range(nq):
            u = ((q[qi] - self.vmin) - np.float32(0.5) * self.scale).astype(np.float32)
            qd = _QDist(self, u)
            cur = int(g["entry"])
            cur_d = qd.one(cur)
            for l in range(int(g["maxlevel"]), 0, -1):
                cur, cur_d = self._greedy(g, qd, cur, cur_d, l)
            rd, ri = self._beam(g, qd, cur, cur_d, 0, ef)
            m = min(k, rd.shape[0])
            D[qi, :m] = rd[:m]
            I[qi, :m] = ri[:m]
        return D, I


# ---------------------------------------------------------------------------
# build
# ---------------------------------------------------------------------------


class OracleHNSWBuild(_HNSWTraverse):
    """hnsw_add restated. add(x) may be called repeatedly; dump() returns
    the dict HipEngine.hnsw_dump() returns.

    counters: fast_path_runs, over_cap_runs, truncated_runs (a run cut to
    1024 candidates), dedup_hits (a proposed link dropped because the row
    or the kept set already holds it), entry_changes, level_at_clamp (nodes
    at level 8), level_clamped (those whose draw was above 8 and was cut),
    shrink_rejections (insert side), apply_shrink_rejections (merge side),
    sel_truncations (a compaction that cut the frontier to ef),
    sel_guard_compacts (the headroom compaction inside an expansion),
    max_frontier_plus_degree (largest frontier size + degree met when a
    node was expanded).
    """

    def __init__(self, d, M, efc, seed, vmin, vdiff, refine=1):
        if M < 2 or M > 256:
            raise ValueError("hnswsq needs 2 <= M <= 256")
        self.d = int(d)
        self.M = int(M)
        self.deg0 = 2 * self.M
        self.efc = min(max(int(efc), 1), 512)
        self.seed = int(seed)
        self.refine = int(refine)
        self.vmin = np.asarray(vmin, dtype=np.float32)
        self.vdiff = np.asarray(vdiff, dtype=np.float32)
        self.scale = (self.vdiff / np.float32(255.0)).astype(np.float32)
        self.g = _empty_graph(self.M, self.efc)
        self.ntotal = 0
        self._set_codes(np.zeros((0, self.d), dtype=np.uint8))
        self.counters = {k: 0 for k in (
            "fast_path_runs", "over_cap_runs", "truncated_runs", "dedup_hits",
            "entry_changes", "level_clamped", "level_at_clamp", "shrink_rejections",
            "apply_shrink_rejections", "sel_truncations", "sel_guard_compacts",
            "max_frontier_plus_degree")}
        self.waves = []  # wave sizes of every add, in order

    # -- public ----------------------------------------------------------------

    def dump(self):
        g = self.g
        out = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in g.items()}
        return out

    def add(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = x.shape[0]
        if n == 0:
            return
        g = self.g
        M, deg0 = self.M, self.deg0
        n0, ntot = self.ntotal, self.ntotal + n
        # 1) encode every new row first (ids are row positions)
        codes = OracleHNSWSearch.encode(x, self.vmin, self.vdiff)
        self._set_codes(np.concatenate([self.codes, codes], axis=0))
        U = ((x - self.vmin[None, :]) - np.float32(0.5) * self.scale[None, :]
             ).astype(np.float32)
        # 2) levels + upper slots in arrival order
        levels = np.zeros(n, dtype=np.int32)
        upslot = np.full(n, -1, dtype=np.int32)
        nslots = int(g["nslots"])
        for i in range(n):
            real = hnsw_level_real(self.seed, n0 + i, M)
            lv = max(0, min(HNSW_MAXL, int(math.floor(real))))
            if real >= HNSW_MAXL + 1:
                self.counters["level_clamped"] += 1
            if lv == HNSW_MAXL:
                self.counters["level_at_clamp"] += 1
            levels[i] = lv
            if lv > 0:
                upslot[i] = nslots
                nslots += 1
        # 3) grow the arrays: fresh adjacency is -1, fresh counts 0
        g["levels"] = np.concatenate([g["levels"], levels])
        g["upslot"] = np.concatenate([g["upslot"], upslot])
        g["cnt0"] = np.concatenate([g["cnt0"], np.zeros(n, dtype=np.int32)])
        g["nbr0"] = np.concatenate(
            [g["nbr0"], np.full((n, deg0), -1, dtype=np.int32)])
        if nslots > g["nslots"]:
            old = int(g["nslots"])
            cntU = np.zeros((nslots, HNSW_MAXL), dtype=np.int32)
            nbrU = np.full((nslots, HNSW_MAXL, M), -1, dtype=np.int32)
            cntU[:old] = g["cntU"][:old]
            nbrU[:old] = g["nbrU"][:old]
            g["cntU"], g["nbrU"], g["nslots"] = cntU, nbrU, nslots
        # 4) wave insertion over frozen snapshots
        w0 = n0
        for W in hnsw_wave_schedule(n0, n):
            self.waves.append(W)
            if g["entry"] < 0:  # very first point
                g["entry"] = 0
                g["maxlevel"] = int(g["levels"][0])
            reqs = []
            for p in range(w0, w0 + W):
                self._insert(g, p, U[p - n0], w0, reqs, refine=False)
            self._apply(reqs)
            self._entry_update(g, w0, W)
            w0 += W
        self.ntotal = ntot
        # 5) refine: the rows of this add, over a copy frozen before the pass
        if self.refine:
            frozen = dict(g)
            for k in ("cnt0", "nbr0", "cntU", "nbrU"):
                frozen[k] = g[k].copy()
            r0 = n0
            while r0 < ntot:
                W = min(HNSW_WMAX, ntot - r0)
                reqs = []
                for p in range(r0, r0 + W):
                    self._insert(frozen, p, U[p - n0], ntot, reqs, refine=True)
                self._apply(reqs)
                r0 += W

    # -- the decisions the parity tests pin, one small method each -----------

    _apply_limit = HNSW_APPLY_CAP

    @staticmethod
    def _closer(cc, dd):
        # shrink test: some kept kc has dist_cc(c, kc) < dist(p or dst, c)
        return bool((cc < dd).any())

    def _insert_cap(self, level):
        return self.M  # M links at every level during insert

    @staticmethod
    def _apply_order(cid, cdist):
        return np.lexsort((cid, cdist))  # (dist, lower id first)

    def _entry_update(self, g, w0, W):
        # highest new level beats the old entry; lowest id on ties
        for i in range(w0, w0 + W):
            if g["levels"][i] > g["maxlevel"]:
                g["maxlevel"] = int(g["levels"][i])
                g["entry"] = i
                self.counters["entry_changes"] += 1

    # -- k_hnsw_insert -----------------------------------------------------------

    def _insert(self, g, p, u, n_snap, reqs, refine):
        live = self.g
        M = self.M
        entry, entry_level = int(live["entry"]), int(live["maxlevel"])
        plevel = int(live["levels"][p])
        if n_snap == 0:
            return  # first point: no links
        self_id = p if refine else -1
        if refine and entry == p:
            return
        qd = _QDist(self, u)
        cur = entry
        cur_d = qd.one(cur)
        for l in range(entry_level, plevel, -1):
            cur, cur_d = self._greedy(g, qd, cur, cur_d, l, self_id)
        for l in range(min(plevel, entry_level), -1, -1):
            rd, ri = self._beam(g, qd, cur, cur_d, l, self.efc, self_id)
            # shrink: keep c unless a kept kc is closer to c than p is
            kept, kept_d = [], []
            for ci in range(rd.shape[0]):
                if len(kept) >= self._insert_cap(l):
                    break
                cid, cdist = int(ri[ci]), rd[ci]
                if kept and self._closer(self._cc_all(cid)[kept], cdist):
                    self.counters["shrink_rejections"] += 1
                    continue
                kept.append(cid)
                kept_d.append(cdist)
            if kept:
                if not refine:
                    if l == 0:
                        live["cnt0"][p] = len(kept)
                        live["nbr0"][p, :len(kept)] = kept
                    else:
                        slot = int(live["upslot"][p])
                        live["cntU"][slot, l - 1] = len(kept)
                        live["nbrU"][slot, l - 1, :len(kept)] = kept
                    for c in kept:
                        reqs.append((c, l, p))
                else:
                    for c in kept:
                        reqs.append((c, l, p))
                        reqs.append((p, l, c))
            if rd.shape[0] > 0:
                cur, cur_d = int(ri[0]), rd[0]

    # -- hnsw_apply_reqs + k_hnsw_apply ------------------------------------------

    def _apply(self, reqs):
        if not reqs:
            return
        g = self.g
        reqs = sorted(reqs)  # (dst, level, src)
        i = 0
        while i < len(reqs):
            j = i
            while j < len(reqs) and reqs[j][:2] == reqs[i][:2]:
                j += 1
            dst, lvl = reqs[i][0], reqs[i][1]
            self._apply_run(g, dst, lvl, [r[2] for r in reqs[i:j]])
            i = j

    def _apply_run(self, g, dst, lvl, srcs):
        c = self.counters
        if lvl == 0:
            cap = self.deg0
            row = g["nbr0"][dst]
            cnt_arr, cnt_idx = g["cnt0"], dst
        else:
            cap = self.M
            slot = int(g["upslot"][dst])
            row = g["nbrU"][slot, lvl - 1]
            cnt_arr, cnt_idx = g["cntU"], (slot, lvl - 1)
        old_cnt = int(cnt_arr[cnt_idx])
        inc = len(srcs)
        if old_cnt + inc <= cap:
            c["fast_path_runs"] += 1
            w = old_cnt
            for src in srcs:
                if (row[:w] == src).any():
                    c["dedup_hits"] += 1
                else:
                    row[w] = src
                    w += 1
            cnt_arr[cnt_idx] = w
            return
        c["over_cap_runs"] += 1
        total = old_cnt + inc
        if total > self._apply_limit:
            # only the first 1024 candidates fit: the existing links, then
            # the incoming sources in ascending id; the rest are dropped
            total = self._apply_limit
            c["truncated_runs"] += 1
        cid = np.concatenate([row[:old_cnt].astype(np.int64),
                              np.asarray(srcs, dtype=np.int64)])[:total]
        cdist = self._cc_all(dst)[cid]
        order = self._apply_order(cid, cdist)
        kept = []
        for ci in order:
            if len(kept) >= cap:
                break
            ident, dd = int(cid[ci]), cdist[ci]
            if ident in kept:
                c["dedup_hits"] += 1
                continue
            if kept and self._closer(self._cc_all(ident)[kept], dd):
                c["apply_shrink_rejections"] += 1
                continue
            kept.append(ident)
        # only the first n_kept slots are rewritten: later slots keep what
        # they held
        cnt_arr[cnt_idx] = len(kept)
        row[:len(kept)] = kept
