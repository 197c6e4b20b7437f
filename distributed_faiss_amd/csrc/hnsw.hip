// dfann — HNSW-over-SQ8 for gfx950 (the reference's "hnswsq" builder,
// distributed_faiss/index.py:51-60: faiss.IndexHNSWSQ(dim, QT_8bit,
// store_n) with efSearch = cfg.nprobe, efConstruction from cfg.extra;
// L2 only — the reference asserts it).
//
// MI355X-native design (not a port of faiss's sequential insertion):
//  * codes: NON-residual SQ8 rows in a slab arena (no coarse quantizer);
//    asymmetric distance dist(q, code) = sum_t (u[t] - c*s[t])^2 with
//    u = (q - vmin) - 0.5*scale — the FAM2 folded algebra with cent = 0,
//    8-lane rows + fixed 3-step butterfly (bitwise-defined order, shared
//    with the oracle). Symmetric (code,code) distance decodes to
//    ((c1-c2)*scale)^2 per dim.
//  * build: BATCHED wave insertion — wave w inserts its points in
//    parallel over a frozen snapshot of the graph after wave w-1 (one
//    block per point), then reverse links are applied in (dst, level,
//    src) SORTED order — the whole build is DETERMINISTIC given (data,
//    seed, wave schedule), unlike an atomics-ordered build, and is
//    restated op-for-op by the oracle (oracle/hnsw.py: the graph is
//    pinned bit for bit). Differs from faiss's strictly sequential
//    insertion (documented deviation; graph quality is gated by recall
//    property tests).
//  * beam search: the Sel threshold+bitonic machinery keeps the top-ef
//    frontier; expanded entries are flagged in bit 31 of the packed id;
//    the visited set is a 16384-slot open-addressing hash in LDS
//    (HNSW_HASH; probe cap 64, HNSW_PROBES; a full cluster treats the id
//    as visited — a deterministic, oracle-replicable approximation).
//  * levels: splitmix64(seed ^ id) -> geometric with mL = 1/ln(M),
//    clamped to HNSW_MAXL. Level-0 degree cap 2M, upper levels M
//    (faiss conventions).

#define HNSW_MAXL 8
#define HNSW_HASH 16384
#define HNSW_PROBES 64

// visited-hash helpers (LDS table of id+1, 0 = empty). Deterministic:
// returns true if id was already present OR the probe window is full.
__device__ __forceinline__ unsigned hnsw_hash(unsigned id) {
  unsigned x = id * 0x9E3779B9u;
  x ^= x >> 16;
  return x & (HNSW_HASH - 1);
}

// single-thread insert (thread 0 only)
__device__ __forceinline__ bool hnsw_visited_insert(unsigned *tab, unsigned id) {
  unsigned h = hnsw_hash(id);
  for (int p = 0; p < HNSW_PROBES; ++p) {
    unsigned slot = (h + p) & (HNSW_HASH - 1);
    unsigned v = tab[slot];
    if (v == id + 1) return true;   // already visited
    if (v == 0) {
      tab[slot] = id + 1;
      return false;
    }
  }
  return true;  // cluster full: treat as visited (deterministic)
}

// asymmetric distance: u/s staged in LDS, code row via slab table.
// 8 lanes per row (lane g8 covers bytes [g8*16, g8*16+16) then strides
// by 128), fixed 3-step butterfly — all 8 lanes converge to the same
// bitwise sum (same contract as the SQ8 scan / oracle).
__device__ __forceinline__ float hnsw_dist_q(
    const float *__restrict__ u, const float *__restrict__ s,
    const uint8_t *const *__restrict__ codes, int rlog, int stride, int d,
    long long id, int g8) {
  const uint8_t *cp = slab_row(codes, rlog, id, stride);
  float part = 0.f;
  for (int t0 = g8 * 16; t0 < d; t0 += 128) {
#pragma clang fp contract(off)
    uint4 wv = *reinterpret_cast<const uint4 *>(cp + t0);
    unsigned w0_ = wv.x, w1_ = wv.y, w2_ = wv.z, w3_ = wv.w;
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      if (t0 + b < d) {
        unsigned word = (b < 4) ? w0_ : (b < 8) ? w1_ : (b < 12) ? w2_ : w3_;
        float cf = DFANN_CVT_UB(word, b);
        int t = t0 + b;
        float diff = u[t] - cf * s[t];
        part = part + diff * diff;
      }
    }
  }
  part += __shfl_xor(part, 4, 8);
  part += __shfl_xor(part, 2, 8);
  part += __shfl_xor(part, 1, 8);
  return part;
}

// symmetric (code, code) distance: diff = (c1-c2)*scale
__device__ __forceinline__ float hnsw_dist_cc(
    const float *__restrict__ s, const uint8_t *const *__restrict__ codes,
    int rlog, int stride, int d, long long id1, long long id2, int g8) {
  const uint8_t *p1 = slab_row(codes, rlog, id1, stride);
  const uint8_t *p2 = slab_row(codes, rlog, id2, stride);
  float part = 0.f;
  for (int t0 = g8 * 16; t0 < d; t0 += 128) {
#pragma clang fp contract(off)
    uint4 a = *reinterpret_cast<const uint4 *>(p1 + t0);
    uint4 b4 = *reinterpret_cast<const uint4 *>(p2 + t0);
    unsigned a_[4] = {a.x, a.y, a.z, a.w};
    unsigned b_[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      if (t0 + b < d) {
        float ca = DFANN_CVT_UB(a_[b >> 2], b);
        float cb2 = DFANN_CVT_UB(b_[b >> 2], b);
        int t = t0 + b;
        float diff = (ca - cb2) * s[t];
        part = part + diff * diff;
      }
    }
  }
  part += __shfl_xor(part, 4, 8);
  part += __shfl_xor(part, 2, 8);
  part += __shfl_xor(part, 1, 8);
  return part;
}

// adjacency accessors: level 0 in nbr0 (cap deg0 = 2M), levels >= 1 in
// nbrU at up_slot[node] (cap M per level, HNSW_MAXL levels)
struct HnswGraph {
  const int *__restrict__ levels;
  const int *__restrict__ nbr0;     // n x deg0
  const int *__restrict__ cnt0;     // n
  const int *__restrict__ up_slot;  // n (-1 if level 0 only)
  const int *__restrict__ nbrU;     // nslots x HNSW_MAXL x M
  const int *__restrict__ cntU;     // nslots x HNSW_MAXL
  int deg0, M;

  __device__ __forceinline__ const int *nbrs(long long node, int level,
                                             int &cnt) const {
    if (level == 0) {
      cnt = cnt0[node];
      return nbr0 + node * (size_t)deg0;
    }
    int slot = up_slot[node];
    cnt = cntU[(size_t)slot * HNSW_MAXL + (level - 1)];
    return nbrU + ((size_t)slot * HNSW_MAXL + (level - 1)) * M;
  }
};

// greedy beam-1 descent at one level: returns the closest node found.
// Block-cooperative: 8 lanes per neighbor, 32 neighbors per pass.
__device__ long long hnsw_greedy(const HnswGraph &g,
                                 const float *__restrict__ u,
                                 const float *__restrict__ s,
                                 const uint8_t *const *__restrict__ codes,
                                 int rlog, int stride, int d, long long cur,
                                 float &cur_d, int level, char *lds_scratch,
                                 int self_id = -1) {
  // lds_scratch: [blockDim/8] floats + ids for per-group minima
  float *gd = reinterpret_cast<float *>(lds_scratch);
  int *gi = reinterpret_cast<int *>(lds_scratch + (blockDim.x >> 3) * 4);
  int g8 = threadIdx.x & 7, grp = threadIdx.x >> 3;
  const int NG = blockDim.x >> 3;
  for (;;) {
    int cnt;
    const int *nb = g.nbrs(cur, level, cnt);
    float best_d = DFANN_FLT_MAX;
    int best_i = -1;
    for (int c0 = 0; c0 < cnt; c0 += NG) {
      int ci = c0 + grp;
      if (ci < cnt) {
        int nid = nb[ci];
        if (nid != self_id) {
          float dd = hnsw_dist_q(u, s, codes, rlog, stride, d, nid, g8);
          if (dd < best_d || (dd == best_d && nid < best_i)) {
            best_d = dd;
            best_i = nid;
          }
        }
      }
    }
    if (g8 == 0) {
      gd[grp] = best_d;
      gi[grp] = best_i;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int i = 1; i < NG; ++i)
        if (gd[i] < gd[0] || (gd[i] == gd[0] && gi[i] < gi[0])) {
          gd[0] = gd[i];
          gi[0] = gi[i];
        }
    }
    __syncthreads();
    float nd = gd[0];
    int ni = gi[0];
    __syncthreads();
    if (ni >= 0 && nd < cur_d) {
      cur = ni;
      cur_d = nd;
    } else {
      return cur;
    }
  }
}

// beam search at one level with the Sel frontier (top-ef of everything
// seen; expanded entries flagged in id bit 31). Returns with the Sel
// compacted: s.d/s.p[0..cnt) = sorted (dist, id|flag) results.
// All appends are order-invariant; the expansion order is the sorted
// order — deterministic.
#define HNSW_FLAG 0x80000000u

__device__ void hnsw_beam(const HnswGraph &g, const float *__restrict__ u,
                          const float *__restrict__ s,
                          const uint8_t *const *__restrict__ codes, int rlog,
                          int stride, int d, long long entry, float entry_d,
                          int level, int ef, Sel &sel, unsigned *vis,
                          float *nd_buf, int *ni_buf, int self_id = -1) {
  // vis: HNSW_HASH LDS table; nd/ni_buf: blockDim/8 scratch
  for (int i = threadIdx.x; i < HNSW_HASH; i += blockDim.x) vis[i] = 0;
  sel_init(sel);
  __syncthreads();
  if (threadIdx.x == 0) {
    hnsw_visited_insert(vis, (unsigned)entry);
    sel_try(sel, entry_d, (unsigned)entry);
  }
  __syncthreads();
  sel_compact(sel, ef);
  int g8 = threadIdx.x & 7, grp = threadIdx.x >> 3;
  const int NG = blockDim.x >> 3;
  __shared__ int sh_expand;
  for (;;) {
    // first unexpanded entry in the sorted top-ef
    if (threadIdx.x == 0) {
      int cnt = *sel.cnt;
      int pick = -1;
      for (int i = 0; i < cnt; ++i)
        if (!(sel.p[i] & HNSW_FLAG)) {
          pick = i;
          break;
        }
      if (pick >= 0) sel.p[pick] |= HNSW_FLAG;
      sh_expand = pick >= 0 ? (int)(sel.p[pick] & ~HNSW_FLAG) : -1;
    }
    __syncthreads();
    int cur = sh_expand;
    if (cur < 0) break;
    int cnt;
    const int *nb = g.nbrs(cur, level, cnt);
    // distances for all neighbors (8 lanes each), buffered
    for (int c0 = 0; c0 < cnt; c0 += NG) {
      int ci = c0 + grp;
      float dd = DFANN_FLT_MAX;
      int nid = -1;
      if (ci < cnt) {
        nid = nb[ci];
        dd = hnsw_dist_q(u, s, codes, rlog, stride, d, nid, g8);
      }
      if (g8 == 0) {
        nd_buf[grp] = dd;
        ni_buf[grp] = nid;
      }
      sel_guard(sel, ef, NG);  // headroom for this pass's appends
      // thread 0: dedup via hash, append survivors (order-invariant)
      if (threadIdx.x == 0) {
        int lim = min(NG, cnt - c0);
        for (int i = 0; i < lim; ++i) {
          unsigned id = (unsigned)ni_buf[i];
          if ((int)id != self_id && !hnsw_visited_insert(vis, id))
            sel_try(sel, nd_buf[i], id);
        }
      }
      __syncthreads();
    }
    __syncthreads();
    sel_compact(sel, ef);
  }
}

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------

// u[t] = (q[t] - vmin[t]) - 0.5*scale[t]  (query-side fold)
extern "C" __global__ void k_hnsw_prep(const float *__restrict__ q,
                                       const float *__restrict__ vmin,
                                       const float *__restrict__ scale,
                                       long long nq, int d,
                                       float *__restrict__ u) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = nq * d;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    int t = (int)(i % d);
    u[i] = (q[i] - vmin[t]) - 0.5f * scale[t];
  }
}

// LDS carve for search/insert:
// [scale d floats][u d floats][vis HNSW_HASH u32][Sel][NG dist][NG id]
// insert adds [kept 512 i32][kept_d 512 f32]
#define HNSW_LDS(d, bs)                                                        \
  ((size_t)(d) * 8 + HNSW_HASH * 4 + SEL_LDS_BYTES + ((bs) >> 3) * 8 + 64)
#define HNSW_LDS_INS(d, bs) (HNSW_LDS(d, bs) + 512 * 8)
#define HNSW_LDS_APPLY(d) ((size_t)(d) * 4 + 1024 * 8 + 512 * 4 + 512)

extern "C" __global__ __launch_bounds__(256) void k_hnsw_search(
    const float *__restrict__ uq, const float *__restrict__ scale,
    const uint8_t *const *__restrict__ codes, int rlog, int stride, int d,
    const int *levels, const int *nbr0, const int *cnt0, const int *up_slot,
    const int *nbrU, const int *cntU, int deg0, int M, long long n,
    long long entry, int entry_level, long long nq, int ef, int k,
    float *__restrict__ D, int64_t *__restrict__ I) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *s_s = reinterpret_cast<float *>(smem);
  float *s_u = s_s + d;
  unsigned *vis = reinterpret_cast<unsigned *>(smem + (size_t)d * 8);
  char *selbase = smem + (size_t)d * 8 + HNSW_HASH * 4;
  char *scr = selbase + SEL_LDS_BYTES;
  float *nd_buf = reinterpret_cast<float *>(scr);
  int *ni_buf = reinterpret_cast<int *>(scr + (blockDim.x >> 3) * 4);
  long long qi = blockIdx.x;
  if (qi >= nq) return;
  for (int t = threadIdx.x; t < d; t += blockDim.x) {
    s_s[t] = scale[t];
    s_u[t] = uq[qi * d + t];
  }
  __syncthreads();
  HnswGraph g{levels, nbr0, cnt0, up_slot, nbrU, cntU, deg0, M};
  Sel sel = sel_carve(selbase);
  int g8 = threadIdx.x & 7;
  long long cur = entry;
  float cur_d = hnsw_dist_q(s_u, s_s, codes, rlog, stride, d, cur, g8);
  // all 8 lanes of group 0 share the same value; broadcast via shfl from
  // lane 0 is unnecessary (butterfly converged); other groups recompute
  __syncthreads();
  for (int l = entry_level; l >= 1; --l)
    cur = hnsw_greedy(g, s_u, s_s, codes, rlog, stride, d, cur, cur_d, l, scr);
  hnsw_beam(g, s_u, s_s, codes, rlog, stride, d, cur, cur_d, 0, ef, sel, vis,
            nd_buf, ni_buf);
  int cnt = *sel.cnt;
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    bool v = j < cnt;
    D[qi * k + j] = v ? sel.d[j] : DFANN_FLT_MAX;
    I[qi * k + j] = v ? (long long)(sel.p[j] & ~HNSW_FLAG) : -1;
  }
}

// insertion: one block per wave point. Points [p0, p0+np) insert over
// the frozen snapshot (n_snap nodes). Own links are written directly
// (this point's rows are untouched by other blocks); reverse requests
// (dst, src, dist) go to a bounded append buffer, applied later in
// sorted order by k_hnsw_apply.
extern "C" __global__ __launch_bounds__(256) void k_hnsw_insert(
    const float *__restrict__ up, const float *__restrict__ scale,
    const uint8_t *const *__restrict__ codes, int rlog, int stride, int d,
    const int *levels, int *nbr0, int *cnt0, const int *up_slot, int *nbrU,
    int *cntU, int deg0, int M, long long n_snap, long long entry,
    int entry_level, long long p0, int np, int efc, int *__restrict__ req,
    int *__restrict__ req_cnt, int req_cap, int refine,
    const int *r_nbr0, const int *r_cnt0, const int *r_nbrU,
    const int *r_cntU) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *s_s = reinterpret_cast<float *>(smem);
  float *s_u = s_s + d;
  unsigned *vis = reinterpret_cast<unsigned *>(smem + (size_t)d * 8);
  char *selbase = smem + (size_t)d * 8 + HNSW_HASH * 4;
  char *scr = selbase + SEL_LDS_BYTES;
  float *nd_buf = reinterpret_cast<float *>(scr);
  int *ni_buf = reinterpret_cast<int *>(scr + (blockDim.x >> 3) * 4);
  // kept-neighbor scratch after the group buffers
  int *kept = ni_buf + (blockDim.x >> 3);
  float *kept_d = reinterpret_cast<float *>(kept + 512);

  long long p = p0 + blockIdx.x;
  if (blockIdx.x >= np) return;
  for (int t = threadIdx.x; t < d; t += blockDim.x) {
    s_s[t] = scale[t];
    s_u[t] = up[(size_t)blockIdx.x * d + t];
  }
  __syncthreads();
  // refine traverses a FROZEN copy of the graph (r_*): a refine block
  // rewrites p's adjacency while other blocks may traverse p — reading
  // the live arrays would race into never-initialized slots
  HnswGraph g{levels, r_nbr0 ? r_nbr0 : (const int *)nbr0,
              r_cnt0 ? r_cnt0 : (const int *)cnt0, up_slot,
              r_nbrU ? r_nbrU : (const int *)nbrU,
              r_cntU ? r_cntU : (const int *)cntU, deg0, M};
  Sel sel = sel_carve(selbase);
  int g8 = threadIdx.x & 7;
  int plevel = levels[p];
  if (n_snap == 0) return;  // first point: no links
  int self_id = refine ? (int)p : -1;
  if (refine && (long long)entry == p) return;  // entry re-links itself: skip
  long long cur = entry;
  float cur_d = hnsw_dist_q(s_u, s_s, codes, rlog, stride, d, cur, g8);
  __syncthreads();
  for (int l = entry_level; l > plevel; --l)
    cur = hnsw_greedy(g, s_u, s_s, codes, rlog, stride, d, cur, cur_d, l, scr,
                      self_id);
  for (int l = min(plevel, entry_level); l >= 0; --l) {
    hnsw_beam(g, s_u, s_s, codes, rlog, stride, d, cur, cur_d, l, efc, sel,
              vis, nd_buf, ni_buf, self_id);
    // ---- faiss shrink heuristic: keep c if dist(p,c) < dist(c, kc)
    // for every kept kc (candidates in ascending distance) ----
    int res_cnt = *sel.cnt;
    int cap = M;  // faiss selects M links at every level during add
    __shared__ int n_kept;
    __shared__ int keep_flag;
    if (threadIdx.x == 0) {
      n_kept = 0;
      keep_flag = 1;
    }
    __syncthreads();
    for (int ci = 0; ci < res_cnt && n_kept < cap; ++ci) {
      unsigned cid = sel.p[ci] & ~HNSW_FLAG;
      float cdist = sel.d[ci];
      // dist(c, kc) for all kept in parallel (8 lanes each)
      int grp = threadIdx.x >> 3;
      const int NG = blockDim.x >> 3;
      for (int k0 = 0; k0 < n_kept; k0 += NG) {
        int ki = k0 + grp;
        float dd = DFANN_FLT_MAX;
        if (ki < n_kept)
          dd = hnsw_dist_cc(s_s, codes, rlog, stride, d, (long long)cid,
                            (long long)kept[ki], g8);
        if (g8 == 0) nd_buf[grp] = dd;
        __syncthreads();
        if (threadIdx.x == 0) {
          int lim = min(NG, n_kept - k0);
          for (int i = 0; i < lim; ++i)
            if (nd_buf[i] < cdist) keep_flag = 0;
        }
        __syncthreads();
      }
      if (threadIdx.x == 0) {
        if (keep_flag) {
          kept[n_kept] = (int)cid;
          kept_d[n_kept] = cdist;
          n_kept = n_kept + 1;
        }
        keep_flag = 1;
      }
      __syncthreads();
    }
    // initial insertion: write own links directly (this point's rows
    // are untouched by other blocks) + queue reverse requests.
    // REFINE: do NOT replace own links — the early waves' long-range
    // links are the graph's inter-cluster bridges (measured: replacing
    // them caps recall ~0.6 at 1M); instead queue BOTH directions
    // through the sorted merge+prune (k_hnsw_apply dedups).
    if (threadIdx.x == 0 && n_kept > 0) {
      if (!refine) {
        if (l == 0) {
          cnt0[p] = n_kept;
          for (int i = 0; i < n_kept; ++i) nbr0[p * (size_t)deg0 + i] = kept[i];
        } else {
          int slot = up_slot[p];
          cntU[(size_t)slot * HNSW_MAXL + (l - 1)] = n_kept;
          for (int i = 0; i < n_kept; ++i)
            nbrU[((size_t)slot * HNSW_MAXL + (l - 1)) * M + i] = kept[i];
        }
        int base = atomicAdd(req_cnt, n_kept);
        for (int i = 0; i < n_kept && base + i < req_cap; ++i) {
          int *r = req + (size_t)(base + i) * 4;
          r[0] = kept[i];
          r[1] = (int)p;
          r[2] = l;
          reinterpret_cast<float *>(r)[3] = kept_d[i];
        }
      } else {
        int base = atomicAdd(req_cnt, 2 * n_kept);
        for (int i = 0; i < n_kept && base + 2 * i + 1 < req_cap; ++i) {
          int *r = req + (size_t)(base + 2 * i) * 4;
          r[0] = kept[i];
          r[1] = (int)p;
          r[2] = l;
          reinterpret_cast<float *>(r)[3] = kept_d[i];
          int *r2 = req + (size_t)(base + 2 * i + 1) * 4;
          r2[0] = (int)p;
          r2[1] = kept[i];
          r2[2] = l;
          reinterpret_cast<float *>(r2)[3] = kept_d[i];
        }
      }
    }
    __syncthreads();
    // entry for the next level: nearest result
    if (*sel.cnt > 0) {
      cur = sel.p[0] & ~HNSW_FLAG;
      cur_d = sel.d[0];
    }
    __syncthreads();
  }
}

// apply reverse links: req sorted by (dst, level, src) on host; one
// block per (dst, level) run given by run offsets. Merges existing
// neighbors + incoming sources, prunes with the shrink heuristic when
// over cap. Deterministic: input order is sorted, selection is
// sequential over candidates sorted by distance.
extern "C" __global__ __launch_bounds__(256) void k_hnsw_apply(
    const float *__restrict__ scale,
    const uint8_t *const *__restrict__ codes, int rlog, int stride, int d,
    int *nbr0, int *cnt0, const int *up_slot, int *nbrU, int *cntU, int deg0,
    int M, const int *__restrict__ req, const int *__restrict__ run_off,
    int n_runs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *s_s = reinterpret_cast<float *>(smem);
  // candidate arrays after scale: ids + dists (deg-cap + incoming <= 1024)
  int *cid = reinterpret_cast<int *>(smem + (size_t)d * 4);
  float *cdist = reinterpret_cast<float *>(smem + (size_t)d * 4 + 1024 * 4);
  int *kept = reinterpret_cast<int *>(smem + (size_t)d * 4 + 1024 * 8);
  float *nd_buf = reinterpret_cast<float *>(kept + 512);
  int run = blockIdx.x;
  if (run >= n_runs) return;
  int r0 = run_off[run], r1 = run_off[run + 1];
  int dst = req[(size_t)r0 * 4 + 0];
  int lvl = req[(size_t)r0 * 4 + 2];
  for (int t = threadIdx.x; t < d; t += blockDim.x) s_s[t] = scale[t];
  __syncthreads();
  int cap = lvl == 0 ? deg0 : M;
  int *nbrs;
  int *cnt_p;
  if (lvl == 0) {
    nbrs = nbr0 + (size_t)dst * deg0;
    cnt_p = cnt0 + dst;
  } else {
    int slot = up_slot[dst];
    nbrs = nbrU + ((size_t)slot * HNSW_MAXL + (lvl - 1)) * M;
    cnt_p = cntU + (size_t)slot * HNSW_MAXL + (lvl - 1);
  }
  int old_cnt = *cnt_p;
  int inc = r1 - r0;
  if (old_cnt + inc <= cap) {
    // fast path: append in sorted request order, skipping srcs already
    // linked (refine re-proposes existing links)
    if (threadIdx.x == 0) {
      int w = old_cnt;
      for (int i = 0; i < inc; ++i) {
        int src = req[(size_t)(r0 + i) * 4 + 1];
        bool dup = false;
        for (int j = 0; j < w; ++j)
          if (nbrs[j] == src) { dup = true; break; }
        if (!dup) nbrs[w++] = src;
      }
      *cnt_p = w;
    }
    return;
  }
  // over cap: gather (id, dist(dst, id)) for old + incoming, sort by
  // (dist, id) with a simple block bitonic over 1024 padded entries,
  // then shrink-select up to cap
  int total = old_cnt + inc;
  // REACHABLE: the refine pass is one wave of up to 4096 points, and with
  // duplicate vectors every point proposes the same lowest-id neighbour,
  // so one run can bring more than 1024 - old_cnt requests. Only the
  // first 1024 candidates are considered: the existing links, then the
  // incoming sources in ascending id (the run is sorted by src) — the
  // largest src ids are dropped. Deterministic and in bounds; the oracle
  // mirrors it and tests/test_gpu_hnsw_build.py reaches it.
  if (total > 1024) total = 1024;
  int g8 = threadIdx.x & 7, grp = threadIdx.x >> 3;
  const int NG = blockDim.x >> 3;
  for (int c0 = 0; c0 < total; c0 += NG) {
    int ci = c0 + grp;
    if (ci < total) {
      int id = ci < old_cnt ? nbrs[ci] : req[(size_t)(r0 + ci - old_cnt) * 4 + 1];
      float dd = hnsw_dist_cc(s_s, codes, rlog, stride, d, (long long)dst,
                              (long long)id, g8);
      if (g8 == 0) {
        cid[ci] = id;
        cdist[ci] = dd;
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x + total; i < 1024; i += blockDim.x) {
    cid[i] = 0x7FFFFFFF;
    cdist[i] = DFANN_FLT_MAX;
  }
  // bitonic sort 1024 entries by (dist, id)
  for (int kk = 2; kk <= 1024; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < 1024; i += blockDim.x) {
        int ixj = i ^ j;
        if (ixj > i) {
          bool asc = ((i & kk) == 0);
          float di = cdist[i], dj = cdist[ixj];
          int pi = cid[i], pj = cid[ixj];
          bool less = dj < di || (dj == di && pj < pi);
          if (asc ? less : !less) {
            cdist[i] = dj; cdist[ixj] = di;
            cid[i] = pj; cid[ixj] = pi;
          }
        }
      }
    }
  }
  __syncthreads();
  __shared__ int n_kept;
  __shared__ int drop_marker;
  if (threadIdx.x == 0) { n_kept = 0; drop_marker = 1; }
  __syncthreads();
  for (int ci = 0; ci < total && n_kept < cap; ++ci) {
    int id = cid[ci];
    float dd = cdist[ci];
    if (threadIdx.x == 0) {
      for (int j = 0; j < n_kept; ++j)
        if (kept[j] == id) { drop_marker = 0; break; }
    }
    __syncthreads();
    for (int k0 = 0; k0 < n_kept; k0 += NG) {
      int ki = k0 + grp;
      float kd = DFANN_FLT_MAX;
      if (ki < n_kept)
        kd = hnsw_dist_cc(s_s, codes, rlog, stride, d, (long long)id,
                          (long long)kept[ki], g8);
      if (g8 == 0) nd_buf[grp] = kd;
      __syncthreads();
      if (threadIdx.x == 0) {
        int lim = min(NG, n_kept - k0);
        for (int i = 0; i < lim; ++i)
          if (nd_buf[i] < dd) drop_marker = 0;
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      if (drop_marker) kept[n_kept] = id, n_kept = n_kept + 1;
      drop_marker = 1;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *cnt_p = n_kept;
    for (int i = 0; i < n_kept; ++i) nbrs[i] = kept[i];
  }
}
