// dfann — MI355X-native ANN engine: host runtime + C-ABI (include/dfann.h).
//
// Self-contained HIP/C++ shared library: no torch, no BLAS — every FLOP of
// the hot path runs in the hand-written gfx950 kernels of kernels.hip.
// Python binds via ctypes (distributed_faiss_amd/hip_engine.py).
//
// Index model:
//  * trained artifacts: coarse centroids (+norms), PQ codebooks / SQ ranges
//  * codes live twice: an arrival-order staging arena (append target) and
//    a CSR image grouped by inverted list (search layout), rebuilt lazily
//    ("finalize") via a host counting sort + device gather — the stable
//    sort preserves arrival order inside each list, so CSR position order
//    == ascending arrival id, which the scan's tie-break relies on.
//  * ids are implicit arrival positions (reference quirk).

#include "kernels.hip"
#include "hnsw.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <stdexcept>
#include <algorithm>

#include "../../include/dfann.h"

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------

static thread_local std::string g_err;

#define HIP_CHECK(expr)                                                        \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      throw std::runtime_error(std::string("HIP error: ") +                    \
                               hipGetErrorString(_e) + " at " #expr);          \
    }                                                                          \
  } while (0)

extern "C" const char *dfann_last_error(void) { return g_err.c_str(); }

// DFANN_TRACE=1: synchronize + log after each build/search phase (debug)
static bool trace_on() {
  static int v = -1;
  if (v < 0) {
    const char *e = getenv("DFANN_TRACE");
    v = (e && e[0] == '1') ? 1 : 0;
  }
  return v == 1;
}

static void trace_point(const char *what, hipStream_t s) {
  if (!trace_on()) return;
  hipError_t e = hipStreamSynchronize(s);
  fprintf(stderr, "[dfann] %s: %s\n", what, hipGetErrorString(e));
  fflush(stderr);
}

// ---------------------------------------------------------------------------
// tiny JSON (flat dict of scalars; produced by our own Python side)
// ---------------------------------------------------------------------------

static bool json_find(const std::string &js, const char *key, std::string &out) {
  std::string pat = std::string("\"") + key + "\"";
  size_t p = js.find(pat);
  if (p == std::string::npos) return false;
  p = js.find(':', p + pat.size());
  if (p == std::string::npos) return false;
  ++p;
  while (p < js.size() && (js[p] == ' ' || js[p] == '\t')) ++p;
  if (p >= js.size()) return false;
  if (js[p] == '"') {
    size_t e = js.find('"', p + 1);
    out = js.substr(p + 1, e - p - 1);
  } else {
    size_t e = p;
    while (e < js.size() && (isdigit(js[e]) || js[e] == '-' || js[e] == '.' ||
                             js[e] == 'e' || js[e] == 'E' || js[e] == '+'))
      ++e;
    out = js.substr(p, e - p);
  }
  return true;
}

static long long json_int(const std::string &js, const char *key, long long dflt) {
  std::string v;
  if (!json_find(js, key, v) || v.empty()) return dflt;
  return atoll(v.c_str());
}

// float-valued keys ("k_factor": 1.6); json_int would truncate them
static double json_float(const std::string &js, const char *key, double dflt) {
  std::string v;
  if (!json_find(js, key, v) || v.empty()) return dflt;
  return atof(v.c_str());
}

static std::string json_str(const std::string &js, const char *key,
                            const char *dflt) {
  std::string v;
  if (!json_find(js, key, v)) return dflt;
  return v;
}

// ---------------------------------------------------------------------------
// device buffer
// ---------------------------------------------------------------------------

struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { free(); }
  void ensure(size_t bytes) {
    if (bytes <= cap) return;
    void *np = nullptr;
    HIP_CHECK(hipMalloc(&np, bytes));
    if (p) HIP_CHECK(hipFree(p));
    p = np;
    cap = bytes;
  }
  // grow preserving `keep` bytes of content
  void grow_keep(size_t bytes, size_t keep) {
    if (bytes <= cap) return;
    size_t nb = std::max(bytes, cap * 2);
    void *np = nullptr;
    HIP_CHECK(hipMalloc(&np, nb));
    if (p && keep) HIP_CHECK(hipMemcpy(np, p, keep, hipMemcpyDeviceToDevice));
    if (p) HIP_CHECK(hipFree(p));
    p = np;
    cap = nb;
  }
  void free() {
    if (p) (void)hipFree(p);  // best-effort in destructor paths
    p = nullptr;
    cap = 0;
  }
  template <typename T> T *as() { return reinterpret_cast<T *>(p); }
};

// ---------------------------------------------------------------------------
// slab arena: a growable row store made of fixed-size slabs (1<<rlog rows
// each). The CSR rebuild recycles old slabs behind its write window
// (rebuild_csr), so code images never need a 2x contiguous transient —
// the round-1 staging-arena + CSR duplication is gone.
// Kernels address rows through a device slab-pointer table (kernels.hip
// slab_row).
// ---------------------------------------------------------------------------

struct SlabArena {
  int stride = 0;
  int rlog = 0;                 // rows per slab = 1 << rlog
  std::vector<void *> slabs;    // nullptr = freed
  int64_t rows = 0;             // rows in use (bump)
  DevBuf table;                 // device copy of `slabs`
  bool table_dirty = true;
  bool zero_new = false;        // zero-fill fresh slabs (refine store: pad
                                // bytes of a row are part of its contract)

  void init(int stride_, size_t target_slab_bytes = (size_t)512 << 20) {
    reset();
    stride = stride_;
    rlog = 0;
    while (((size_t)2 << rlog) * stride <= target_slab_bytes) ++rlog;
  }
  int64_t rps() const { return (int64_t)1 << rlog; }
  size_t slab_bytes() const { return (size_t)rps() * stride; }
  void ensure_rows(int64_t n) {
    size_t need = (size_t)((n + rps() - 1) >> rlog);
    while (slabs.size() < need) {
      void *p = nullptr;
      HIP_CHECK(hipMalloc(&p, slab_bytes()));
      if (zero_new) {
        // null-stream memset: drained before any stream writes rows
        HIP_CHECK(hipMemset(p, 0, slab_bytes()));
        HIP_CHECK(hipStreamSynchronize(0));
      }
      slabs.push_back(p);
      table_dirty = true;
    }
  }
  void free_slab(size_t i) {
    if (i < slabs.size() && slabs[i]) {
      (void)hipFree(slabs[i]);
      slabs[i] = nullptr;  // kernels past the window never touch it
    }
  }
  const uint8_t *const *dev_table(hipStream_t s) {
    if (table_dirty) {
      table.ensure(std::max(slabs.size() * 8, (size_t)8));
      if (!slabs.empty())
        HIP_CHECK(hipMemcpyAsync(table.p, slabs.data(), slabs.size() * 8,
                                 hipMemcpyHostToDevice, s));
      HIP_CHECK(hipStreamSynchronize(s));
      table_dirty = false;
    }
    return table.as<const uint8_t *const>();
  }
  uint8_t *const *dev_table_mut(hipStream_t s) {
    return const_cast<uint8_t *const *>(
        reinterpret_cast<const uint8_t *const *>(dev_table(s)));
  }
  // contiguous-host <-> arena row-range copies (persistence, get_lists)
  void copy_rows_to_host(void *dst, int64_t row0, int64_t n) const {
    char *d = (char *)dst;
    int64_t r = row0;
    while (n > 0) {
      int64_t in_slab = std::min<int64_t>(n, rps() - (r & (rps() - 1)));
      const char *src = (const char *)slabs[r >> rlog] +
                        (size_t)(r & (rps() - 1)) * stride;
      HIP_CHECK(hipMemcpy(d, src, (size_t)in_slab * stride,
                          hipMemcpyDeviceToHost));
      d += (size_t)in_slab * stride;
      r += in_slab;
      n -= in_slab;
    }
  }
  void copy_rows_from_host(const void *src, int64_t row0, int64_t n) {
    ensure_rows(row0 + n);
    const char *s = (const char *)src;
    int64_t r = row0;
    while (n > 0) {
      int64_t in_slab = std::min<int64_t>(n, rps() - (r & (rps() - 1)));
      char *dst = (char *)slabs[r >> rlog] + (size_t)(r & (rps() - 1)) * stride;
      HIP_CHECK(hipMemcpy(dst, s, (size_t)in_slab * stride,
                          hipMemcpyHostToDevice));
      s += (size_t)in_slab * stride;
      r += in_slab;
      n -= in_slab;
    }
  }
  void reset() {
    for (auto *p : slabs)
      if (p) (void)hipFree(p);
    slabs.clear();
    rows = 0;
    table.free();
    table_dirty = true;
  }
  ~SlabArena() { reset(); }
};

// ---------------------------------------------------------------------------
// splitmix64 (identical to oracle/core.py)
// ---------------------------------------------------------------------------

struct SplitMix64 {
  uint64_t x;
  explicit SplitMix64(uint64_t seed) : x(seed) {}
  uint64_t next() {
    uint64_t z = (x += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
  }
};

// first k of a partial Fisher-Yates over range(n) (== oracle
// partial_shuffle_indices)
static std::vector<int64_t> pick_init(int64_t n, int64_t k, uint64_t seed) {
  k = std::min(k, n);
  std::vector<int64_t> idx(n);
  for (int64_t i = 0; i < n; ++i) idx[i] = i;
  SplitMix64 rng(seed);
  for (int64_t i = 0; i < k; ++i) {
    int64_t j = i + (int64_t)(rng.next() % (uint64_t)(n - i));
    std::swap(idx[i], idx[j]);
  }
  idx.resize(k);
  return idx;
}

// ---------------------------------------------------------------------------
// index object
// ---------------------------------------------------------------------------

enum IdxType { T_FLAT = 0, T_IVFFLAT = 1, T_IVFPQ = 2, T_IVFSQ = 3, T_HNSW = 4 };
enum { M_IP = 0, M_L2 = 1 };

static int round16(int b) { return (b + 15) & ~15; }

// work items per row of k_sq_encode: one per dimension, or for the packed
// widths one per owned unit of the row's stride (4-bit: a byte, 6-bit: a
// 3-byte group), so that pad bytes are written (as zero) too
static int sq_encode_items(int bits, int d, int stride) {
  return bits == 4 ? stride : bits == 6 ? (stride + 2) / 3 : d;
}

struct TimingEv {
  hipEvent_t a, b;
};

struct dfann_index {
  std::string spec_json;
  int type = T_FLAT;
  int metric = M_IP;
  int d = 0, nlist = 0, m = 0, nbits = 8, dsub = 0, nprobe = 1;
  // ivfsq code width: 16 = fp16, 8 / 6 / 4 = integer codes trained on
  // per-dimension ranges; hnswsq is always 8
  int sq_bits = 16;
  bool sq_int() const { return sq_bits != 16; }
  float sq_q() const { return (float)((1 << sq_bits) - 1); }  // top code
  uint64_t seed = 1234;
  bool trained = false;
  int64_t ntotal = 0;    // ids ever issued (= the first id of the next add)
  int64_t nremoved = 0;  // ids taken out again by dfann_remove_ids (§6j)
  int64_t nlive() const { return ntotal - nremoved; }  // rows stored
  int code_bytes = 0, stride = 0;
  int ws_mb = 512;  // chunk budget for key matrices (spec "ws_mb"; tests
                    // shrink it to force the multi-chunk paths)
  int max_ppc = 256;  // k-means subsample cap per centroid (spec "max_ppc")
  bool coarse_bf16 = false;  // spec "coarse_bf16": assign/coarse GEMMs on
                             // bf16 MFMA (~16x f32 rate) — approximate
                             // ranking path for huge nlist
  bool pq_pre = false;  // spec "pq_precomputed": PQ-L2 term2/term3 tables
  int pq_lut_global = -1;  // spec "pq_lut_global": ADC LUTs built to HBM
                           // by k_pq_lut, scan stages them coalesced
                           // (-1 auto: on together with pq_lut_f16;
                           // 0 off; 1 force, f32 rows unless pq_lut_f16)
  int pq_lut_mb = 2048;  // spec "pq_lut_mb": LUT chunk budget (measured:
                         // bigger chunks win — launch concurrency beats
                         // LLC residency; sweep in BASELINE.md ladder)
  bool pq_lut_f16 = false;  // spec "pq_lut_f16": __half ADC tables —
                            // halves the LUT HBM round-trip AND the scan
                            // LDS (4 blocks/CU at m=64). APPROXIMATION
                            // (faiss GpuIndexIVFPQ useFloat16LookupTables
                            // equivalent): documented tolerance path,
                            // off by default; the exact path stays the
                            // parity contract.
  int scan_fan = 1;  // spec "scan_fan": list-segment fan, clamped to
                     // 1..16 (experiment; non-PQ scans only)

  DevBuf centroids, cnorm, codebooks, sq_vmin, sq_vdiff, sq_scale;
  // CSR code image (slab arena; csr_rows rows grouped by list) + pending
  // appends (slab arena in arrival order, merged in by rebuild_csr)
  SlabArena csr_arena, pend_arena;
  std::vector<int32_t> h_pend_assign;  // pending rows' list assignment
  int64_t csr_rows = 0;                // rows in the CSR image
  int merge_mb = 2048;  // spec "merge_mb": pending bytes that trigger an
                        // incremental merge during add (bounds the
                        // rebuild transient to ~2x this)
  DevBuf cr_ids, cr_off, id2pos, cr_ids_new;
  std::vector<int64_t> h_off;
  bool dirty = false;
  // HNSW (type "hnswsq"): graph over non-residual SQ8 codes in csr_arena
  // (arrival order, never rebuilt). M = h->m, deg0 = 2M.
  int hnsw_efc = 100;
  int hnsw_entry = -1, hnsw_maxlevel = -1, hnsw_nslots = 0;
  std::vector<int32_t> h_levels, h_upslot;
  DevBuf hn_levels, hn_nbr0, hn_cnt0, hn_upslot, hn_nbrU, hn_cntU;
  DevBuf hn_req, hn_reqcnt, hn_runoff, hn_u;
  // flat arena
  DevBuf flat;
  // workspace
  DevBuf ws1, ws2, ws3, ws4, ws5, ws_bf16a, ws_bf16b;
  DevBuf cent_bf16;
  DevBuf chk_ws;  // one word for the input checks of train / add (§6i)
  DevBuf term2, term3_ws, qn_ws;  // PQ-L2 precomputed tables
  DevBuf pq_lut_ws;  // HBM ADC LUTs for the GLUT scan path
  // range search: results live here until the next range
  // call; range_ws = [wave counts | offsets | per-query totals | error word]
  int64_t range_max = 1LL << 27;  // spec "range_max_results"
  DevBuf range_D, range_I, range_ws;
  DevBuf filt_ws;    // filtered search: allow-bitmap in CSR-position space
                     // (rebuilt by k_filter_id2pos on every filtered call)
  // removal. ivf: keep words, their popcounts and the int64
  // prefix of one compaction. flat: the tombstones, a live bitmap over ids
  // that exists from the first removal on (host mirror: adds extend it)
  DevBuf rm_keep, rm_cnt, rm_prefix;
  DevBuf flat_live;
  std::vector<uint32_t> h_flat_live;
  // refine stage: raw rows in arrival order (row i = id i),
  // never rebuilt or moved; the base stage searches k' into rf_D / rf_I
  int refine = 0;          // spec "refine": 0 off, 1 fp32, 2 fp16
  double k_factor = 1.0;   // spec "k_factor" / dfann_set_k_factor
  SlabArena refine_arena;
  DevBuf rf_D, rf_I;
  // OPQ pre-transform (faiss IndexPreTransform(OPQMatrix)):
  // y = A x in front of an ivfpq that works entirely at d = d_out. d_in is
  // the user-facing dimension (== d without a transform); the refine store
  // and k_refine stay at d_in.
  int d_in = 0;
  bool opq = false;       // spec "opq"
  bool opq_set = false;   // A learned / injected / loaded
  int opq_niter = 16;     // spec "opq_niter" (faiss OPQMatrix: 50)
  DevBuf opq_A, opq_At;   // (d_out, d_in) and its transpose, fp32
  DevBuf opq_q, opq_x, opq_r;  // transformed queries / add chunk / decode

  // timing
  bool timing = false;
  std::vector<TimingEv> ev_scan, ev_gemm, ev_merge, ev_lut;
  int64_t scan_rows = 0, scan_bytes = 0, gemm_flops = 0;

  ~dfann_index() {
    for (auto &v : {ev_scan, ev_gemm, ev_merge, ev_lut})
      for (auto &e : v) {
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
      }
  }

  TimingEv ev_begin(hipStream_t s) {
    TimingEv e;
    HIP_CHECK(hipEventCreate(&e.a));
    HIP_CHECK(hipEventCreate(&e.b));
    HIP_CHECK(hipEventRecord(e.a, s));
    return e;
  }
  void ev_end(TimingEv e, hipStream_t s, std::vector<TimingEv> &dst) {
    HIP_CHECK(hipEventRecord(e.b, s));
    dst.push_back(e);
  }
};

// ---------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------

static bool use_regsel(int k) { return k <= 16; }

// PQ codewords per sub-quantizer: 256 (nbits=8) or 16 (nbits=4)
static int pq_ksub(const dfann_index *h) { return 1 << h->nbits; }

// Wave-per-query merges (k_merge_cand_w / k_merge_shards_w): register-path
// k and at most 256 candidates per query, i.e. four per lane.
// DFANN_MERGE_WAVE=0 (A/B knob, read per call) keeps the block-per-query
// kernels.
static bool merge_wave_ok(int k, int64_t C) {
  if (const char *e = getenv("DFANN_MERGE_WAVE"))  // experiment override
    if (atoi(e) == 0) return false;
  return use_regsel(k) && C <= 256;
}

// The three selection paths of the merges (k_merge_cand* / k_merge_shards*)
// and their launch shape, all at 256 threads: wave-per-query (4 queries a
// block, no LDS), register path, LDS selection. `first` is the fastest
// path the caller admits; the slower ones follow in this order.
enum MergePath { MERGE_WAVE, MERGE_RK, MERGE_LDS };
struct MergeLaunch {
  MergePath path;
  dim3 grid;
  size_t lds;
};
static MergeLaunch merge_launch(int64_t nq, int k, int64_t C,
                                MergePath first = MERGE_WAVE) {
  if (first == MERGE_WAVE && merge_wave_ok(k, C))
    return {MERGE_WAVE, dim3((unsigned)((nq + 3) / 4)), 0};
  if (first <= MERGE_RK && use_regsel(k))
    return {MERGE_RK, dim3((unsigned)nq), REGSEL_LDS_BYTES + 128};
  return {MERGE_LDS, dim3((unsigned)nq), SEL_LDS_BYTES};
}

static dim3 grid1d(int64_t total, int block = 256, int64_t cap = 65535LL * 8) {
  int64_t g = (total + block - 1) / block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return dim3((unsigned)g);
}

// C[i][j] keys for rows of A vs rows of B under `metric`.
// mode: 0 -ip, 1 bn-2ip, 2 qn+bn-2ip (needs qn). Result in `keys` (rows x N).
// B_bf16: pre-converted B for the approximate bf16 path (used only when
// h->coarse_bf16 and the caller provides it).
static void gemm_keys_b(dfann_index *h, const float *A, int64_t Mrows,
                        const float *B, const unsigned short *B_bf16,
                        int64_t N, int K, const float *bn, const float *qn,
                        int mode, float *keys, hipStream_t stream) {
  dim3 g((unsigned)((N + GT - 1) / GT), (unsigned)((Mrows + GT - 1) / GT));
  TimingEv e;
  if (h && h->timing) e = h->ev_begin(stream);
  if (h && h->coarse_bf16 && B_bf16) {
    h->ws_bf16a.ensure((size_t)Mrows * K * 2);
    hipLaunchKernelGGL(k_f32_to_bf16, grid1d(Mrows * K), dim3(256), 0, stream,
                       A, Mrows * K, h->ws_bf16a.as<unsigned short>());
    if (K % 8 == 0 && N >= 2048 && Mrows >= 256 && K >= 64) {
      // big coarse/assign shapes: 256^2-tile glds kernel (512 threads)
      dim3 g2((unsigned)((N + 255) / 256), (unsigned)((Mrows + 255) / 256));
      hipLaunchKernelGGL(k_gemm_bf16_256, g2, dim3(512), 0, stream,
                         h->ws_bf16a.as<unsigned short>(), B_bf16, keys,
                         (int)Mrows, (int)N, K, K, K, (int)N, qn, bn, mode);
    } else {
      auto bk = (K % 8 == 0) ? k_gemm_bf16_glds : k_gemm_bf16_nt;
      hipLaunchKernelGGL(bk, g, dim3(256), 0, stream,
                         h->ws_bf16a.as<unsigned short>(), B_bf16, keys,
                         (int)Mrows, (int)N, K, K, K, (int)N, qn, bn, mode);
    }
  } else {
    hipLaunchKernelGGL(k_gemm_nt, g, dim3(256), 0, stream, A, B, keys,
                       (int)Mrows, (int)N, K, K, K, (int)N, qn, bn, mode);
  }
  if (h && h->timing) {
    h->ev_end(e, stream, h->ev_gemm);
    h->gemm_flops += 2LL * Mrows * N * K;
  }
  HIP_CHECK(hipGetLastError());
}

static void gemm_keys(dfann_index *h, const float *A, int64_t Mrows,
                      const float *B, int64_t N, int K, const float *bn,
                      const float *qn, int mode, float *keys,
                      hipStream_t stream) {
  gemm_keys_b(h, A, Mrows, B, nullptr, N, K, bn, qn, mode, keys, stream);
}

// refresh derived images after (re)training / loading: bf16 centroids,
// PQ-L2 precomputed term2
static void refresh_cent_bf16(dfann_index *h, hipStream_t stream) {
  if (h->coarse_bf16 && h->centroids.p) {
    h->cent_bf16.ensure((size_t)h->nlist * h->d * 2);
    hipLaunchKernelGGL(k_f32_to_bf16, grid1d((int64_t)h->nlist * h->d),
                       dim3(256), 0, stream, h->centroids.as<float>(),
                       (long long)h->nlist * h->d,
                       h->cent_bf16.as<unsigned short>());
  }
  if (h->pq_pre && h->type == T_IVFPQ && h->metric == M_L2 &&
      h->centroids.p && h->codebooks.p) {
    h->term2.ensure((size_t)h->nlist * h->m * 256 * 4);
    hipLaunchKernelGGL(k_pq_term2, grid1d((int64_t)h->nlist * h->m * 256),
                       dim3(256), 0, stream, h->centroids.as<float>(),
                       h->codebooks.as<float>(), h->nlist, h->m, h->dsub,
                       h->term2.as<float>());
  }
  HIP_CHECK(hipGetLastError());
}

static void rownorms(const float *x, int64_t n, int d, float *out,
                     hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_rownorm, dim3((unsigned)n), dim3(256), 0, stream, x, n, d,
                     out);
  HIP_CHECK(hipGetLastError());
}

// nearest-centroid assignment of (n x d) rows against h->centroids
static void assign_rows(dfann_index *h, const float *x, int64_t n,
                        int32_t *assign_dev, hipStream_t stream) {
  int nlist = h->nlist;
  // chunk points so the key matrix stays within the ws budget
  int64_t chunk = std::max<int64_t>(1, ((int64_t)h->ws_mb << 20) / ((int64_t)nlist * 4));
  chunk = std::min<int64_t>(chunk, n);
  h->ws1.ensure((size_t)chunk * nlist * 4);
  float *keys = h->ws1.as<float>();
  h->ws2.ensure((size_t)n * 4);
  float *bestv = h->ws2.as<float>();
  hipLaunchKernelGGL(k_assign_init, grid1d(n), dim3(256), 0, stream, bestv,
                     assign_dev, n);
  for (int64_t s = 0; s < n; s += chunk) {
    int64_t c = std::min(chunk, n - s);
    gemm_keys_b(h, x + s * h->d, c, h->centroids.as<float>(),
                h->cent_bf16.as<unsigned short>(), nlist, h->d,
                h->cnorm.as<float>(), nullptr, h->metric == M_IP ? 0 : 1, keys,
                stream);
    hipLaunchKernelGGL(k_assign_rowblock, dim3((unsigned)c), dim3(256), 0,
                       stream, keys, c, (long long)nlist, (long long)nlist, 0,
                       bestv + s, assign_dev + s);
  }
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// input checks of train / add. Both end in a host read of
// one word, so they sit where the caller synchronizes anyway.
// ---------------------------------------------------------------------------

// "NaN" / "Inf" when the array holds such a value, nullptr when all of it
// is finite: k_absmax's unsigned maximum ranks NaN > Inf > finite by bit
// pattern (the sign is cleared first).
static const char *nonfinite_class(dfann_index *h, const float *x,
                                   int64_t total, hipStream_t stream) {
  if (total == 0) return nullptr;
  h->chk_ws.ensure(8);
  HIP_CHECK(hipMemsetAsync(h->chk_ws.p, 0, 4, stream));
  hipLaunchKernelGGL(k_absmax, grid1d(total), dim3(256), 0, stream, x,
                     (long long)total, h->chk_ws.as<unsigned>());
  HIP_CHECK(hipGetLastError());
  unsigned bits = 0;
  HIP_CHECK(hipMemcpyAsync(&bits, h->chk_ws.p, 4, hipMemcpyDeviceToHost,
                           stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  if (bits > 0x7F800000u) return "NaN";
  if (bits == 0x7F800000u) return "Inf";
  return nullptr;
}

// lowest row of a device assignment that is still -1, or -1 when every row
// has a list
static int64_t first_unassigned(dfann_index *h, const int32_t *assign_dev,
                                int64_t n, hipStream_t stream) {
  if (n == 0) return -1;
  h->chk_ws.ensure(8);
  HIP_CHECK(hipMemsetAsync(h->chk_ws.p, 0xFF, 8, stream));
  hipLaunchKernelGGL(k_first_unassigned, grid1d(n), dim3(256), 0, stream,
                     assign_dev, (long long)n,
                     h->chk_ws.as<unsigned long long>());
  HIP_CHECK(hipGetLastError());
  unsigned long long first = 0;
  HIP_CHECK(hipMemcpyAsync(&first, h->chk_ws.p, 8, hipMemcpyDeviceToHost,
                           stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  return first == ~0ULL ? -1 : (int64_t)first;
}

// ---------------------------------------------------------------------------
// k-means (restating faiss Clustering; deviations shared with the oracle —
// oracle/__init__.py header): niter 25, strided subsample to k*256, seeded
// partial-FY init, metric-driven assignment, mean update, deterministic
// largest-donor empty-cluster split.
// ---------------------------------------------------------------------------

static void kmeans_device(dfann_index *h, const float *x, int64_t n, int kcent,
                          int d, int metric, uint64_t seed, float *cent_out,
                          hipStream_t stream, bool hot_start = false,
                          int niter = 25) {
  // hot_start: cent_out already holds the centroids to refine (OPQ's
  // per-round PQ retraining); niter: Lloyd iterations. The defaults are
  // the plain training run.
  const int NITER = niter;
  int64_t cap = (int64_t)kcent * (h ? h->max_ppc : 256);
  DevBuf xt_buf;
  const float *xt = x;
  int64_t nt = n;
  if (n > cap) {
    xt_buf.ensure((size_t)cap * d * 4);
    hipLaunchKernelGGL(k_gather_strided, grid1d(cap * d), dim3(256), 0, stream,
                       x, n, cap, d, xt_buf.as<float>());
    xt = xt_buf.as<float>();
    nt = cap;
  }
  trace_point("kmeans:subsample", stream);
  if (nt < kcent) throw std::runtime_error("kmeans: n < k");

  // init centroids
  DevBuf idx_buf;
  std::vector<int64_t> idx;
  if (!hot_start) {
    idx = pick_init(nt, kcent, seed);
    idx_buf.ensure(idx.size() * 8);
    HIP_CHECK(hipMemcpyAsync(idx_buf.p, idx.data(), idx.size() * 8,
                             hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_gather_rows, grid1d((int64_t)kcent * d), dim3(256), 0,
                       stream, xt, idx_buf.as<int64_t>(), (long long)kcent, d,
                       cent_out);
  }
  trace_point("kmeans:init", stream);

  DevBuf cn, asg, bestv, keys, sums, counts;
  cn.ensure((size_t)kcent * 4);
  asg.ensure((size_t)nt * 4);
  bestv.ensure((size_t)nt * 4);
  sums.ensure((size_t)kcent * d * 8);  // 64-bit fixed point (k_centroid_accum)
  counts.ensure((size_t)kcent * 4);
  // fixed-point scale 2^e with nt * max|x| * 2^e < 2^62 (frexp: max|x| <
  // 2^ea, nt <= 2^en). bestv is free until the first assignment pass.
  HIP_CHECK(hipMemsetAsync(bestv.p, 0, 4, stream));
  hipLaunchKernelGGL(k_absmax, grid1d(nt * d), dim3(256), 0, stream, xt,
                     (long long)(nt * d), bestv.as<unsigned>());
  float absmax = 0.f;
  HIP_CHECK(hipMemcpyAsync(&absmax, bestv.p, 4, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  int ea = 0, en = 0;
  if (std::isfinite(absmax) && absmax > 0.f) std::frexp(absmax, &ea);
  std::frexp((double)nt, &en);
  const double acc_scale = std::ldexp(1.0, 62 - ea - en);
  const double acc_inv_scale = std::ldexp(1.0, -(62 - ea - en));
  int64_t chunk = std::max<int64_t>(
      1, ((int64_t)(h ? h->ws_mb : 512) << 20) / ((int64_t)kcent * 4));
  chunk = std::min(chunk, nt);
  keys.ensure((size_t)chunk * kcent * 4);
  std::vector<int> h_counts(kcent);
  std::vector<float> h_cent;

  DevBuf cent_b16;
  bool use_b16 = h && h->coarse_bf16;
  if (use_b16) cent_b16.ensure((size_t)kcent * d * 2);
  for (int it = 0; it < NITER; ++it) {
    rownorms(cent_out, kcent, d, cn.as<float>(), stream);
    if (use_b16)
      hipLaunchKernelGGL(k_f32_to_bf16, grid1d((int64_t)kcent * d), dim3(256),
                         0, stream, cent_out, (long long)kcent * d,
                         cent_b16.as<unsigned short>());
    hipLaunchKernelGGL(k_assign_init, grid1d(nt), dim3(256), 0, stream,
                       bestv.as<float>(), asg.as<int>(), nt);
    for (int64_t s = 0; s < nt; s += chunk) {
      int64_t c = std::min(chunk, nt - s);
      gemm_keys_b(h, xt + s * d, c, cent_out,
                  use_b16 ? cent_b16.as<unsigned short>() : nullptr, kcent, d,
                  cn.as<float>(), nullptr, metric == M_IP ? 0 : 1,
                  keys.as<float>(), stream);
      hipLaunchKernelGGL(k_assign_rowblock, dim3((unsigned)c), dim3(256), 0,
                         stream, keys.as<float>(), c, (long long)kcent,
                         (long long)kcent, 0, bestv.as<float>() + s,
                         asg.as<int>() + s);
    }
    HIP_CHECK(hipMemsetAsync(sums.p, 0, (size_t)kcent * d * 8, stream));
    HIP_CHECK(hipMemsetAsync(counts.p, 0, (size_t)kcent * 4, stream));
    trace_point("kmeans:assign", stream);
    hipLaunchKernelGGL(k_centroid_accum, grid1d(nt * d), dim3(256), 0, stream,
                       xt, asg.as<int>(), nt, d, acc_scale,
                       sums.as<unsigned long long>(), counts.as<int>());
    trace_point("kmeans:accum", stream);
    hipLaunchKernelGGL(k_centroid_div, grid1d((int64_t)kcent * d), dim3(256), 0,
                       stream, cent_out, sums.as<unsigned long long>(),
                       counts.as<int>(), (long long)kcent, d, acc_inv_scale);
    // empty clusters: deterministic largest-donor split (== oracle)
    HIP_CHECK(hipMemcpyAsync(h_counts.data(), counts.p, (size_t)kcent * 4,
                             hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    // every row joined a cluster? (k_centroid_accum skips a row whose
    // assignment is still -1: finite values whose products overflow)
    int64_t n_asg = 0;
    for (int c = 0; c < kcent; ++c) n_asg += h_counts[c];
    if (n_asg != nt)
      throw std::runtime_error(
          "train: k-means found no nearest centroid for " +
          std::to_string(nt - n_asg) + " of " + std::to_string(nt) +
          " rows (values too large for fp32 distances)");
    bool any_empty = false;
    for (int c = 0; c < kcent; ++c)
      if (h_counts[c] == 0) { any_empty = true; break; }
    if (any_empty) {
      h_cent.resize((size_t)kcent * d);
      HIP_CHECK(hipMemcpy(h_cent.data(), cent_out, (size_t)kcent * d * 4,
                          hipMemcpyDeviceToHost));
      std::vector<int> cw(h_counts.begin(), h_counts.end());
      const float eps = 1.0f / 1024.0f;
      for (int ci = 0; ci < kcent; ++ci) {
        if (h_counts[ci] != 0) continue;
        int cj = (int)(std::max_element(cw.begin(), cw.end()) - cw.begin());
        for (int t = 0; t < d; ++t) {
          float v = h_cent[(size_t)cj * d + t];
          h_cent[(size_t)ci * d + t] = v * (1.0f + eps);
          h_cent[(size_t)cj * d + t] = v * (1.0f - eps);
        }
        cw[ci] = cw[cj] / 2;
        cw[cj] -= cw[cj] / 2;
      }
      HIP_CHECK(hipMemcpy(cent_out, h_cent.data(), (size_t)kcent * d * 4,
                          hipMemcpyHostToDevice));
    }
  }
  xt_buf.free();
}

// ---------------------------------------------------------------------------
// OPQ pre-transform
// ---------------------------------------------------------------------------

// y (n x dout) = x (n x din) . A^T with A (dout x din): the one transform
// launch (k_transform). Counted under gemm_ms / gemm_flops when `h` is given.
static void run_transform(dfann_index *h, const float *A, int64_t n,
                          const float *x, int din, int dout, float *y,
                          hipStream_t stream) {
  if (n == 0) return;
  dim3 g((unsigned)((n + TF_T - 1) / TF_T), (unsigned)((dout + TF_T - 1) / TF_T));
  TimingEv e;
  if (h && h->timing) e = h->ev_begin(stream);
  hipLaunchKernelGGL(k_transform, g, dim3(256), 0, stream, x, A, y,
                     (long long)n, din, dout);
  if (h && h->timing) {
    h->ev_end(e, stream, h->ev_gemm);
    h->gemm_flops += 2LL * n * din * dout;
  }
  HIP_CHECK(hipGetLastError());
}

static void opq_require(const dfann_index *h) {
  if (!h->opq) throw std::runtime_error("index has no opq transform");
  if (!h->opq_set)
    throw std::runtime_error("opq transform not set (train the index or call "
                             "dfann_set_transform)");
}

// The query batch at d_out: q itself without a transform. The workspace
// grows only when a larger batch is first seen (no sync, graph-capturable).
static const float *opq_queries(dfann_index *h, int64_t nq, const float *q,
                                hipStream_t stream) {
  if (!h->opq || nq == 0) return q;
  opq_require(h);
  h->opq_q.ensure((size_t)nq * h->d * 4);
  run_transform(h, h->opq_A.as<float>(), nq, q, h->d_in, h->d,
                h->opq_q.as<float>(), stream);
  return h->opq_q.as<float>();
}

// install A (device, d_out x d_in fp32) and derive its transpose
static void opq_install(dfann_index *h, hipStream_t stream) {
  h->opq_At.ensure((size_t)h->d * h->d_in * 4);
  hipLaunchKernelGGL(k_opq_transpose, grid1d((int64_t)h->d * h->d_in),
                     dim3(256), 0, stream, h->opq_A.as<float>(), h->d, h->d_in,
                     h->opq_At.as<float>());
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(stream));
  h->opq_set = true;
}

static double opq_read(const double *dev, hipStream_t stream) {
  double v = 0.0;
  HIP_CHECK(hipMemcpyAsync(&v, dev, 8, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  return v;
}

template <typename TA, typename TB>
static void opq_dgemm(const TA *A, long long sai, long long sak, const TB *B,
                      long long sbk, long long sbj, int R, int C, long long K,
                      double alpha, double beta, const double *E, double *out,
                      hipStream_t stream) {
  dim3 g((unsigned)((C + 31) / 32), (unsigned)((R + 31) / 32));
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_opq_dgemm<TA, TB>), g, dim3(256), 0,
                     stream, A, sai, sak, B, sbk, sbj, R, C, K, alpha, beta, E,
                     out);
  HIP_CHECK(hipGetLastError());
}

// Orthonormal polar factor of X (R x C, R >= C, fp64, in place) by
// Newton-Schulz: X <- 1.5 X - 0.5 X (X^T X) from X / |X|_F, until
// max|X^T X - I| < 1e-10 (fp64 round-off of the C-term dot products is
// ~1e-13). GEMM-only; the iteration count adapts to the singular-value
// spread (each step lifts a small singular value by 1.5x).
static void opq_polar(double *X, int R, int C, DevBuf &G, DevBuf &T,
                      DevBuf &scal, hipStream_t stream) {
  const long long total = (long long)R * C;
  G.ensure((size_t)C * C * 8);
  T.ensure((size_t)total * 8);
  scal.ensure(16);
  double *s = scal.as<double>();
  hipLaunchKernelGGL(k_opq_sumsq, dim3(1), dim3(256), 0, stream, X, total, s);
  double fro = std::sqrt(opq_read(s, stream));
  if (!(fro > 0.0) || !std::isfinite(fro))
    throw std::runtime_error("opq: polar factor of a zero / non-finite matrix");
  hipLaunchKernelGGL(k_opq_axpby, grid1d(total), dim3(256), 0, stream, X,
                     1.0 / fro, (const double *)nullptr, 0.0, total);
  const int CAP = 200;
  const double TOL = 1e-10;
  double err = 0.0;
  double *cur = X, *nxt = T.as<double>();
  for (int it = 0; it <= CAP; ++it) {
    // G = cur^T cur
    opq_dgemm<double, double>(cur, 1, C, cur, C, 1, C, C, R, 1.0, 0.0, nullptr,
                              G.as<double>(), stream);
    hipLaunchKernelGGL(k_opq_maxdev, dim3(1), dim3(256), 0, stream,
                       G.as<double>(), C, s);
    err = opq_read(s, stream);
    if (err < TOL) break;
    if (it == CAP)
      throw std::runtime_error(
          "opq: Newton-Schulz polar iteration did not converge in " +
          std::to_string(CAP) + " steps (max|XtX - I| = " +
          std::to_string(err) + ")");
    // nxt = 1.5 cur - 0.5 cur G
    opq_dgemm<double, double>(cur, C, 1, G.as<double>(), C, 1, R, C, C, -0.5,
                              1.5, cur, nxt, stream);
    std::swap(cur, nxt);
  }
  if (cur != X)
    HIP_CHECK(hipMemcpyAsync(X, cur, (size_t)total * 8,
                             hipMemcpyDeviceToDevice, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
}

// Learn A on the raw training rows (restates faiss OPQMatrix::train):
// alternate a plain m x ksub PQ on Y = Xc A^T with the orthogonal
// Procrustes update A^T = polar(Xc^T Yhat).
static void opq_learn(dfann_index *h, int64_t n, const float *x,
                      hipStream_t stream) {
  const int di = h->d_in, dout = h->d, m = h->m, dsub = h->dsub;
  const int ksub = pq_ksub(h);
  // 1) strided subsample, centred (the mean is a training device only)
  const int64_t nt = std::min<int64_t>(n, 65536);
  if (nt < ksub)
    throw std::runtime_error("opq: fewer training rows than PQ codewords");
  DevBuf xc, mean;
  xc.ensure((size_t)nt * di * 4);
  mean.ensure((size_t)di * 8);
  hipLaunchKernelGGL(k_gather_strided, grid1d(nt * di), dim3(256), 0, stream, x,
                     (long long)n, (long long)nt, di, xc.as<float>());
  hipLaunchKernelGGL(k_opq_colmean, dim3((unsigned)di), dim3(256), 0, stream,
                     xc.as<float>(), (long long)nt, di, mean.as<double>());
  hipLaunchKernelGGL(k_opq_center, grid1d(nt * di), dim3(256), 0, stream,
                     xc.as<float>(), (long long)nt, di, mean.as<double>());
  HIP_CHECK(hipGetLastError());
  // 2) seeded Gaussian d_in x d_in (SplitMix64 + Box-Muller), orthonormalised
  //    by the same polar routine; its first d_out columns are A^T
  DevBuf Q, P, M, G, T, scal;
  {
    std::vector<double> g((size_t)di * di);
    SplitMix64 rng(h->seed ^ 0x4F50514D41545258ULL);  // "OPQMATRX"
    for (size_t i = 0; i < g.size(); i += 2) {
      double u1 = ((double)(rng.next() >> 11) + 1.0) * (1.0 / 9007199254740992.0);
      double u2 = (double)(rng.next() >> 11) * (1.0 / 9007199254740992.0);
      double r = std::sqrt(-2.0 * std::log(u1));
      g[i] = r * std::cos(6.283185307179586 * u2);
      if (i + 1 < g.size()) g[i + 1] = r * std::sin(6.283185307179586 * u2);
    }
    Q.ensure(g.size() * 8);
    HIP_CHECK(hipMemcpy(Q.p, g.data(), g.size() * 8, hipMemcpyHostToDevice));
  }
  opq_polar(Q.as<double>(), di, di, G, T, scal, stream);
  P.ensure((size_t)di * dout * 8);
  M.ensure((size_t)di * dout * 8);
  hipLaunchKernelGGL(k_opq_take_cols, grid1d((int64_t)di * dout), dim3(256), 0,
                     stream, Q.as<double>(), di, dout, P.as<double>());
  Q.free();  // (columns of an orthonormal square matrix: no second pass)
  h->opq_A.ensure((size_t)dout * di * 4);
  h->opq_At.ensure((size_t)dout * di * 4);
  auto store = [&]() {
    hipLaunchKernelGGL(k_opq_store, grid1d((int64_t)di * dout), dim3(256), 0,
                       stream, P.as<double>(), di, dout, h->opq_A.as<float>(),
                       h->opq_At.as<float>());
    HIP_CHECK(hipGetLastError());
  };
  store();
  // 3) alternate
  DevBuf y, yhat, sub, cb, cbn, best, bestv;
  y.ensure((size_t)nt * dout * 4);
  yhat.ensure((size_t)nt * dout * 4);
  sub.ensure((size_t)nt * dsub * 4);
  cb.ensure((size_t)m * ksub * dsub * 4);
  cbn.ensure((size_t)ksub * 4);
  best.ensure((size_t)nt * 4);
  bestv.ensure((size_t)nt * 4);
  int64_t chunk = std::max<int64_t>(1, ((int64_t)h->ws_mb << 20) / (ksub * 4));
  chunk = std::min<int64_t>(chunk, nt);
  h->ws1.ensure((size_t)chunk * ksub * 4);
  for (int it = 0; it < h->opq_niter; ++it) {
    run_transform(nullptr, h->opq_A.as<float>(), nt, xc.as<float>(), di, dout,
                  y.as<float>(), stream);
    for (int j = 0; j < m; ++j) {
      float *cbj = cb.as<float>() + (size_t)j * ksub * dsub;
      hipLaunchKernelGGL(k_subspace_slice, grid1d(nt * dsub), dim3(256), 0,
                         stream, y.as<float>(), (long long)nt, dout, j * dsub,
                         dsub, sub.as<float>());
      // faiss niter_pq_0 / niter_pq (40 / 4): here the engine's 25 on the
      // first round, then 4 hot-started
      kmeans_device(h, sub.as<float>(), nt, ksub, dsub, M_L2,
                    h->seed + 1000 + j, cbj, stream, it > 0, it == 0 ? 25 : 4);
      // encode + decode
      rownorms(cbj, ksub, dsub, cbn.as<float>(), stream);
      hipLaunchKernelGGL(k_assign_init, grid1d(nt), dim3(256), 0, stream,
                         bestv.as<float>(), best.as<int>(), nt);
      for (int64_t s0 = 0; s0 < nt; s0 += chunk) {
        int64_t c = std::min(chunk, nt - s0);
        gemm_keys(nullptr, sub.as<float>() + s0 * dsub, c, cbj, ksub, dsub,
                  cbn.as<float>(), nullptr, 1, h->ws1.as<float>(), stream);
        hipLaunchKernelGGL(k_assign_rowblock, dim3((unsigned)c), dim3(256), 0,
                           stream, h->ws1.as<float>(), c, (long long)ksub,
                           (long long)ksub, 0, bestv.as<float>() + s0,
                           best.as<int>() + s0);
      }
      hipLaunchKernelGGL(k_opq_decode_sub, grid1d(nt * dsub), dim3(256), 0,
                         stream, best.as<int>(), cbj, (long long)nt, dout,
                         j * dsub, dsub, ksub, yhat.as<float>());
      HIP_CHECK(hipGetLastError());
    }
    // M = Xc^T Yhat (d_in x d_out), regularised with the previous rotation so
    // that a null direction of the data keeps its orientation instead of
    // stalling the iteration at a zero singular value
    opq_dgemm<float, float>(xc.as<float>(), 1, di, yhat.as<float>(), dout, 1,
                            di, dout, nt, 1.0, 0.0, nullptr, M.as<double>(),
                            stream);
    hipLaunchKernelGGL(k_opq_sumsq, dim3(1), dim3(256), 0, stream,
                       M.as<double>(), (long long)di * dout, scal.as<double>());
    double fro = std::sqrt(opq_read(scal.as<double>(), stream));
    if (!std::isfinite(fro))
      throw std::runtime_error("opq: non-finite training data");
    if (!(fro > 0.0)) break;  // all-zero data: keep the initial rotation
    hipLaunchKernelGGL(k_opq_axpby, grid1d((int64_t)di * dout), dim3(256), 0,
                       stream, M.as<double>(), 1.0, P.as<double>(), 1e-6 * fro,
                       (long long)di * dout);
    opq_polar(M.as<double>(), di, dout, G, T, scal, stream);
    std::swap(M.p, P.p);
    std::swap(M.cap, P.cap);
    store();
    trace_point("opq:iter", stream);
  }
  HIP_CHECK(hipStreamSynchronize(stream));
  h->opq_set = true;
}

// ---------------------------------------------------------------------------
// create / train / add / finalize
// ---------------------------------------------------------------------------

static dfann_index *create_from_spec(const std::string &js) {
  auto *h = new dfann_index();
  h->spec_json = js;
  std::string t = json_str(js, "type", "");
  if (t == "flat") h->type = T_FLAT;
  else if (t == "ivf_flat") h->type = T_IVFFLAT;
  else if (t == "ivfpq") h->type = T_IVFPQ;
  else if (t == "ivfsq") h->type = T_IVFSQ;
  else if (t == "hnswsq") h->type = T_HNSW;
  else { delete h; throw std::runtime_error("unknown index type '" + t + "'"); }
  h->d = (int)json_int(js, "dim", 0);
  h->metric = (int)json_int(js, "metric", M_IP);
  h->nlist = (int)json_int(js, "nlist", 0);
  h->m = (int)json_int(js, "m", 0);
  h->nbits = (int)json_int(js, "nbits", 8);
  h->nprobe = (int)json_int(js, "nprobe", 1);
  h->seed = (uint64_t)json_int(js, "seed", 1234);
  {
    std::string sq = json_str(js, "sq_type", "fp16");
    h->sq_bits = sq == "8bit" ? 8 : sq == "6bit" ? 6 : sq == "4bit" ? 4 : 16;
  }
  h->ws_mb = (int)json_int(js, "ws_mb", 512);
  if (h->ws_mb < 1) h->ws_mb = 1;
  h->coarse_bf16 = json_int(js, "coarse_bf16", 0) != 0;
  h->max_ppc = (int)json_int(js, "max_ppc", 256);
  h->pq_pre = json_int(js, "pq_precomputed", 0) != 0;
  h->pq_lut_global = (int)json_int(js, "pq_lut_global", -1);
  h->pq_lut_mb = (int)json_int(js, "pq_lut_mb", 2048);
  if (h->pq_lut_mb < 1) h->pq_lut_mb = 1;
  h->pq_lut_f16 = json_int(js, "pq_lut_f16", 0) != 0;
  h->scan_fan = (int)json_int(js, "scan_fan", 1);
  if (h->scan_fan < 1) h->scan_fan = 1;
  if (h->scan_fan > 16) h->scan_fan = 16;
  h->range_max = json_int(js, "range_max_results", 1LL << 27);
  if (h->range_max < 0) throw std::runtime_error("range_max_results must be >= 0");
  if (h->d <= 0) { delete h; throw std::runtime_error("bad dim"); }
  h->d_in = h->d;
  h->opq = json_int(js, "opq", 0) != 0;
  if (h->opq) {
    // faiss IndexPreTransform(OPQMatrix(d, M, d2), IndexIVFPQ): from here on
    // h->d is the inner index dimension d_out (faiss extract_index_ivf sees
    // the same: quantizer and PQ live at d2), h->d_in the caller's
    int d_out = (int)json_int(js, "opq_dim", h->d_in);
    h->opq_niter = (int)json_int(js, "opq_niter", 16);
    std::string bad;
    if (h->type != T_IVFPQ)
      bad = "\"opq\" unsupported for index type '" + t + "' (ivfpq only)";
    else if (d_out > h->d_in || d_out <= 0)
      bad = "opq_dim=" + std::to_string(d_out) + " must be in 1..dim (" +
            std::to_string(h->d_in) + ")";
    else if (h->m <= 0 || d_out % h->m)
      bad = "opq_dim=" + std::to_string(d_out) + " is not a multiple of m=" +
            std::to_string(h->m);
    else if (h->pq_pre)
      bad = "\"opq\" with pq_precomputed unsupported (the term2 table is not "
            "wired behind the transform)";
    else if (h->opq_niter < 1)
      bad = "opq_niter must be >= 1";
    if (!bad.empty()) { delete h; throw std::runtime_error(bad); }
    h->d = d_out;
  } else if (json_int(js, "opq_dim", 0) != 0) {
    delete h;
    throw std::runtime_error("opq_dim given without \"opq\": 1");
  }
  if (h->type != T_FLAT && h->type != T_HNSW && h->nlist <= 0) {
    delete h;
    throw std::runtime_error("bad nlist");
  }
  if (h->type == T_IVFPQ) {
    if (h->nbits != 4 && h->nbits != 8) {
      int nb = h->nbits;
      delete h;
      throw std::runtime_error("ivfpq nbits=" + std::to_string(nb) +
                               " unsupported (supported: 4, 8)");
    }
    if (h->m <= 0 || h->d % h->m) {
      delete h;
      throw std::runtime_error("bad m (dim % m != 0)");
    }
    h->dsub = h->d / h->m;
    h->code_bytes = h->nbits == 4 ? (h->m + 1) / 2 : h->m;
    if (h->nbits == 4) {
      // only the in-kernel fp32 LUT exists at 4 bits; a
      // knob that would change results or layout is refused, not dropped
      const char *bad = h->pq_lut_f16           ? "pq_lut_f16"
                        : h->pq_lut_global == 1 ? "pq_lut_global"
                        : h->pq_pre             ? "pq_precomputed"
                                                : nullptr;
      if (bad) {
        delete h;
        throw std::runtime_error(std::string("ivfpq nbits=4: ") + bad +
                                 " unsupported (in-kernel fp32 LUT only)");
      }
    }
  } else if (h->type == T_IVFSQ) {
    // integer codes are a packed little-endian bit stream (faiss
    // Codec4bit / Codec6bit); 8 bits is the byte-per-dim case of it
    h->code_bytes = h->sq_int() ? (h->d * h->sq_bits + 7) / 8 : 2 * h->d;
  } else if (h->type == T_IVFFLAT) {
    h->code_bytes = 4 * h->d;
  } else if (h->type == T_HNSW) {
    // reference index.py:51-60: faiss.IndexHNSWSQ(dim, QT_8bit, store_n)
    // with L2 asserted; spec m = store_n (link cap M), nprobe = efSearch
    if (h->metric != M_L2)
      { delete h; throw std::runtime_error("hnswsq requires L2 (ref index.py:52)"); }
    if (h->m <= 0) h->m = 128;  // reference store_n default
    if (h->m < 2) {
      // the level draw uses mL = 1/ln(M): M = 1 has no level distribution
      delete h;
      throw std::runtime_error(
          "hnswsq store_n < 2 unsupported (level draw needs 1/ln(M))");
    }
    if (h->m > 256) {
      delete h;
      throw std::runtime_error(
          "hnswsq store_n > 256 unsupported (level-0 degree cap 2M is "
          "sized 512 in the merge kernels)");
    }
    h->hnsw_efc = (int)json_int(js, "ef_construction", 100);
    if (h->hnsw_efc < 1) h->hnsw_efc = 1;
    if (h->hnsw_efc > 512) h->hnsw_efc = 512;
    h->sq_bits = 8;
    h->code_bytes = h->d;
  } else {
    h->code_bytes = 4 * h->d;
    h->trained = true;  // flat needs no training
  }
  h->stride = round16(h->code_bytes);
  h->merge_mb = (int)json_int(js, "merge_mb", 2048);
  if (h->merge_mb < 1) h->merge_mb = 1;
  // 64 MB slabs: small enough that an empty index costs little, large
  // enough that the 1B-row table stays a few thousand L1-hot entries
  // ("slab_mb" shrinks them: the window logic of rebuild_csr and of the
  // removal compaction is only reachable in a test at a small slab size)
  int csr_slab_mb = (int)json_int(js, "slab_mb", 64);
  csr_slab_mb = std::min(std::max(csr_slab_mb, 1), 4096);
  h->csr_arena.init(h->stride, (size_t)csr_slab_mb << 20);
  h->pend_arena.init(h->stride, (size_t)csr_slab_mb << 20);
  if (h->nlist > 0) h->h_off.assign(h->nlist + 1, 0);
  // refine stage (faiss IndexRefineFlat / IndexRefine(SQfp16))
  std::string rf = json_str(js, "refine", "");
  if (!rf.empty()) {
    if (rf == "fp32") h->refine = 1;
    else if (rf == "fp16") h->refine = 2;
    else {
      delete h;
      throw std::runtime_error("unknown refine codec '" + rf +
                               "' (supported: fp32, fp16)");
    }
    if (h->type != T_IVFPQ && h->type != T_IVFSQ) {
      delete h;
      throw std::runtime_error("refine unsupported for index type '" + t +
                               "' (supported bases: ivfpq, ivfsq)");
    }
    h->k_factor = json_float(js, "k_factor", 1.0);
    if (!(h->k_factor >= 1.0)) {
      delete h;
      throw std::runtime_error("k_factor must be >= 1");
    }
    if (REFINE_LDS_BYTES(h->d_in) > 64 * 1024) {
      delete h;
      throw std::runtime_error("refine: dim too large for the query stage");
    }
    int slab_mb = (int)json_int(js, "refine_slab_mb", 64);
    if (slab_mb < 1) slab_mb = 1;
    h->refine_arena.init(round16(h->d_in * (h->refine == 1 ? 4 : 2)),
                         (size_t)slab_mb << 20);
    h->refine_arena.zero_new = true;
  } else if (json_float(js, "k_factor", 1.0) < 1.0) {
    delete h;
    throw std::runtime_error("k_factor must be >= 1");
  }
  return h;
}

static void hnsw_train_ranges(dfann_index *h, int64_t n, const float *x,
                              hipStream_t stream) {
  DevBuf mn, mx;
  mn.ensure((size_t)h->d * 4);
  mx.ensure((size_t)h->d * 4);
  h->sq_vmin.ensure((size_t)h->d * 4);
  h->sq_vdiff.ensure((size_t)h->d * 4);
  h->sq_scale.ensure((size_t)h->d * 4);
  hipLaunchKernelGGL(k_minmax_init, grid1d(h->d), dim3(256), 0, stream,
                     mn.as<unsigned>(), mx.as<unsigned>(), h->d);
  hipLaunchKernelGGL(k_minmax_dims, grid1d(n * h->d), dim3(256), 0, stream, x,
                     n, h->d, mn.as<unsigned>(), mx.as<unsigned>());
  hipLaunchKernelGGL(k_minmax_decode, grid1d(h->d), dim3(256), 0, stream,
                     mn.as<unsigned>(), mx.as<unsigned>(), h->d,
                     h->sq_vmin.as<float>(), h->sq_vdiff.as<float>(),
                     h->sq_scale.as<float>(), h->sq_q());
  HIP_CHECK(hipStreamSynchronize(stream));
}

static void train_impl(dfann_index *h, int64_t n, const float *x,
                       hipStream_t stream) {
  if (h->type == T_FLAT) { h->trained = true; return; }
  if (h->trained) return;  // faiss semantics: re-train of trained is a no-op here
  if (h->type == T_HNSW) {
    // non-residual SQ8 codec: per-dim ranges over the raw training set
    // (faiss IndexHNSWSQ trains its storage IndexScalarQuantizer)
    hnsw_train_ranges(h, n, x, stream);
    h->trained = true;
    return;
  }
  h->centroids.ensure((size_t)h->nlist * h->d * 4);
  h->cnorm.ensure((size_t)h->nlist * 4);
  trace_point("train:begin", stream);
  kmeans_device(h, x, n, h->nlist, h->d, h->metric, h->seed,
                h->centroids.as<float>(), stream);
  trace_point("train:coarse-kmeans", stream);
  rownorms(h->centroids.as<float>(), h->nlist, h->d, h->cnorm.as<float>(),
           stream);
  refresh_cent_bf16(h, stream);  // bf16 image for the assign below
  if (h->type == T_IVFPQ || (h->type == T_IVFSQ && h->sq_int())) {
    DevBuf asg, resid;
    asg.ensure((size_t)n * 4);
    resid.ensure((size_t)n * h->d * 4);
    assign_rows(h, x, n, asg.as<int>(), stream);
    trace_point("train:assign", stream);
    // all n rows are assigned here, not only the k-means subsample
    int64_t bad = first_unassigned(h, asg.as<int>(), n, stream);
    if (bad >= 0)
      throw std::runtime_error(
          "train: row " + std::to_string(bad) +
          " has no nearest centroid (values too large for fp32 distances)");
    hipLaunchKernelGGL(k_residual, grid1d(n * h->d), dim3(256), 0, stream, x,
                       h->centroids.as<float>(), asg.as<int>(), n, h->d,
                       resid.as<float>());
    trace_point("train:residual", stream);
    if (h->type == T_IVFPQ) {
      const int ksub = pq_ksub(h);
      h->codebooks.ensure((size_t)h->m * ksub * h->dsub * 4);
      DevBuf sub;
      sub.ensure((size_t)n * h->dsub * 4);
      for (int j = 0; j < h->m; ++j) {
        hipLaunchKernelGGL(k_subspace_slice, grid1d(n * h->dsub), dim3(256), 0,
                           stream, resid.as<float>(), n, h->d, j * h->dsub,
                           h->dsub, sub.as<float>());
        kmeans_device(h, sub.as<float>(), n, ksub, h->dsub, M_L2,
                      h->seed + 1 + j,
                      h->codebooks.as<float>() + (size_t)j * ksub * h->dsub,
                      stream);
        trace_point("train:pq-sub", stream);
      }
    } else {  // SQ8 / SQ6 / SQ4 ranges on residuals
      DevBuf mn, mx;
      mn.ensure((size_t)h->d * 4);
      mx.ensure((size_t)h->d * 4);
      h->sq_vmin.ensure((size_t)h->d * 4);
      h->sq_vdiff.ensure((size_t)h->d * 4);
      h->sq_scale.ensure((size_t)h->d * 4);
      hipLaunchKernelGGL(k_minmax_init, grid1d(h->d), dim3(256), 0, stream,
                         mn.as<unsigned>(), mx.as<unsigned>(), h->d);
      hipLaunchKernelGGL(k_minmax_dims, grid1d(n * h->d), dim3(256), 0, stream,
                         resid.as<float>(), n, h->d, mn.as<unsigned>(),
                         mx.as<unsigned>());
      hipLaunchKernelGGL(k_minmax_decode, grid1d(h->d), dim3(256), 0, stream,
                         mn.as<unsigned>(), mx.as<unsigned>(), h->d,
                         h->sq_vmin.as<float>(), h->sq_vdiff.as<float>(),
                         h->sq_scale.as<float>(), h->sq_q());
    }
  }
  refresh_cent_bf16(h, stream);  // + term2 now that codebooks exist
  HIP_CHECK(hipStreamSynchronize(stream));
  h->trained = true;
}

// Merge [old CSR + pending appends] into a fresh CSR slab set.
// Order-preserving two-source merge: new list l = old rows of l (already
// in ascending-arrival order) followed by pending rows of l (arrival
// order via the counting-sort permutation), so CSR position order within
// a list stays == ascending arrival id (the scan tie-break contract).
// Old slabs are freed behind the write window: because new pos >= old
// pos for every old row, old slab s is fully consumed once the write
// cursor passes (s+1)*rps + pend_rows — peak memory stays
// ~codes + pending + one slab instead of the round-1 2x duplication.
static void rebuild_csr(dfann_index *h, hipStream_t stream) {
  if (!h->dirty) return;
  int64_t n_pend = (int64_t)h->h_pend_assign.size();
  int64_t n_old = h->csr_rows;
  int64_t n_new = n_old + n_pend;
  // pending counting sort (stable -> arrival order within each list)
  std::vector<int64_t> pend_off(h->nlist + 1, 0);
  for (int32_t a : h->h_pend_assign) pend_off[a + 1]++;
  for (int l = 0; l < h->nlist; ++l) pend_off[l + 1] += pend_off[l];
  std::vector<unsigned> psrc(std::max<int64_t>(n_pend, 1));
  {
    std::vector<int64_t> fill(pend_off.begin(), pend_off.end() - 1);
    for (int64_t i = 0; i < n_pend; ++i)
      psrc[fill[h->h_pend_assign[i]]++] = (unsigned)i;
  }
  std::vector<int64_t> old_off = h->h_off;
  if ((int64_t)old_off.size() != h->nlist + 1)
    old_off.assign(h->nlist + 1, 0);
  std::vector<int64_t> new_off(h->nlist + 1, 0);
  for (int l = 0; l < h->nlist; ++l)
    new_off[l + 1] = new_off[l] + (old_off[l + 1] - old_off[l]) +
                     (pend_off[l + 1] - pend_off[l]);
  // device tables
  DevBuf d_new_off, d_old_off, d_pend_off, d_psrc;
  d_new_off.ensure((size_t)(h->nlist + 1) * 8);
  d_old_off.ensure((size_t)(h->nlist + 1) * 8);
  d_pend_off.ensure((size_t)(h->nlist + 1) * 8);
  d_psrc.ensure((size_t)std::max<int64_t>(n_pend, 1) * 4);
  HIP_CHECK(hipMemcpyAsync(d_new_off.p, new_off.data(),
                           (size_t)(h->nlist + 1) * 8, hipMemcpyHostToDevice,
                           stream));
  HIP_CHECK(hipMemcpyAsync(d_old_off.p, old_off.data(),
                           (size_t)(h->nlist + 1) * 8, hipMemcpyHostToDevice,
                           stream));
  HIP_CHECK(hipMemcpyAsync(d_pend_off.p, pend_off.data(),
                           (size_t)(h->nlist + 1) * 8, hipMemcpyHostToDevice,
                           stream));
  if (n_pend)
    HIP_CHECK(hipMemcpyAsync(d_psrc.p, psrc.data(), (size_t)n_pend * 4,
                             hipMemcpyHostToDevice, stream));
  h->cr_ids_new.ensure((size_t)std::max<int64_t>(n_new, 1) * 8);
  // id2pos covers the id space, not the row count. A grown table starts as
  // all sentinels: the gather rewrites every stored id, removed ids stay
  // PAD_POS.
  if ((size_t)h->ntotal * 4 > h->id2pos.cap) {
    h->id2pos.ensure(std::max((size_t)h->ntotal * 4, h->id2pos.cap * 2));
    HIP_CHECK(hipMemsetAsync(h->id2pos.p, 0xFF, h->id2pos.cap, stream));
  }
  SlabArena next;
  next.init(h->stride, h->csr_arena.slab_bytes());
  const int64_t rps = next.rps();
  // pending row p arrived as id (ntotal - n_pend) + p: the CSR row count
  // stops being the id base once a row was removed
  int64_t id_base = h->ntotal - n_pend;
  size_t old_free_cursor = 0;
  const uint8_t *const *old_tab = h->csr_arena.dev_table(stream);
  const uint8_t *const *pend_tab = h->pend_arena.dev_table(stream);
  for (int64_t j0 = 0; j0 < n_new; j0 += rps) {
    int64_t j1 = std::min(n_new, j0 + rps);
    next.ensure_rows(j1);
    hipLaunchKernelGGL(k_rebuild_gather, grid1d(j1 - j0), dim3(256), 0, stream,
                       j0, j1, d_new_off.as<int64_t>(), d_old_off.as<int64_t>(),
                       d_pend_off.as<int64_t>(), d_psrc.as<unsigned>(),
                       old_tab, pend_tab, next.dev_table_mut(stream),
                       h->cr_ids.as<int64_t>(), id_base,
                       h->cr_ids_new.as<int64_t>(), h->id2pos.as<unsigned>(),
                       h->nlist, next.rlog, h->stride);
    HIP_CHECK(hipGetLastError());
    // recycle old slabs fully behind the window: every old row s maps to
    // new pos >= its old pos, so old pos < j1 - n_pend are consumed
    if (h->csr_arena.rlog == next.rlog) {
      int64_t consumed = j1 - n_pend;
      bool freed_any = false;
      while ((int64_t)((old_free_cursor + 1) << next.rlog) <= consumed &&
             old_free_cursor < h->csr_arena.slabs.size()) {
        if (!freed_any) {
          HIP_CHECK(hipStreamSynchronize(stream));
          freed_any = true;
        }
        h->csr_arena.free_slab(old_free_cursor++);
      }
    }
  }
  HIP_CHECK(hipStreamSynchronize(stream));
  h->csr_arena.reset();
  std::swap(h->csr_arena.stride, next.stride);
  std::swap(h->csr_arena.rlog, next.rlog);
  std::swap(h->csr_arena.slabs, next.slabs);
  h->csr_arena.rows = n_new;
  h->csr_arena.table_dirty = true;
  next.rows = 0;
  h->pend_arena.reset();
  h->pend_arena.init(h->stride, h->csr_arena.slab_bytes());
  h->h_pend_assign.clear();
  h->csr_rows = n_new;
  // swap id arrays (DevBuf members)
  std::swap(h->cr_ids.p, h->cr_ids_new.p);
  std::swap(h->cr_ids.cap, h->cr_ids_new.cap);
  h->h_off = new_off;
  h->cr_off.ensure((size_t)(h->nlist + 1) * 8);
  HIP_CHECK(hipMemcpy(h->cr_off.p, h->h_off.data(), (size_t)(h->nlist + 1) * 8,
                      hipMemcpyHostToDevice));
  h->dirty = false;
}

// encode a chunk of rows into the pending arena at rows [row0, row0+n)
static void encode_chunk(dfann_index *h, int64_t n, const float *x,
                         const int *asg, int64_t row0, hipStream_t stream) {
  h->pend_arena.ensure_rows(row0 + n);
  uint8_t *const *dst = h->pend_arena.dev_table_mut(stream);
  int rlog = h->pend_arena.rlog;
  if (h->type == T_IVFFLAT) {
    hipLaunchKernelGGL(k_pack_rows, grid1d(n * h->d), dim3(256), 0, stream, x,
                       n, h->d, h->stride, rlog, row0, dst);
    return;
  }
  DevBuf resid;
  resid.ensure((size_t)n * h->d * 4);
  hipLaunchKernelGGL(k_residual, grid1d(n * h->d), dim3(256), 0, stream, x,
                     h->centroids.as<float>(), asg, n, h->d,
                     resid.as<float>());
  if (h->type == T_IVFPQ) {
    // per-subspace encode as a distance GEMM + running argmin (~20x a
    // naive per-thread 256-way argmin kernel)
    DevBuf sub, best, bestv, cbn;
    sub.ensure((size_t)n * h->dsub * 4);
    best.ensure((size_t)n * 4);
    bestv.ensure((size_t)n * 4);
    const int ksub = pq_ksub(h);
    cbn.ensure(ksub * 4);
    int64_t chunk = std::max<int64_t>(1, ((int64_t)h->ws_mb << 20) / (ksub * 4));
    chunk = std::min<int64_t>(chunk, n);
    h->ws1.ensure((size_t)chunk * ksub * 4);
    for (int j = 0; j < h->m; ++j) {
      hipLaunchKernelGGL(k_subspace_slice, grid1d(n * h->dsub), dim3(256), 0,
                         stream, resid.as<float>(), n, h->d, j * h->dsub,
                         h->dsub, sub.as<float>());
      const float *cbj = h->codebooks.as<float>() + (size_t)j * ksub * h->dsub;
      rownorms(cbj, ksub, h->dsub, cbn.as<float>(), stream);
      hipLaunchKernelGGL(k_assign_init, grid1d(n), dim3(256), 0, stream,
                         bestv.as<float>(), best.as<int>(), n);
      for (int64_t s0 = 0; s0 < n; s0 += chunk) {
        int64_t c = std::min(chunk, n - s0);
        gemm_keys(nullptr, sub.as<float>() + s0 * h->dsub, c, cbj, ksub,
                  h->dsub, cbn.as<float>(), nullptr, 1, h->ws1.as<float>(),
                  stream);
        hipLaunchKernelGGL(k_assign_rowblock, dim3((unsigned)c), dim3(256), 0,
                           stream, h->ws1.as<float>(), c, (long long)ksub,
                           (long long)ksub, 0, bestv.as<float>() + s0,
                           best.as<int>() + s0);
      }
      hipLaunchKernelGGL(h->nbits == 4 ? k_codes_from_best4 : k_codes_from_best,
                         grid1d(n), dim3(256), 0, stream, best.as<int>(), n, j,
                         h->stride, rlog, row0, dst);
    }
  } else {
    hipLaunchKernelGGL(k_sq_encode,
                       grid1d(n * sq_encode_items(h->sq_bits, h->d, h->stride)),
                       dim3(256), 0, stream, resid.as<float>(),
                       h->sq_int() ? h->sq_vmin.as<float>() : nullptr,
                       h->sq_int() ? h->sq_vdiff.as<float>() : nullptr, n, h->d,
                       h->stride, h->sq_bits, rlog, row0, dst);
  }
  HIP_CHECK(hipGetLastError());
}

static void hnsw_add(dfann_index *h, int64_t n, const float *x,
                     hipStream_t stream);

// append n raw rows to the refine store at rows [ntotal, ntotal+n), in
// arrival order on the caller's stream (the caller bumps ntotal after)
static void refine_append(dfann_index *h, int64_t n, const float *x,
                          hipStream_t stream) {
  SlabArena &ra = h->refine_arena;
  const int64_t row0 = h->ntotal;
  ra.ensure_rows(row0 + n);
  // refreshed here (it synchronizes when a slab was added) so that no
  // search ever has to
  uint8_t *const *tab = ra.dev_table_mut(stream);
  if (h->refine == 2) {
    hipLaunchKernelGGL(k_refine_store_f16, grid1d(n * h->d_in), dim3(256), 0,
                       stream, x, (long long)n, h->d_in, ra.stride, ra.rlog,
                       (long long)row0, tab);
  } else if (ra.stride == 4 * h->d_in) {
    // fp32 rows with no pad: device-to-device copies, one per slab touched
    int64_t r = row0, left = n;
    const float *src = x;
    while (left > 0) {
      int64_t in_slab = std::min<int64_t>(left, ra.rps() - (r & (ra.rps() - 1)));
      char *dst = (char *)ra.slabs[r >> ra.rlog] +
                  (size_t)(r & (ra.rps() - 1)) * ra.stride;
      HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)in_slab * ra.stride,
                               hipMemcpyDeviceToDevice, stream));
      src += in_slab * h->d_in;
      r += in_slab;
      left -= in_slab;
    }
  } else {
    // d % 4 != 0: rows are padded to 16 B, so the copy is strided
    hipLaunchKernelGGL(k_pack_rows, grid1d(n * h->d_in), dim3(256), 0, stream, x,
                       (long long)n, h->d_in, ra.stride, ra.rlog, (long long)row0,
                       tab);
  }
  HIP_CHECK(hipGetLastError());
  ra.rows = row0 + n;
}

// flat tombstones: bring the live bitmap up to ntotal ids, ids from `from`
// on live, and refresh the device copy. The host mirror is the master.
static void flat_live_extend(dfann_index *h, int64_t from) {
  const size_t words = (size_t)((h->ntotal + 31) / 32);
  h->h_flat_live.resize(words, 0u);
  for (int64_t i = from; i < h->ntotal; ++i)
    h->h_flat_live[(size_t)(i >> 5)] |= 1u << (unsigned)(i & 31);
  h->flat_live.grow_keep(std::max(words * 4, (size_t)16), 0);
  if (words)
    HIP_CHECK(hipMemcpy(h->flat_live.p, h->h_flat_live.data(), words * 4,
                        hipMemcpyHostToDevice));
}

static void add_impl(dfann_index *h, int64_t n, const float *x,
                     hipStream_t stream) {
  if (!h->trained) throw std::runtime_error("add on untrained index");
  if (n == 0) return;
  if (h->opq) opq_require(h);
  if (h->type == T_HNSW) { hnsw_add(h, n, x, stream); return; }
  if (h->type == T_FLAT) {
    h->flat.grow_keep(((size_t)h->ntotal + n) * h->d * 4,
                      (size_t)h->ntotal * h->d * 4);
    HIP_CHECK(hipMemcpyAsync(h->flat.as<float>() + (size_t)h->ntotal * h->d, x,
                             (size_t)n * h->d * 4, hipMemcpyDeviceToDevice,
                             stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    h->ntotal += n;
    if (h->nremoved) flat_live_extend(h, h->ntotal - n);
    return;
  }
  // internal chunking: bounds the residual/assign transients for huge
  // ingests (a 125M x 128 add would otherwise stage a 64 GB fp32
  // residual buffer)
  const int64_t CH = std::max<int64_t>(
      65536, ((int64_t)h->ws_mb << 20) / std::max(4 * h->d, 1));
  DevBuf asg;
  std::vector<int32_t> h_asg;
  for (int64_t s = 0; s < n; s += CH) {
    int64_t c = std::min(CH, n - s);
    asg.ensure((size_t)c * 4);
    // OPQ: the chunk at d_out; the refine store keeps the raw d_in rows
    const float *xs = x + s * h->d_in;
    const float *xi = xs;
    if (h->opq) {
      h->opq_x.ensure((size_t)c * h->d * 4);
      run_transform(h, h->opq_A.as<float>(), c, xs, h->d_in, h->d,
                    h->opq_x.as<float>(), stream);
      xi = h->opq_x.as<float>();
    }
    assign_rows(h, xi, c, asg.as<int>(), stream);
    // The host copy of the assignments comes first: a row without a list
    // (-1: a NaN row, or products that overflow) refuses the whole chunk
    // before k_residual indexes a centroid by it and before rebuild_csr
    // counts it. Nothing of the chunk is stored; earlier chunks stay.
    h_asg.resize((size_t)c);
    HIP_CHECK(hipMemcpyAsync(h_asg.data(), asg.p, (size_t)c * 4,
                             hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    for (int64_t i = 0; i < c; ++i)
      if ((uint32_t)h_asg[i] >= (uint32_t)h->nlist)
        throw std::runtime_error(
            "add: row " + std::to_string(s + i) +
            " of the batch has no nearest centroid (NaN, or values too "
            "large for fp32 distances); rows from " + std::to_string(s) +
            " on were not added");
    int64_t row0 = (int64_t)h->h_pend_assign.size();
    encode_chunk(h, c, xi, asg.as<int>(), row0, stream);
    if (h->refine) refine_append(h, c, xs, stream);
    h->h_pend_assign.insert(h->h_pend_assign.end(), h_asg.begin(),
                            h_asg.end());
    HIP_CHECK(hipStreamSynchronize(stream));
    h->ntotal += c;
    h->dirty = true;
    // incremental merge: bounds the pending arena (and so the rebuild
    // transient) to ~merge_mb
    if ((int64_t)h->h_pend_assign.size() * h->stride >=
        ((int64_t)h->merge_mb << 20))
      rebuild_csr(h, stream);
  }
}

static void finalize_csr(dfann_index *h, hipStream_t stream) {
  rebuild_csr(h, stream);
}


// ---------------------------------------------------------------------------
// HNSW host orchestration (type "hnswsq")
// ---------------------------------------------------------------------------

// deterministic level draw (splitmix64; clamped). Restated by the oracle
// (oracle/hnsw.py hnsw_draw_level); M >= 2 is enforced at create.
static int hnsw_draw_level(uint64_t seed, int64_t id, int M) {
  SplitMix64 rng(seed ^ (uint64_t)(id * 0x9E3779B97F4A7C15ULL + 0x51ED2701ULL));
  double u = ((double)(rng.next() >> 11) + 1.0) * (1.0 / 9007199254740992.0);
  double mL = 1.0 / log((double)M);
  int l = (int)floor(-log(u) * mL);
  if (l < 0) l = 0;
  if (l > HNSW_MAXL) l = HNSW_MAXL;
  return l;
}

// drain + apply the reverse-link requests of one insertion wave in
// (dst, level, src) sorted order (deterministic)
static void hnsw_apply_reqs(dfann_index *h, hipStream_t stream,
                            size_t lds_apply, int64_t req_cap) {
  const int M = h->m, deg0 = 2 * h->m;
  int rcnt = 0;
  HIP_CHECK(hipMemcpyAsync(&rcnt, h->hn_reqcnt.p, 4, hipMemcpyDeviceToHost,
                           stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  if (rcnt > req_cap)
    throw std::runtime_error("hnsw: reverse-link buffer overflow");
  if (rcnt <= 0) return;
  std::vector<int> hreq((size_t)rcnt * 4);
  HIP_CHECK(hipMemcpy(hreq.data(), h->hn_req.p, (size_t)rcnt * 16,
                      hipMemcpyDeviceToHost));
  std::vector<int64_t> order(rcnt);
  for (int i = 0; i < rcnt; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
    const int *ra = &hreq[(size_t)a * 4], *rb = &hreq[(size_t)b * 4];
    if (ra[0] != rb[0]) return ra[0] < rb[0];
    if (ra[2] != rb[2]) return ra[2] < rb[2];
    return ra[1] < rb[1];
  });
  std::vector<int> sorted((size_t)rcnt * 4);
  std::vector<int> runoff;
  for (int i = 0; i < rcnt; ++i) {
    const int *r = &hreq[(size_t)order[i] * 4];
    if (i == 0 || r[0] != sorted[(size_t)(i - 1) * 4] ||
        r[2] != sorted[(size_t)(i - 1) * 4 + 2])
      runoff.push_back(i);
    memcpy(&sorted[(size_t)i * 4], r, 16);
  }
  runoff.push_back(rcnt);
  int n_runs = (int)runoff.size() - 1;
  HIP_CHECK(hipMemcpy(h->hn_req.p, sorted.data(), (size_t)rcnt * 16,
                      hipMemcpyHostToDevice));
  h->hn_runoff.ensure(runoff.size() * 4);
  HIP_CHECK(hipMemcpy(h->hn_runoff.p, runoff.data(), runoff.size() * 4,
                      hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_hnsw_apply, dim3((unsigned)n_runs), dim3(256),
                     lds_apply, stream, h->sq_scale.as<float>(),
                     h->csr_arena.dev_table(stream), h->csr_arena.rlog,
                     h->stride, h->d, h->hn_nbr0.as<int>(),
                     h->hn_cnt0.as<int>(), h->hn_upslot.as<int>(),
                     h->hn_nbrU.as<int>(), h->hn_cntU.as<int>(), deg0, M,
                     h->hn_req.as<int>(), h->hn_runoff.as<int>(), n_runs);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(stream));
}

static void hnsw_add(dfann_index *h, int64_t n, const float *x,
                     hipStream_t stream) {
  const int M = h->m, deg0 = 2 * h->m;
  const int64_t n0 = h->ntotal, ntot = n0 + n;
  // A non-finite row would insert with NaN distances: an empty beam, so a
  // node without links, and once its level makes it the entry point every
  // later insert and query starts from that isolated node. Refused whole.
  if (const char *cls = nonfinite_class(h, x, n * h->d, stream))
    throw std::runtime_error(
        std::string("add: the batch holds a non-finite value (") + cls +
        "); hnswsq adds no row of it");
  // 1) encode rows [n0, ntot) into the code arena (arrival order; the
  //    HNSW arena is never rebuilt — ids ARE row positions)
  h->csr_arena.ensure_rows(ntot);
  {
    const int64_t CH = std::max<int64_t>(
        65536, ((int64_t)h->ws_mb << 20) / std::max(4 * h->d, 1));
    for (int64_t s0 = 0; s0 < n; s0 += CH) {
      int64_t c = std::min(CH, n - s0);
      hipLaunchKernelGGL(k_sq_encode, grid1d(c * h->d), dim3(256), 0, stream,
                         x + s0 * h->d, h->sq_vmin.as<float>(),
                         h->sq_vdiff.as<float>(), c, h->d, h->stride, 8,
                         h->csr_arena.rlog, n0 + s0,
                         h->csr_arena.dev_table_mut(stream));
    }
    HIP_CHECK(hipGetLastError());
  }
  // 2) levels + upper slots (host, deterministic)
  h->h_levels.resize(ntot);
  h->h_upslot.resize(ntot);
  int old_nslots = h->hnsw_nslots;
  for (int64_t i = n0; i < ntot; ++i) {
    int lv = hnsw_draw_level(h->seed, i, M);
    h->h_levels[i] = lv;
    h->h_upslot[i] = lv > 0 ? h->hnsw_nslots++ : -1;
  }
  // 3) grow device graph arrays (grow_keep preserves; new ranges zeroed
  //    or uploaded). Graph memory is deg0*4 B/node — the dominant HNSW
  //    cost, same as faiss's links storage.
  h->hn_levels.grow_keep((size_t)ntot * 4, (size_t)n0 * 4);
  HIP_CHECK(hipMemcpyAsync(h->hn_levels.as<int>() + n0,
                           h->h_levels.data() + n0, (size_t)n * 4,
                           hipMemcpyHostToDevice, stream));
  h->hn_upslot.grow_keep((size_t)ntot * 4, (size_t)n0 * 4);
  HIP_CHECK(hipMemcpyAsync(h->hn_upslot.as<int>() + n0,
                           h->h_upslot.data() + n0, (size_t)n * 4,
                           hipMemcpyHostToDevice, stream));
  h->hn_nbr0.grow_keep((size_t)ntot * deg0 * 4, (size_t)n0 * deg0 * 4);
  // -1-fill fresh adjacency: slots beyond each cnt stay deterministic
  // (dump comparisons, persistence) instead of hipMalloc garbage
  HIP_CHECK(hipMemsetAsync(h->hn_nbr0.as<int>() + (size_t)n0 * deg0, 0xFF,
                           (size_t)n * deg0 * 4, stream));
  h->hn_cnt0.grow_keep((size_t)ntot * 4, (size_t)n0 * 4);
  HIP_CHECK(hipMemsetAsync(h->hn_cnt0.as<int>() + n0, 0, (size_t)n * 4,
                           stream));
  if (h->hnsw_nslots > old_nslots) {
    h->hn_nbrU.grow_keep((size_t)h->hnsw_nslots * HNSW_MAXL * M * 4,
                         (size_t)old_nslots * HNSW_MAXL * M * 4);
    HIP_CHECK(hipMemsetAsync(
        h->hn_nbrU.as<int>() + (size_t)old_nslots * HNSW_MAXL * M, 0xFF,
        (size_t)(h->hnsw_nslots - old_nslots) * HNSW_MAXL * M * 4, stream));
    h->hn_cntU.grow_keep((size_t)h->hnsw_nslots * HNSW_MAXL * 4,
                         (size_t)old_nslots * HNSW_MAXL * 4);
    HIP_CHECK(hipMemsetAsync(
        h->hn_cntU.as<int>() + (size_t)old_nslots * HNSW_MAXL, 0,
        (size_t)(h->hnsw_nslots - old_nslots) * HNSW_MAXL * 4, stream));
  }
  // 4) wave insertion over frozen snapshots
  const int64_t WMAX = 4096;
  // x2: the refine pass queues both directions per kept link
  const int64_t req_cap = 2 * WMAX * M * (HNSW_MAXL + 1);
  h->hn_req.ensure((size_t)req_cap * 16);
  h->hn_reqcnt.ensure(4);
  h->hn_u.ensure((size_t)WMAX * h->d * 4);
  size_t lds_ins = HNSW_LDS_INS(h->d, 256);
  size_t lds_apply = HNSW_LDS_APPLY(h->d);
  std::vector<int> hreq;
  std::vector<int64_t> order;
  std::vector<int> runoff;
  int64_t w0 = n0;
  while (w0 < ntot) {
    if (h->hnsw_entry < 0) {  // very first point
      h->hnsw_entry = 0;
      h->hnsw_maxlevel = h->h_levels[0];
    }
    int64_t W = w0 == 0
                    ? 1
                    : std::min<int64_t>(
                          std::min(WMAX, std::max<int64_t>(256, w0 / 8)),
                          ntot - w0);
    W = std::min(W, ntot - w0);
    hipLaunchKernelGGL(k_hnsw_prep, grid1d(W * h->d), dim3(256), 0, stream,
                       x + (w0 - n0) * h->d, h->sq_vmin.as<float>(),
                       h->sq_scale.as<float>(), W, h->d, h->hn_u.as<float>());
    HIP_CHECK(hipMemsetAsync(h->hn_reqcnt.p, 0, 4, stream));
    hipLaunchKernelGGL(k_hnsw_insert, dim3((unsigned)W), dim3(256), lds_ins,
                       stream, h->hn_u.as<float>(), h->sq_scale.as<float>(),
                       h->csr_arena.dev_table(stream), h->csr_arena.rlog,
                       h->stride, h->d, h->hn_levels.as<int>(),
                       h->hn_nbr0.as<int>(), h->hn_cnt0.as<int>(),
                       h->hn_upslot.as<int>(), h->hn_nbrU.as<int>(),
                       h->hn_cntU.as<int>(), deg0, M, w0, h->hnsw_entry,
                       h->hnsw_maxlevel, w0, (int)W, h->hnsw_efc,
                       h->hn_req.as<int>(), h->hn_reqcnt.as<int>(),
                       (int)req_cap, 0, (const int *)nullptr,
                       (const int *)nullptr, (const int *)nullptr,
                       (const int *)nullptr);
    HIP_CHECK(hipGetLastError());
    hnsw_apply_reqs(h, stream, lds_apply, req_cap);
    // entry update: highest new level (lowest id on ties) beats the old
    for (int64_t i = w0; i < w0 + W; ++i)
      if (h->h_levels[i] > h->hnsw_maxlevel) {
        h->hnsw_maxlevel = h->h_levels[i];
        h->hnsw_entry = (int)i;
      }
    w0 += W;
  }
  h->csr_arena.rows = ntot;
  h->ntotal = ntot;
  // REFINEMENT pass: re-link every new point over the
  // FINAL graph — the initial waves insert over stale snapshots (a
  // point cannot link to its own wave, and early points saw a tiny
  // graph). One extra pass raises mean degree and recall substantially
  // (measured in scripts/hnsw_diag.py); deterministic: fixed wave order
  // over the evolving-but-deterministic graph. spec "hnsw_refine" = 0
  // disables.
  if (json_int(h->spec_json, "hnsw_refine", 1) != 0) {
    // freeze the pre-refine graph: refine blocks traverse the copy
    // while own-link writes and reverse-link merges go to the live
    // arrays — race-free and deterministic
    DevBuf fz_nbr0, fz_cnt0, fz_nbrU, fz_cntU;
    fz_nbr0.ensure((size_t)ntot * deg0 * 4);
    fz_cnt0.ensure((size_t)ntot * 4);
    HIP_CHECK(hipMemcpyAsync(fz_nbr0.p, h->hn_nbr0.p, (size_t)ntot * deg0 * 4,
                             hipMemcpyDeviceToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(fz_cnt0.p, h->hn_cnt0.p, (size_t)ntot * 4,
                             hipMemcpyDeviceToDevice, stream));
    if (h->hnsw_nslots) {
      fz_nbrU.ensure((size_t)h->hnsw_nslots * HNSW_MAXL * M * 4);
      fz_cntU.ensure((size_t)h->hnsw_nslots * HNSW_MAXL * 4);
      HIP_CHECK(hipMemcpyAsync(fz_nbrU.p, h->hn_nbrU.p,
                               (size_t)h->hnsw_nslots * HNSW_MAXL * M * 4,
                               hipMemcpyDeviceToDevice, stream));
      HIP_CHECK(hipMemcpyAsync(fz_cntU.p, h->hn_cntU.p,
                               (size_t)h->hnsw_nslots * HNSW_MAXL * 4,
                               hipMemcpyDeviceToDevice, stream));
    } else {
      fz_nbrU.ensure(16);
      fz_cntU.ensure(16);
    }
    int64_t r0 = n0;
    while (r0 < ntot) {
      int64_t W = std::min<int64_t>(WMAX, ntot - r0);
      hipLaunchKernelGGL(k_hnsw_prep, grid1d(W * h->d), dim3(256), 0, stream,
                         x + (r0 - n0) * h->d, h->sq_vmin.as<float>(),
                         h->sq_scale.as<float>(), W, h->d,
                         h->hn_u.as<float>());
      HIP_CHECK(hipMemsetAsync(h->hn_reqcnt.p, 0, 4, stream));
      hipLaunchKernelGGL(k_hnsw_insert, dim3((unsigned)W), dim3(256), lds_ins,
                         stream, h->hn_u.as<float>(), h->sq_scale.as<float>(),
                         h->csr_arena.dev_table(stream), h->csr_arena.rlog,
                         h->stride, h->d, h->hn_levels.as<int>(),
                         h->hn_nbr0.as<int>(), h->hn_cnt0.as<int>(),
                         h->hn_upslot.as<int>(), h->hn_nbrU.as<int>(),
                         h->hn_cntU.as<int>(), deg0, M, ntot, h->hnsw_entry,
                         h->hnsw_maxlevel, r0, (int)W, h->hnsw_efc,
                         h->hn_req.as<int>(), h->hn_reqcnt.as<int>(),
                         (int)req_cap, 1, fz_nbr0.as<const int>(),
                         fz_cnt0.as<const int>(), fz_nbrU.as<const int>(),
                         fz_cntU.as<const int>());
      HIP_CHECK(hipGetLastError());
      hnsw_apply_reqs(h, stream, lds_apply, req_cap);
      r0 += W;
    }
  }
}

static void hnsw_search(dfann_index *h, int64_t nq, const float *q, int k,
                        float *D, int64_t *I, hipStream_t stream) {
  int ef = std::max(h->nprobe, k);
  if (ef > 512) ef = 512;
  h->hn_u.ensure((size_t)nq * h->d * 4);
  hipLaunchKernelGGL(k_hnsw_prep, grid1d(nq * h->d), dim3(256), 0, stream, q,
                     h->sq_vmin.as<float>(), h->sq_scale.as<float>(), nq, h->d,
                     h->hn_u.as<float>());
  TimingEv e;
  if (h->timing) e = h->ev_begin(stream);
  hipLaunchKernelGGL(k_hnsw_search, dim3((unsigned)nq), dim3(256),
                     HNSW_LDS(h->d, 256), stream, h->hn_u.as<float>(),
                     h->sq_scale.as<float>(), h->csr_arena.dev_table(stream),
                     h->csr_arena.rlog, h->stride, h->d,
                     h->hn_levels.as<int>(), h->hn_nbr0.as<int>(),
                     h->hn_cnt0.as<int>(), h->hn_upslot.as<int>(),
                     h->hn_nbrU.as<int>(), h->hn_cntU.as<int>(), 2 * h->m,
                     h->m, h->ntotal, h->hnsw_entry, h->hnsw_maxlevel, nq, ef,
                     k, D, I);
  if (h->timing) h->ev_end(e, stream, h->ev_scan);
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// search
// ---------------------------------------------------------------------------

// Top-k of each row of a (rows x cols) key matrix into out_d / out_p (row
// stride ldo, positions offset by `base`): register path for k <= 16
// (bs_rk threads), LDS-buffer selection otherwise (256, Sel capacity is
// sized for it). allow != nullptr: the filtered twins.
static void launch_topk_rows(hipStream_t stream, unsigned bs_rk,
                             const float *keys, int64_t rows, int64_t cols,
                             int k, unsigned base, int64_t ldo, float *out_d,
                             unsigned *out_p, const uint32_t *allow) {
  bool rk = use_regsel(k);
  dim3 g((unsigned)rows), b(rk ? bs_rk : 256u);
  size_t lds = rk ? REGSEL_LDS_BYTES : SEL_LDS_BYTES;
  if (allow)
    hipLaunchKernelGGL(rk ? k_topk_rows_rk_f : k_topk_rows_f, g, b, lds,
                       stream, keys, (long long)rows, (long long)cols,
                       (long long)cols, k, base, (long long)ldo, out_d, out_p,
                       allow);
  else
    hipLaunchKernelGGL(rk ? k_topk_rows_rk : k_topk_rows, g, b, lds, stream,
                       keys, (long long)rows, (long long)cols, (long long)cols,
                       k, base, (long long)ldo, out_d, out_p);
}

// Merge C candidates per query into the final top-k (D, I). ids maps
// positions to ids (nullptr: positions are the ids). first: see
// merge_launch.
static void launch_merge_cand(hipStream_t stream, const float *cand_d,
                              const unsigned *cand_p, int64_t nq, int C, int k,
                              const int64_t *ids, bool ip, float *D,
                              int64_t *I, MergePath first) {
  const MergeLaunch m = merge_launch(nq, k, C, first);
  auto kern = m.path == MERGE_WAVE ? k_merge_cand_w
              : m.path == MERGE_RK ? k_merge_cand_rk
                                   : k_merge_cand;
  hipLaunchKernelGGL(kern, m.grid, dim3(256), m.lds, stream, cand_d, cand_p,
                     nq, C, k, ids, ip ? 1 : 0, D, I);
}

static void pad_fill(dfann_index *h, int64_t nq, int k, float *D, int64_t *I,
                     hipStream_t stream) {
  // empty index: all pads — the LDS merge kernel on zero candidates
  launch_merge_cand(stream, nullptr, nullptr, nq, 0, k, nullptr,
                    h->metric == M_IP, D, I, MERGE_LDS);
  HIP_CHECK(hipGetLastError());
}

// Fused coarse path: k_gemm_bf16_256_topk keeps the NP (nprobe rounded up
// to a power of two) best (key, list) pairs per row and 256-column tile,
// k_coarse_reduce_rk picks the final nprobe. No nq x nlist score matrix:
// ws1 holds the candidates, nq * n_tile * NP * 8 bytes, and all queries
// go in one launch. Taken for the shapes that reach k_gemm_bf16_256 with
// a register-path nprobe; DFANN_COARSE_FUSED=0 (A/B knob) keeps the
// two-pass path.
static bool coarse_fused_ok(const dfann_index *h, int64_t nq, int nprobe) {
  if (const char *e = getenv("DFANN_COARSE_FUSED"))  // experiment override
    if (atoi(e) == 0) return false;
  int K = h->d;
  return h->coarse_bf16 && h->cent_bf16.p && K % 8 == 0 && h->nlist >= 2048 &&
         nq >= 256 && K >= 64 && use_regsel(nprobe);
}

template <int NP>
static void launch_gemm_topk(dim3 g, hipStream_t stream,
                             const unsigned short *A, const unsigned short *B,
                             int M, int N, int K, const float *bn, int mode,
                             float *cand_d, unsigned *cand_p) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gemm_bf16_256_topk<NP>), g, dim3(512),
                     0, stream, A, B, M, N, K, K, K, (const float *)nullptr,
                     bn, mode, cand_d, cand_p);
}

static void coarse_fused(dfann_index *h, int64_t nq, const float *q,
                         int nprobe, int32_t *probes, float *keys,
                         hipStream_t stream) {
  int nlist = h->nlist, K = h->d;
  int np = 1;
  while (np < nprobe) np <<= 1;
  int n_tile = (nlist + 255) / 256;
  int ncand = n_tile * np;
  h->ws1.ensure((size_t)nq * ncand * 8);
  float *cand_d = h->ws1.as<float>();
  unsigned *cand_p = reinterpret_cast<unsigned *>(cand_d + (size_t)nq * ncand);
  h->ws_bf16a.ensure((size_t)nq * K * 2);
  const unsigned short *A = h->ws_bf16a.as<unsigned short>();
  const unsigned short *B = h->cent_bf16.as<unsigned short>();
  const float *bn = h->cnorm.as<float>();
  int mode = h->metric == M_IP ? 0 : 1;
  dim3 g((unsigned)n_tile, (unsigned)((nq + 255) / 256));
  TimingEv e;
  if (h->timing) e = h->ev_begin(stream);
  hipLaunchKernelGGL(k_f32_to_bf16, grid1d(nq * K), dim3(256), 0, stream, q,
                     nq * K, h->ws_bf16a.as<unsigned short>());
  switch (np) {
    case 1: launch_gemm_topk<1>(g, stream, A, B, (int)nq, nlist, K, bn, mode, cand_d, cand_p); break;
    case 2: launch_gemm_topk<2>(g, stream, A, B, (int)nq, nlist, K, bn, mode, cand_d, cand_p); break;
    case 4: launch_gemm_topk<4>(g, stream, A, B, (int)nq, nlist, K, bn, mode, cand_d, cand_p); break;
    case 8: launch_gemm_topk<8>(g, stream, A, B, (int)nq, nlist, K, bn, mode, cand_d, cand_p); break;
    default: launch_gemm_topk<16>(g, stream, A, B, (int)nq, nlist, K, bn, mode, cand_d, cand_p); break;
  }
  if (h->timing) {
    h->ev_end(e, stream, h->ev_gemm);
    h->gemm_flops += 2LL * nq * nlist * K;
  }
  unsigned bs = ncand <= 256 ? 64 : ncand <= 1024 ? 128 : 256;
  hipLaunchKernelGGL(k_coarse_reduce_rk, dim3((unsigned)nq), dim3(bs),
                     REGSEL_LDS_BYTES, stream, cand_d, cand_p, (long long)nq,
                     ncand, nprobe, keys, reinterpret_cast<unsigned *>(probes));
  HIP_CHECK(hipGetLastError());
}

static void coarse_impl(dfann_index *h, int64_t nq, const float *q, int nprobe,
                        int32_t *probes, float *keys, hipStream_t stream) {
  if (coarse_fused_ok(h, nq, nprobe)) {
    coarse_fused(h, nq, q, nprobe, probes, keys, stream);
    return;
  }
  int nlist = h->nlist;
  int64_t chunk = std::max<int64_t>(1, ((int64_t)h->ws_mb << 20) / ((int64_t)nlist * 4));
  chunk = std::min<int64_t>(chunk, nq);
  h->ws1.ensure((size_t)chunk * nlist * 4);
  float *sc = h->ws1.as<float>();
  for (int64_t s = 0; s < nq; s += chunk) {
    int64_t c = std::min(chunk, nq - s);
    gemm_keys_b(h, q + s * h->d, c, h->centroids.as<float>(),
                h->cent_bf16.as<unsigned short>(), nlist, h->d,
                h->cnorm.as<float>(), nullptr, h->metric == M_IP ? 0 : 1, sc,
                stream);
    // 256 measured best (128 is -3%: this kernel is one streaming
    // phase — no phase diversity to recover, unlike the scans)
    unsigned tk_bs = 256;
    if (const char *e = getenv("DFANN_TOPK_BS"))  // experiment override
      if (int v = atoi(e)) tk_bs = (unsigned)((v / 64) * 64);
    launch_topk_rows(stream, tk_bs, sc, c, nlist, nprobe, 0u, nprobe,
                     keys + s * nprobe,
                     reinterpret_cast<unsigned *>(probes) + s * nprobe,
                     nullptr);
  }
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// The inverted-list scan: plan_scan picks mode and launch geometry from
// the index, scan_kernel maps (mode, metric, selector, filtered) to the
// kernel, scan_and_merge fills one ScanArgs and launches it. The mode
// list is DFANN_SCAN_MODES (kernels.hip).
// ---------------------------------------------------------------------------

#define DFANN_SCAN_ENUM(MODE, ...) SCAN_##MODE,
enum ScanMode { DFANN_SCAN_MODES(DFANN_SCAN_ENUM, DFANN_SCAN_ENUM) };
#undef DFANN_SCAN_ENUM

typedef void (*scan_kern_t)(ScanArgs);
struct ScanKernels {
  const char *mode;
  scan_kern_t fn[2][2][2];  // [ip][rk][filt]
  scan_kern_t range_fn[2][2];  // [ip][filt]
};
#define DFANN_SCAN_FNS(NAME, MET, SUFFIX)                                      \
  {{k_scan_##NAME##_##MET##SUFFIX, k_scan_##NAME##_##MET##SUFFIX##_f},         \
   {k_scan_##NAME##_##MET##SUFFIX##_rk, k_scan_##NAME##_##MET##SUFFIX##_rk_f}}
#define DFANN_SCAN_RFNS(NAME, MET, SUFFIX)                                     \
  {k_scan_##NAME##_##MET##SUFFIX##_rg, k_scan_##NAME##_##MET##SUFFIX##_rg_f}
#define DFANN_SCAN_ROW(MODE, NAME, SUFFIX, ...)                                \
  {#MODE,                                                                      \
   {DFANN_SCAN_FNS(NAME, l2, SUFFIX), DFANN_SCAN_FNS(NAME, ip, SUFFIX)},       \
   {DFANN_SCAN_RFNS(NAME, l2, SUFFIX), DFANN_SCAN_RFNS(NAME, ip, SUFFIX)}},
#define DFANN_SCAN_ROW_L2(MODE, NAME, SUFFIX, ...)                             \
  {#MODE, {DFANN_SCAN_FNS(NAME, l2, SUFFIX), {}},                              \
   {DFANN_SCAN_RFNS(NAME, l2, SUFFIX), {}}},
static const ScanKernels SCAN_KERNELS[] = {
    DFANN_SCAN_MODES(DFANN_SCAN_ROW, DFANN_SCAN_ROW_L2)};
#undef DFANN_SCAN_ROW_L2
#undef DFANN_SCAN_ROW
#undef DFANN_SCAN_RFNS
#undef DFANN_SCAN_FNS

static scan_kern_t scan_kernel(ScanMode mode, bool ip, bool rk, bool filt,
                               bool range = false) {
  const ScanKernels &row = SCAN_KERNELS[mode];
  scan_kern_t fn = range ? row.range_fn[ip][filt] : row.fn[ip][rk][filt];
  if (!fn)
    throw std::runtime_error(std::string("no scan kernel for mode ") +
                             row.mode + (ip ? " ip" : " l2") +
                             (range ? " range" : rk ? " rk" : "") +
                             (filt ? " filtered" : ""));
  return fn;
}

struct ScanPlan {
  ScanMode mode;
  int fam_floats;    // staged query terms / LUT per block, in FLOAT units
  size_t lds;        // dynamic LDS per block
  unsigned scan_bs;  // threads per block
  int fan;           // list segments per (query, probe)
  bool lut_f16;      // GLUT rows are __half
  int64_t glut_qch;  // GLUT: queries per LUT chunk (not clamped to nq)
};

// range: the range kernels — no selector LDS, never a
// list fan, block size by the register path's rule (k is ignored)
static ScanPlan plan_scan(const dfann_index *h, int k, int nprobe,
                          bool range = false) {
  ScanPlan p;
  bool rk = range || use_regsel(k);
  switch (h->type) {
    case T_IVFPQ:
      if (h->nbits == 4) {
        p.mode = SCAN_PQ4;
        p.fam_floats = h->m * 16 + h->d;
      } else {
        p.mode = SCAN_PQ;
        p.fam_floats = h->m * 256 + h->d;
      }
      break;
    case T_IVFFLAT:
      p.mode = SCAN_IVFFLAT;
      p.fam_floats = h->d;
      break;
    case T_IVFSQ:
      p.mode = h->sq_bits == 8   ? SCAN_SQ8
               : h->sq_bits == 6 ? SCAN_SQ6
               : h->sq_bits == 4 ? SCAN_SQ4
                                 : SCAN_SQF;
      p.fam_floats = h->sq_int() ? 2 * h->d : h->d;
      break;
    default:
      throw std::runtime_error("scan on flat index");
  }
  // nbits=4 has the in-kernel fp32 LUT only: the PRE / GLUT / fp16 paths
  // and their env overrides below do not apply to it
  const bool pq8 = h->type == T_IVFPQ && h->nbits == 8;
  bool use_pre = pq8 && h->metric == M_L2 && h->pq_pre && h->term2.p;
  if (use_pre) {
    p.mode = SCAN_PQ_PRE;
    p.fam_floats = h->m * 256;  // LUT only, no rbuf
  }
  // GLUT path: LUTs built once to HBM by k_pq_lut, scan stages them as
  // coalesced float4 slabs. The in-kernel build re-reads the full
  // m*256*dsub codebook from L2 per (query, probe) block and dominates
  // the launch at large m (measured 8.1 ms/launch at the configs[3]
  // shape, ~125 GB/s of algorithmic code bytes).
  int glut_knob = h->pq_lut_global;
  if (const char *e = getenv("DFANN_PQ_LUT_GLOBAL"))  // experiment override
    glut_knob = atoi(e);
  bool lut_f16 = h->pq_lut_f16;
  if (const char *e = getenv("DFANN_PQ_LUT_F16"))  // experiment override
    lut_f16 = atoi(e) != 0;
  // f32 GLUT measured a wash vs the in-kernel build (BASELINE.md ladder),
  // so auto engages only for the fp16-LUT approximation path where the
  // halved round-trip wins; =1 still forces the f32 variant for A/B.
  bool use_glut = pq8 && !use_pre && h->dsub <= 64 &&
                  (glut_knob == 1 || (glut_knob != 0 && lut_f16));
  p.lut_f16 = lut_f16 && use_glut;
  p.glut_qch = 0;
  if (use_glut) {
    p.mode = p.lut_f16 ? SCAN_PQ_GH : SCAN_PQ_G;
    // LUT only, no rbuf; fam_floats is in FLOAT units
    p.fam_floats = p.lut_f16 ? h->m * 128 : h->m * 256;
    // chunk queries so the LUT buffer stays inside the budget (measured:
    // bigger chunks win — concurrency beats LLC residency)
    size_t row_b =
        (size_t)nprobe * h->m * 256 * (p.lut_f16 ? 2 : 4);  // bytes/query
    int lut_mb = h->pq_lut_mb;
    if (const char *e = getenv("DFANN_PQ_LUT_MB"))  // experiment override
      if (int v = atoi(e)) lut_mb = v;
    int budget_mb = std::min(h->ws_mb, lut_mb);
    p.glut_qch =
        std::max<int64_t>(1, (int64_t)(((size_t)budget_mb << 20) / row_b));
  }
  // segment fan (spec "scan_fan"): kept as an experiment knob — measured
  // NEGATIVE at the 10M SQ8 shape (per-block staging/extraction overhead
  // outweighs tail imbalance: 1936 -> 1339 GB/s at fan 8), so default 1.
  p.fan = (h->type != T_IVFPQ && !range) ? h->scan_fan : 1;
  // REGSEL extract scratch aliases the fam region (used only after the
  // scan, behind a barrier) -> max, not sum (kernels.hip ivf_scan_body)
  p.lds = range ? (size_t)p.fam_floats * 4
          : rk  ? std::max((size_t)p.fam_floats * 4, (size_t)REGSEL_LDS_BYTES)
                : (size_t)p.fam_floats * 4 + SEL_LDS_BYTES;
  if (p.lds > 160 * 1024)
    throw std::runtime_error("scan LDS over budget (m too large)");
  // big-LDS blocks (m=64 LUTs: ~69 KB -> 2 blocks/CU) run 512 threads so
  // the CU still holds 4 waves/SIMD (register path only; the LDS-buffer
  // selection path is capacity-sized for 256)
  // Register-topk scans: SMALL blocks win (measured sweeps, BASELINE.md
  // ladder) — more independent blocks per CU de-correlates the
  // per-block phases (staging burst -> rows -> extract) and keeps the
  // memory system busy (the SQ wait decomposition showed 53% of scan
  // wave cycles parked): 1M f16 GLUT (8 KB LDS) 128 threads =
  // 16 blocks/CU (+27% step); configs[3] f16 (32 KB) 256 = 5 blocks
  // (+8% over 384); SQ8 10M 128 threads +8%. The LDS-buffer selection
  // path keeps 256 (Sel capacity is sized for it).
  p.scan_bs = 256;
  // round-2 addition: SQ scans drop to 64-thread blocks — measured +4%
  // on the config-5 125M SQ8 scan (2075 vs 1991 GB/s, gpurun_out/r2j_*)
  // and +6% at 10M; even more independent per-CU phases than the r1
  // 128-thread finding. IVF-Flat measured −5% at 64 (r2z_ivfflat), so
  // the drop is SQ-only.
  if (rk)
    p.scan_bs = p.lds <= 16 * 1024 ? 128 : (p.lds <= 32 * 1024 ? 256 : 512);
  if (rk && h->type == T_IVFSQ && p.lds <= 4 * 1024) p.scan_bs = 64;
  if (const char *e = getenv("DFANN_SCAN_BS"))  // experiment override
    if (int v = atoi(e)) p.scan_bs = (unsigned)((v / 64) * 64);
  // the range counts workspace holds 8 waves per (query, probe)
  if (range) p.scan_bs = std::min(std::max(p.scan_bs, 64u), 512u);
  return p;
}

struct ScanJob {
  ScanPlan p;
  scan_kern_t kern;
  ScanArgs a;   // everything but the per-chunk pointers
  int64_t qch;  // queries per launch (nq, or the GLUT chunk)
};

// Plan, kernel and the arguments that do not change between launches; the
// filter translate and the PRE per-batch tables run here.
// allow != nullptr: filtered search. The caller's id-space bitmap is
// translated to CSR-position space (k_filter_id2pos, on every call — a
// cache keyed on the caller's pointer would go stale silently) and the
// FILT twins of the scans test one bit per row. Needs a finalized CSR.
static ScanJob scan_prepare(dfann_index *h, int64_t nq, const float *q,
                            int nprobe, int k, hipStream_t stream,
                            const uint32_t *allow, bool range) {
  const bool filt = allow != nullptr;
  const bool ip = h->metric == M_IP;
  ScanJob j;
  j.p = plan_scan(h, k, nprobe, range);
  const ScanPlan &p = j.p;
  j.kern = scan_kernel(p.mode, ip, use_regsel(k), filt, range);
  const bool use_pre = p.mode == SCAN_PQ_PRE;
  const bool use_glut = p.mode == SCAN_PQ_G || p.mode == SCAN_PQ_GH;

  ScanArgs a = {};
  a.cent = h->centroids.as<float>();
  a.cb = h->codebooks.as<float>();
  a.sq_vmin = h->sq_vmin.as<float>();
  a.sq_scale = h->sq_scale.as<float>();
  a.off = h->cr_off.as<int64_t>();
  a.nlist = h->nlist;
  a.nprobe = nprobe;
  a.d = h->d;
  a.m = h->m;
  a.dsub = h->dsub;
  a.k = k;
  a.stride = h->stride;
  a.rlog = h->csr_arena.rlog;
  a.fam_floats = p.fam_floats;
  a.fan = p.fan;
  if (filt) {
    // outside the scan timing events: not counted in scan_ms
    // (over the csr_rows positions: fewer than ntotal after a removal)
    int64_t waves = (h->csr_rows + 63) / 64;
    h->filt_ws.ensure((size_t)waves * 8);
    hipLaunchKernelGGL(k_filter_id2pos, dim3((unsigned)((waves + 3) / 4)),
                       dim3(256), 0, stream, allow, h->cr_ids.as<int64_t>(),
                       (long long)h->csr_rows, h->filt_ws.as<unsigned>());
    a.posbits = h->filt_ws.as<unsigned>();
  }
  if (use_pre) {
    // per-batch tables: q norms + term3 (counted as LUT-build time)
    TimingEv el;
    if (h->timing) el = h->ev_begin(stream);
    h->qn_ws.ensure((size_t)nq * 4);
    h->term3_ws.ensure((size_t)nq * h->m * 256 * 4);
    rownorms(q, nq, h->d, h->qn_ws.as<float>(), stream);
    hipLaunchKernelGGL(k_pq_term3, grid1d(nq * (int64_t)h->m * 256), dim3(256),
                       0, stream, q, h->codebooks.as<float>(), nq, h->m,
                       h->dsub, h->term3_ws.as<float>());
    if (h->timing) h->ev_end(el, stream, h->ev_lut);
    a.term2 = h->term2.as<float>();
    a.term3 = h->term3_ws.as<float>();
    a.qn = h->qn_ws.as<float>();
  }
  // one launch covers all queries, except on the GLUT path, which walks
  // them in chunks of the LUT buffer: build the chunk's LUTs, scan it
  j.qch = use_glut ? std::min(p.glut_qch, nq) : nq;
  if (use_glut) {
    h->pq_lut_ws.ensure((size_t)j.qch * nprobe * h->m * 256 *
                        (p.lut_f16 ? 2 : 4));
    a.glut = h->pq_lut_ws.as<float>();
  }
  j.a = a;
  return j;
}

// The one scan launch. per_chunk(a, q0) sets the output pointers of the
// launch that starts at query q0. build_lut = false skips the GLUT build
// (the buffer still holds the tables of the only chunk).
template <typename PerChunk>
static void scan_launch(dfann_index *h, const ScanJob &j, int64_t nq,
                        const float *q, int nprobe, const int32_t *probes,
                        const float *keys, hipStream_t stream, bool build_lut,
                        PerChunk per_chunk) {
  const ScanPlan &p = j.p;
  const bool ip = h->metric == M_IP;
  const bool use_glut = p.mode == SCAN_PQ_G || p.mode == SCAN_PQ_GH;
  ScanArgs a = j.a;
  for (int64_t q0 = 0; q0 < nq; q0 += j.qch) {
    int64_t nqc = std::min<int64_t>(j.qch, nq - q0);
    a.q = q + q0 * h->d;
    a.probes = probes + q0 * nprobe;
    a.keys = keys + q0 * nprobe;
    a.nq = (int)nqc;
    per_chunk(a, q0);
    if (use_glut && build_lut) {
      long long qpn = (long long)nqc * nprobe;
      dim3 lg((unsigned)((qpn + PQ_LUT_QPT - 1) / PQ_LUT_QPT),
              (unsigned)h->m);
      int pad = h->dsub | 1;
      size_t lut_lds = (size_t)(256 + PQ_LUT_QPT) * pad * 4;
      TimingEv el;
      if (h->timing) el = h->ev_begin(stream);
      if (p.lut_f16) {
        hipLaunchKernelGGL(k_pq_lut_f16, lg, dim3(256), lut_lds, stream, a.q,
                           a.cent, a.cb, a.probes, h->nlist, a.nq, nprobe,
                           h->d, h->m, h->dsub, ip ? 1 : 0,
                           h->pq_lut_ws.as<__half>());
      } else {
        hipLaunchKernelGGL(k_pq_lut, lg, dim3(256), lut_lds, stream, a.q,
                           a.cent, a.cb, a.probes, h->nlist, a.nq, nprobe,
                           h->d, h->m, h->dsub, ip ? 1 : 0,
                           h->pq_lut_ws.as<float>());
      }
      if (h->timing) h->ev_end(el, stream, h->ev_lut);
    }
    TimingEv e;
    if (h->timing) e = h->ev_begin(stream);
    // (uploads the slab table after a CSR rebuild: inside the scan events)
    a.codes = h->csr_arena.dev_table(stream);
    hipLaunchKernelGGL(j.kern, dim3((unsigned)(nqc * nprobe * p.fan)),
                       dim3(p.scan_bs), p.lds, stream, a);
    if (h->timing) h->ev_end(e, stream, h->ev_scan);
  }
}

// timing: algorithmic units of one scan pass, sum of probed list lengths
static void scan_account(dfann_index *h, int64_t nq, int nprobe,
                         const int32_t *probes) {
  if (!h->timing) return;
  std::vector<int32_t> hp((size_t)nq * nprobe);
  HIP_CHECK(hipMemcpy(hp.data(), probes, hp.size() * 4, hipMemcpyDeviceToHost));
  int64_t rows = 0;
  for (int32_t L : hp)  // a probe outside [0, nlist) is an empty slot
    if ((uint32_t)L < (uint32_t)h->nlist)
      rows += h->h_off[L + 1] - h->h_off[L];
  h->scan_rows += rows;
  h->scan_bytes += rows * h->stride;
}

static void scan_and_merge(dfann_index *h, int64_t nq, const float *q,
                           int nprobe, const int32_t *probes,
                           const float *keys, int k, float *D, int64_t *I,
                           hipStream_t stream,
                           const uint32_t *allow = nullptr) {
  const bool ip = h->metric == M_IP;
  const ScanJob j = scan_prepare(h, nq, q, nprobe, k, stream, allow, false);
  const int fan = j.p.fan;
  h->ws3.ensure((size_t)nq * nprobe * fan * k * 4);
  h->ws4.ensure((size_t)nq * nprobe * fan * k * 4);
  float *cand_d = h->ws3.as<float>();
  unsigned *cand_p = h->ws4.as<unsigned>();
  scan_launch(h, j, nq, q, nprobe, probes, keys, stream, true,
              [&](ScanArgs &a, int64_t q0) {
                a.cand_d = cand_d + q0 * nprobe * fan * k;
                a.cand_p = cand_p + q0 * nprobe * fan * k;
              });
  scan_account(h, nq, nprobe, probes);
  TimingEv em;
  if (h->timing) em = h->ev_begin(stream);
  launch_merge_cand(stream, cand_d, cand_p, nq, nprobe * fan * k, k,
                    h->cr_ids.as<int64_t>(), ip, D, I, MERGE_WAVE);
  if (h->timing) h->ev_end(em, stream, h->ev_merge);
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// range search: count pass, offsets, one sync for the
// total, fill pass — the scans' range twins, same plan and row arithmetic
// as the top-k scans.
// ---------------------------------------------------------------------------

static void range_check(const dfann_index *h, const uint32_t *allow,
                        int64_t nbits) {
  if (h->type == T_FLAT)
    throw std::runtime_error("range search unsupported for flat");
  if (h->type == T_HNSW)
    throw std::runtime_error("range search unsupported for hnswsq");
  if (h->refine)
    throw std::runtime_error("range search unsupported with refine");
  if (!h->trained) throw std::runtime_error("range search on untrained index");
  if (allow && nbits < h->ntotal)
    throw std::runtime_error(
        "range search: allow bitmap covers " + std::to_string(nbits) +
        " ids but the index holds " + std::to_string(h->ntotal));
}

static void range_scan(dfann_index *h, int64_t nq, const float *q, int nprobe,
                       const int32_t *probes, const float *keys, float radius,
                       const uint32_t *allow, int64_t *lims, int64_t *total_out,
                       hipStream_t stream) {
  const ScanJob j = scan_prepare(h, nq, q, nprobe, 1, stream, allow, true);
  const int W = (int)j.p.scan_bs / 64;
  // workspace: offsets and counts for 8 waves per (query, probe) whatever
  // the block size, the per-query totals and the error word
  const size_t nslot = (size_t)nq * nprobe * 8;
  h->range_ws.ensure(nslot * 8 + (size_t)nq * 8 + 8 + nslot * 4);
  long long *off = h->range_ws.as<long long>();
  long long *tot = off + nslot;
  int *err = reinterpret_cast<int *>(tot + nq);
  int *cnt = err + 2;
  HIP_CHECK(hipMemsetAsync(err, 0, 8, stream));
  auto pass = [&](int fill) {
    // a single GLUT chunk's tables survive from the count pass
    scan_launch(h, j, nq, q, nprobe, probes, keys, stream,
                fill == 0 || j.qch < nq, [&](ScanArgs &a, int64_t q0) {
                  a.radius = radius;
                  a.range_fill = fill;
                  a.range_cnt = cnt + q0 * nprobe * W;
                  a.range_off = off + q0 * nprobe * W;
                  a.range_lims = lims + q0;
                  a.cr_ids = h->cr_ids.as<int64_t>();
                  a.range_D = h->range_D.as<float>();
                  a.range_I = h->range_I.as<int64_t>();
                  a.range_err = err;
                });
    scan_account(h, nq, nprobe, probes);
  };
  pass(0);
  hipLaunchKernelGGL(k_range_offsets, dim3((unsigned)nq), dim3(256), 0, stream,
                     cnt, nprobe * W, off, tot);
  hipLaunchKernelGGL(k_range_lims, dim3(1), dim3(256), 0, stream, tot,
                     (long long)nq, reinterpret_cast<long long *>(lims));
  HIP_CHECK(hipGetLastError());
  int64_t total = 0;
  HIP_CHECK(hipMemcpyAsync(&total, lims + nq, 8, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  *total_out = total;
  if (total > h->range_max)
    throw std::runtime_error(
        "range search: " + std::to_string(total) +
        " results exceed range_max_results = " + std::to_string(h->range_max));
  if (total == 0) return;
  h->range_D.ensure((size_t)total * 4);
  h->range_I.ensure((size_t)total * 8);
  pass(1);
  // a fill pass that met another hit count than the count pass stored
  // nothing outside its segment and raised the error word
  int herr = 0;
  HIP_CHECK(hipMemcpyAsync(&herr, err, 4, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  if (herr)
    throw std::runtime_error("range search: count and fill passes disagree");
}

// probes_in == nullptr: coarse-select the index's nprobe lists
static void range_impl(dfann_index *h, int64_t nq, const float *q_dev,
                       int nprobe, const int32_t *probes_in,
                       const float *keys_in, float radius,
                       const uint32_t *allow, int64_t nbits, int64_t *lims,
                       int64_t *total_out, const float **D_out,
                       const int64_t **I_out, hipStream_t stream) {
  range_check(h, allow, nbits);
  *total_out = 0;
  if (nq == 0 || h->nlive() == 0) {
    HIP_CHECK(hipMemsetAsync(lims, 0, (size_t)(nq + 1) * 8, stream));
  } else {
    const float *qi = opq_queries(h, nq, q_dev, stream);
    finalize_csr(h, stream);
    const int32_t *probes = probes_in;
    const float *keys = keys_in;
    if (!probes) {
      nprobe = std::min(std::min(h->nprobe, h->nlist), 512);
      DevBuf &pb = h->ws2;
      pb.ensure((size_t)nq * nprobe * 8);
      int32_t *pr = pb.as<int32_t>();
      float *ke = reinterpret_cast<float *>(pb.as<uint8_t>() +
                                            (size_t)nq * nprobe * 4);
      coarse_impl(h, nq, qi, nprobe, pr, ke, stream);
      probes = pr;
      keys = ke;
    } else if (nprobe < 1 || nprobe > 512) {
      throw std::runtime_error("range search: nprobe must be in 1..512");
    }
    range_scan(h, nq, qi, nprobe, probes, keys, radius, allow, lims, total_out,
               stream);
  }
  *D_out = h->range_D.as<float>();
  *I_out = h->range_I.as<int64_t>();
}

// allow != nullptr: filtered (id-space bitmap; flat ids are positions)
static void flat_search_impl(dfann_index *h, int64_t nq, const float *q, int k,
                             float *D, int64_t *I, hipStream_t stream,
                             const uint32_t *allow = nullptr) {
  if (h->nlive() == 0) { pad_fill(h, nq, k, D, I, stream); return; }
  // tombstones: once anything was removed every search is a
  // filtered one, under the live bitmap or under its AND with the caller's
  if (h->nremoved) {
    const unsigned *live = h->flat_live.as<unsigned>();
    if (allow) {
      int64_t words = (h->ntotal + 31) / 32;
      h->filt_ws.ensure((size_t)words * 4);
      hipLaunchKernelGGL(k_bits_and, grid1d(words), dim3(256), 0, stream,
                         allow, live, (long long)h->ntotal,
                         h->filt_ws.as<unsigned>());
      allow = h->filt_ws.as<unsigned>();
    } else {
      allow = live;
    }
  }
  bool ip = h->metric == M_IP;
  const int64_t CH = std::min<int64_t>(65536, std::max<int64_t>(
      4096, ((int64_t)h->ws_mb << 20) / (64 * 4)));
  int64_t nch = (h->ntotal + CH - 1) / CH;
  // chunk queries so scores fit
  int64_t qch = std::max<int64_t>(1, ((int64_t)h->ws_mb << 20) / (CH * 4));
  qch = std::min(qch, nq);
  h->ws1.ensure((size_t)qch * CH * 4);
  h->ws2.ensure((size_t)std::max<int64_t>(CH, nq) * 4);            // bnorm / qnorm
  h->ws3.ensure((size_t)nq * nch * k * 4);                         // chunk winners d
  h->ws4.ensure((size_t)nq * nch * k * 4);                         // chunk winners p
  h->ws5.ensure((size_t)nq * 4);                                   // qnorm
  float *sc = h->ws1.as<float>();
  float *bn = h->ws2.as<float>();
  float *qn = h->ws5.as<float>();
  float *wd = h->ws3.as<float>();
  unsigned *wp = h->ws4.as<unsigned>();
  if (!ip) rownorms(q, nq, h->d, qn, stream);
  for (int64_t ci = 0; ci < nch; ++ci) {
    int64_t b0 = ci * CH;
    int64_t bn_rows = std::min(CH, h->ntotal - b0);
    const float *base = h->flat.as<float>() + (size_t)b0 * h->d;
    if (!ip) rownorms(base, bn_rows, h->d, bn, stream);
    for (int64_t s = 0; s < nq; s += qch) {
      int64_t c = std::min(qch, nq - s);
      gemm_keys(h, q + s * h->d, c, base, bn_rows, h->d, bn, qn + s,
                ip ? 0 : 2, sc, stream);
      // winners layout: (nq, nch, k) — row stride nch*k
      launch_topk_rows(stream, 256, sc, c, bn_rows, k, (unsigned)b0, nch * k,
                       wd + (s * nch + ci) * k, wp + (s * nch + ci) * k,
                       allow);
    }
  }
  // merge chunk winners (flat ids are positions: no id table; block-per-
  // query kernels only: MERGE_RK excludes just the wave path, k > 16 still
  // goes to the LDS kernel)
  launch_merge_cand(stream, wd, wp, nq, (int)(nch * k), k, nullptr, ip, D, I,
                    MERGE_RK);
  HIP_CHECK(hipGetLastError());
}

// shared argument checks of the two filtered entries
static void check_filter(dfann_index *h, const uint32_t *allow,
                         int64_t nbits) {
  if (h->type == T_HNSW)
    throw std::runtime_error("filtered search unsupported for hnswsq");
  if (!allow) throw std::runtime_error("filtered search: null allow bitmap");
  if (nbits < h->ntotal)
    throw std::runtime_error(
        "filtered search: allow bitmap covers " + std::to_string(nbits) +
        " ids but the index holds " + std::to_string(h->ntotal));
}

// shared host checks of the two preassigned top-k entries (the range entry
// bounds its nprobe in range_impl). The probe VALUES are not checked: that
// would need a host sync, and the scans treat a probe outside [0, nlist)
// as an empty slot.
static void check_preassigned(int k, int nprobe) {
  if (k > 512)
    throw std::runtime_error("search_preassigned: k > 512 unsupported (k = " +
                             std::to_string(k) + ")");
  if (k < 1)
    throw std::runtime_error("search_preassigned: k < 1 (k = " +
                             std::to_string(k) + ")");
  if (nprobe < 1 || nprobe > 512)
    throw std::runtime_error(
        "search_preassigned: nprobe must be in 1..512 (nprobe = " +
        std::to_string(nprobe) + ")");
}

static void search_impl(dfann_index *h, int64_t nq, const float *q, int k,
                        float *D, int64_t *I, hipStream_t stream,
                        const uint32_t *allow = nullptr) {
  if (!h->trained) throw std::runtime_error("search on untrained index");
  if (k > 512) throw std::runtime_error("k > 512 unsupported");
  if (nq == 0) return;
  if (h->type == T_FLAT) {
    flat_search_impl(h, nq, q, k, D, I, stream, allow);
    return;
  }
  if (h->nlive() == 0) { pad_fill(h, nq, k, D, I, stream); return; }
  if (h->type == T_HNSW) { hnsw_search(h, nq, q, k, D, I, stream); return; }
  finalize_csr(h, stream);
  int nprobe = std::min(h->nprobe, h->nlist);
  if (nprobe > 512) {
    // documented clamp (include/dfann.h Limits): warn once per process
    static bool warned = false;
    if (!warned) {
      warned = true;
      fprintf(stderr,
              "[dfann] warning: nprobe=%d exceeds the engine cap; clamped to "
              "512 (the faiss-backed reference would probe more lists)\n",
              nprobe);
    }
    nprobe = 512;
  }
  // probes + keys
  DevBuf &pb = h->ws2;
  pb.ensure((size_t)nq * nprobe * 8);
  int32_t *probes = pb.as<int32_t>();
  float *keys = reinterpret_cast<float *>(pb.as<uint8_t>() + (size_t)nq * nprobe * 4);
  coarse_impl(h, nq, q, nprobe, probes, keys, stream);
  scan_and_merge(h, nq, q, nprobe, probes, keys, k, D, I, stream, allow);
}

// ---------------------------------------------------------------------------
// refine stage
// ---------------------------------------------------------------------------

// k' = min(512, max(k, ceil(k * k_factor))). A product within 1e-4 above
// an integer counts as that integer, so a k_factor that went through
// float32 (1.6f = 1.60000002) still gives k' = 16 at k = 10.
static int refine_kprime(const dfann_index *h, int k) {
  int kp = (int)std::ceil((double)k * h->k_factor - 1e-4);
  kp = std::max(kp, k);
  return std::min(kp, REFINE_KMAX);
}

// Runs `base(k', D', I')` (any of the search entries) into the workspace
// and re-ranks its candidates exactly into the caller's (nq, k) D / I.
// Stream-ordered, no host sync; the workspace grows only when a shape is
// first seen, so a warmed-up call captures into a HIP graph.
template <typename Base>
static void search_with_refine(dfann_index *h, int64_t nq, const float *q,
                               int k, float *D, int64_t *I, hipStream_t stream,
                               Base base) {
  if (!h->refine) { base(k, D, I); return; }
  if (k > 512) throw std::runtime_error("k > 512 unsupported");
  if (k < 1) throw std::runtime_error("k < 1");
  if (nq == 0) return;
  const int kp = refine_kprime(h, k);
  h->rf_D.ensure((size_t)nq * kp * 4);
  h->rf_I.ensure((size_t)nq * kp * 8);
  base(kp, h->rf_D.as<float>(), h->rf_I.as<int64_t>());
  SlabArena &ra = h->refine_arena;
  const uint8_t *const *tab = ra.dev_table(stream);
  const size_t lds = REFINE_LDS_BYTES(h->d_in);
  const bool ip = h->metric == M_IP;
  auto kern = h->refine == 2 ? (ip ? k_refine<__half, 0> : k_refine<__half, 1>)
                             : (ip ? k_refine<float, 0> : k_refine<float, 1>);
  hipLaunchKernelGGL(kern, dim3((unsigned)nq), dim3(256), lds, stream, q, tab,
                     ra.rlog, ra.stride, (long long)ra.rows,
                     h->rf_I.as<int64_t>(), (long long)nq, kp, k, h->d_in, D, I);
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// removal
// ---------------------------------------------------------------------------

// threads per row of k_remove_compact: stride / 16 (one 16-byte unit each)
// or 1 (a thread per row). DFANN_REMOVE_LANES=1 (A/B knob, read per call)
// takes the thread-per-row shape; BASELINE.md "Removal" has the comparison.
static int remove_lanes(const dfann_index *h) {
  if (const char *e = getenv("DFANN_REMOVE_LANES"))
    if (atoi(e) == 1) return 1;
  return h->stride / 16;
}

// flat: tombstones. The bitmap is small (ntotal / 8 bytes) and the call
// synchronizes anyway, so the host mirror is updated and uploaded.
static int64_t remove_flat(dfann_index *h, const uint32_t *remove,
                           hipStream_t stream) {
  const size_t words = (size_t)((h->ntotal + 31) / 32);
  std::vector<uint32_t> rm(words);
  HIP_CHECK(hipMemcpyAsync(rm.data(), remove, words * 4, hipMemcpyDeviceToHost,
                           stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  if (h->ntotal & 31) rm[words - 1] &= (1u << (unsigned)(h->ntotal & 31)) - 1u;
  const bool have = h->nremoved > 0;
  int64_t n = 0;
  for (size_t w = 0; w < words; ++w) {
    if (have) rm[w] &= h->h_flat_live[w];
    n += __builtin_popcount(rm[w]);
  }
  if (n == 0) return 0;
  if (!have) {  // first removal: everything issued so far is live
    h->h_flat_live.assign(words, 0u);
    flat_live_extend(h, 0);
  }
  for (size_t w = 0; w < words; ++w) h->h_flat_live[w] &= ~rm[w];
  HIP_CHECK(hipMemcpy(h->flat_live.p, h->h_flat_live.data(), words * 4,
                      hipMemcpyHostToDevice));
  h->nremoved += n;
  return n;
}

// ivf: physical removal. Old positions are walked in ascending windows of
// one slab, one launch each. A kept row's new position is never past its old
// one, so window w writes new slabs <= w only — and new slab 0 is the one
// fresh allocation while new slab i >= 1 IS old slab i - 1, which windows
// < w have read completely. The launches are ordered by the stream: no host
// sync and no allocator call between windows, peak memory ~codes + one slab
// (the bound of rebuild_csr). Old slabs past the survivors are freed at the
// end.
static int64_t remove_ivf(dfann_index *h, const uint32_t *remove,
                          hipStream_t stream) {
  finalize_csr(h, stream);  // pending rows are removable too
  const int64_t n = h->csr_rows;
  if (n == 0) return 0;
  const int64_t words = (n + 63) / 64;
  h->rm_keep.ensure((size_t)words * 8);
  h->rm_cnt.ensure((size_t)words * 4);
  h->rm_prefix.ensure((size_t)(words + 1) * 8);
  auto *keepw = h->rm_keep.as<unsigned long long>();
  auto *prefix = h->rm_prefix.as<long long>();
  hipLaunchKernelGGL(k_remove_keep, dim3((unsigned)((words + 3) / 4)),
                     dim3(256), 0, stream, remove, h->cr_ids.as<int64_t>(),
                     (long long)n, keepw, h->rm_cnt.as<int>());
  hipLaunchKernelGGL(k_remove_scan, dim3(1), dim3(256), 0, stream,
                     h->rm_cnt.as<int>(), (long long)words, prefix);
  HIP_CHECK(hipGetLastError());
  int64_t kept = 0;
  HIP_CHECK(hipMemcpyAsync(&kept, prefix + words, 8, hipMemcpyDeviceToHost,
                           stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  if (kept == n) return 0;  // nothing stored was named: not a byte changes
  h->cr_ids_new.ensure((size_t)std::max<int64_t>(kept, 1) * 8);
  SlabArena next;
  next.init(h->stride, h->csr_arena.slab_bytes());
  if (next.rlog != h->csr_arena.rlog)
    throw std::runtime_error("remove_ids: slab geometry mismatch");
  const int64_t rps = next.rps();
  const int lanes = remove_lanes(h);
  SlabArena &old = h->csr_arena;
  // kept < n, so the survivors need no more slabs than the old image has
  const size_t n_new_slabs = (size_t)((kept + rps - 1) >> next.rlog);
  if (n_new_slabs > old.slabs.size())
    throw std::runtime_error("remove_ids: slab count mismatch");
  if (n_new_slabs) next.ensure_rows(1);  // the fresh slab
  for (size_t i = 1; i < n_new_slabs; ++i) next.slabs.push_back(old.slabs[i - 1]);
  next.table_dirty = true;
  const uint8_t *const *old_tab = old.dev_table(stream);
  uint8_t *const *new_tab = next.dev_table_mut(stream);
  for (int64_t p0 = 0; p0 < n; p0 += rps) {
    const int64_t p1 = std::min(n, p0 + rps);
    hipLaunchKernelGGL(k_remove_compact, grid1d((p1 - p0) * lanes, 256, 1LL << 30),
                       dim3(256), 0, stream, (long long)p0, (long long)p1,
                       lanes, keepw, prefix, (long long)words, old_tab, new_tab,
                       h->cr_ids.as<int64_t>(), h->cr_ids_new.as<int64_t>(),
                       h->id2pos.as<unsigned>(), next.rlog, h->stride);
    HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_remove_off, grid1d(h->nlist + 1), dim3(256), 0, stream,
                     keepw, prefix, (long long)words, h->cr_off.as<int64_t>(),
                     h->nlist);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(h->h_off.data(), h->cr_off.p,
                           (size_t)(h->nlist + 1) * 8, hipMemcpyDeviceToHost,
                           stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  // old slabs [0, n_new_slabs - 1) live on in `next`; reset frees the rest
  for (size_t i = 1; i < n_new_slabs; ++i) old.slabs[i - 1] = nullptr;
  old.reset();
  std::swap(old.stride, next.stride);
  std::swap(old.rlog, next.rlog);
  std::swap(old.slabs, next.slabs);
  old.rows = kept;
  old.table_dirty = true;
  next.rows = 0;
  h->csr_rows = kept;
  std::swap(h->cr_ids.p, h->cr_ids_new.p);
  std::swap(h->cr_ids.cap, h->cr_ids_new.cap);
  h->nremoved += n - kept;
  return n - kept;
}

// ---------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------

#define API_BEGIN try {
#define API_END                                                                \
  return 0;                                                                    \
  }                                                                            \
  catch (const std::exception &e) { g_err = e.what(); return 1; }

extern "C" int dfann_create(const char *spec_json, dfann_index **out) {
  API_BEGIN
  *out = create_from_spec(spec_json);
  API_END
}

extern "C" int dfann_destroy(dfann_index *h) {
  API_BEGIN
  delete h;
  API_END
}

extern "C" int dfann_train(dfann_index *h, int64_t n, const float *x_dev,
                           dfann_stream stream) {
  API_BEGIN
  hipStream_t s = (hipStream_t)stream;
  // one pass over the raw rows before anything is learned from them: a
  // non-finite value is refused and the index stays untrained (flat trains
  // nothing, a trained index ignores the call)
  if (!h->trained && h->type != T_FLAT)
    if (const char *cls = nonfinite_class(h, x_dev, n * h->d_in, s))
      throw std::runtime_error(
          std::string("train: the training set holds a non-finite value (") +
          cls + ")");
  if (h->opq && !h->trained) {
    // faiss IndexPreTransform::train: learn the transform on the raw rows
    // (kept as is when one was injected), then train the inner index on
    // the transformed set
    if (!h->opq_set) opq_learn(h, n, x_dev, s);
    DevBuf y;
    y.ensure((size_t)std::max<int64_t>(n, 1) * h->d * 4);
    run_transform(nullptr, h->opq_A.as<float>(), n, x_dev, h->d_in, h->d,
                  y.as<float>(), s);
    train_impl(h, n, y.as<float>(), s);
    return 0;
  }
  train_impl(h, n, x_dev, s);
  API_END
}

extern "C" int dfann_add(dfann_index *h, int64_t n, const float *x_dev,
                         dfann_stream stream) {
  API_BEGIN
  add_impl(h, n, x_dev, (hipStream_t)stream);
  API_END
}

extern "C" int dfann_search(dfann_index *h, int64_t nq, const float *q_dev,
                            int k, float *D_dev, int64_t *I_dev,
                            dfann_stream stream) {
  API_BEGIN
  hipStream_t s = (hipStream_t)stream;
  // OPQ: transformed once; the refine stage re-ranks against the original
  const float *qi = opq_queries(h, nq, q_dev, s);
  search_with_refine(h, nq, q_dev, k, D_dev, I_dev, s,
                     [&](int kb, float *Db, int64_t *Ib) {
                       search_impl(h, nq, qi, kb, Db, Ib, s);
                     });
  API_END
}

extern "C" int dfann_coarse(dfann_index *h, int64_t nq, const float *q_dev,
                            int nprobe, int32_t *probes_dev, float *keys_dev,
                            dfann_stream stream) {
  API_BEGIN
  if (!h->trained || h->type == T_FLAT)
    throw std::runtime_error("coarse needs a trained IVF index");
  nprobe = std::min(nprobe, h->nlist);
  const float *qi = opq_queries(h, nq, q_dev, (hipStream_t)stream);
  coarse_impl(h, nq, qi, nprobe, probes_dev, keys_dev, (hipStream_t)stream);
  API_END
}

extern "C" int dfann_search_preassigned(dfann_index *h, int64_t nq,
                                        const float *q_dev, int nprobe,
                                        const int32_t *probes_dev,
                                        const float *keys_dev, int k,
                                        float *D_dev, int64_t *I_dev,
                                        dfann_stream stream) {
  API_BEGIN
  if (!h->trained || h->type == T_FLAT)
    throw std::runtime_error("search_preassigned needs a trained IVF index");
  check_preassigned(k, nprobe);
  if (nq == 0) return 0;
  if (!probes_dev || !keys_dev)
    throw std::runtime_error("search_preassigned: null probes / keys");
  hipStream_t s = (hipStream_t)stream;
  const float *qi = opq_queries(h, nq, q_dev, s);
  search_with_refine(h, nq, q_dev, k, D_dev, I_dev, s,
                     [&](int kb, float *Db, int64_t *Ib) {
                       if (h->nlive() == 0) {
                         pad_fill(h, nq, kb, Db, Ib, s);
                         return;
                       }
                       finalize_csr(h, s);
                       scan_and_merge(h, nq, qi, nprobe, probes_dev,
                                      keys_dev, kb, Db, Ib, s);
                     });
  API_END
}

extern "C" int dfann_search_filtered(dfann_index *h, int64_t nq,
                                     const float *q_dev, int k,
                                     const uint32_t *allow_bits_dev,
                                     int64_t nbits, float *D_dev,
                                     int64_t *I_dev, dfann_stream stream) {
  API_BEGIN
  check_filter(h, allow_bits_dev, nbits);
  hipStream_t s = (hipStream_t)stream;
  const float *qi = opq_queries(h, nq, q_dev, s);
  // the filter applies in the base stage only: refine sees allowed ids
  search_with_refine(h, nq, q_dev, k, D_dev, I_dev, s,
                     [&](int kb, float *Db, int64_t *Ib) {
                       search_impl(h, nq, qi, kb, Db, Ib, s,
                                   allow_bits_dev);
                     });
  API_END
}

extern "C" int dfann_search_preassigned_filtered(
    dfann_index *h, int64_t nq, const float *q_dev, int nprobe,
    const int32_t *probes_dev, const float *keys_dev, int k,
    const uint32_t *allow_bits_dev, int64_t nbits, float *D_dev,
    int64_t *I_dev, dfann_stream stream) {
  API_BEGIN
  if (!h->trained || h->type == T_FLAT)
    throw std::runtime_error("search_preassigned needs a trained IVF index");
  check_filter(h, allow_bits_dev, nbits);
  check_preassigned(k, nprobe);
  if (nq == 0) return 0;
  if (!probes_dev || !keys_dev)
    throw std::runtime_error("search_preassigned: null probes / keys");
  hipStream_t s = (hipStream_t)stream;
  const float *qi = opq_queries(h, nq, q_dev, s);
  search_with_refine(h, nq, q_dev, k, D_dev, I_dev, s,
                     [&](int kb, float *Db, int64_t *Ib) {
                       if (h->nlive() == 0) {
                         pad_fill(h, nq, kb, Db, Ib, s);
                         return;
                       }
                       finalize_csr(h, s);
                       scan_and_merge(h, nq, qi, nprobe, probes_dev,
                                      keys_dev, kb, Db, Ib, s, allow_bits_dev);
                     });
  API_END
}

extern "C" int dfann_remove_ids(dfann_index *h, const uint32_t *remove_bits_dev,
                                int64_t nbits, int64_t *nremoved_out,
                                dfann_stream stream) {
  API_BEGIN
  if (nremoved_out) *nremoved_out = 0;
  if (h->type == T_HNSW)
    throw std::runtime_error("remove_ids unsupported for hnswsq");
  if (!remove_bits_dev) throw std::runtime_error("remove_ids: null bitmap");
  if (nbits < h->ntotal)
    throw std::runtime_error(
        "remove_ids: bitmap covers " + std::to_string(nbits) +
        " ids but the index holds " + std::to_string(h->ntotal));
  // an untrained ivf index and an index without rows have nothing to remove
  if (!h->trained || h->nlive() == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  int64_t n = h->type == T_FLAT ? remove_flat(h, remove_bits_dev, s)
                                : remove_ivf(h, remove_bits_dev, s);
  if (nremoved_out) *nremoved_out = n;
  API_END
}

extern "C" int dfann_range_search(dfann_index *h, int64_t nq,
                                  const float *q_dev, float radius,
                                  const uint32_t *allow_dev, int64_t nbits,
                                  int64_t *lims_dev, int64_t *total_out,
                                  const float **D_dev_out,
                                  const int64_t **I_dev_out,
                                  dfann_stream stream) {
  API_BEGIN
  range_impl(h, nq, q_dev, 0, nullptr, nullptr, radius, allow_dev, nbits,
             lims_dev, total_out, D_dev_out, I_dev_out, (hipStream_t)stream);
  API_END
}

extern "C" int dfann_range_search_preassigned(
    dfann_index *h, int64_t nq, const float *q_dev, int nprobe,
    const int32_t *probes_dev, const float *keys_dev, float radius,
    const uint32_t *allow_dev, int64_t nbits, int64_t *lims_dev,
    int64_t *total_out, const float **D_dev_out, const int64_t **I_dev_out,
    dfann_stream stream) {
  API_BEGIN
  if (!probes_dev || !keys_dev)
    throw std::runtime_error("range search: null probes / keys");
  range_impl(h, nq, q_dev, nprobe, probes_dev, keys_dev, radius, allow_dev,
             nbits, lims_dev, total_out, D_dev_out, I_dev_out,
             (hipStream_t)stream);
  API_END
}

extern "C" int dfann_search_reconstruct(dfann_index *h, int64_t nq,
                                        const float *q_dev, int k,
                                        float *D_dev, int64_t *I_dev,
                                        float *R_dev, dfann_stream stream) {
  API_BEGIN
  if (h->refine) {
    // a refine index returns the STORED rows, not the code decode
    hipStream_t s = (hipStream_t)stream;
    const float *qi = opq_queries(h, nq, q_dev, s);
    search_with_refine(h, nq, q_dev, k, D_dev, I_dev, s,
                       [&](int kb, float *Db, int64_t *Ib) {
                         search_impl(h, nq, qi, kb, Db, Ib, s);
                       });
    if (nq == 0) return 0;
    SlabArena &ra = h->refine_arena;
    auto rk = h->refine == 2 ? k_refine_reconstruct<__half>
                             : k_refine_reconstruct<float>;
    hipLaunchKernelGGL(rk, dim3((unsigned)(nq * k)), dim3(64), 0, s, I_dev,
                       (long long)(nq * k), h->d_in, ra.dev_table(s), ra.rlog,
                       ra.stride, (long long)ra.rows, R_dev);
    HIP_CHECK(hipGetLastError());
    return 0;
  }
  const float *qi = opq_queries(h, nq, q_dev, (hipStream_t)stream);
  search_impl(h, nq, qi, k, D_dev, I_dev, (hipStream_t)stream);
  if (nq == 0) return 0;
  // OPQ: decode at d_out, then rotate back with A^T (faiss
  // VectorTransform::reverse_transform of an orthonormal matrix)
  float *R_dec = R_dev;
  if (h->opq) {
    h->opq_r.ensure((size_t)nq * k * h->d * 4);
    R_dec = h->opq_r.as<float>();
  }
  int rtype;
  const float *flat_src = nullptr;
  if (h->type == T_FLAT) { rtype = 0; flat_src = h->flat.as<float>(); }
  else if (h->type == T_IVFFLAT) rtype = 0;
  else if (h->type == T_IVFPQ) rtype = h->nbits == 4 ? 6 : 2;
  else if (h->type == T_HNSW) rtype = 5;
  else
    rtype = h->sq_bits == 8 ? 3 : h->sq_bits == 6 ? 8 : h->sq_bits == 4 ? 7 : 4;
  hipLaunchKernelGGL(k_reconstruct, dim3((unsigned)(nq * k)), dim3(64), 0,
                     (hipStream_t)stream, I_dev, nq, k, rtype, h->d, h->m,
                     h->dsub, h->stride, h->csr_arena.rlog, flat_src,
                     h->csr_arena.dev_table((hipStream_t)stream),
                     h->id2pos.as<unsigned>(), h->cr_off.as<int64_t>(),
                     h->nlist, h->centroids.as<float>(),
                     h->codebooks.as<float>(), h->sq_vmin.as<float>(),
                     h->sq_scale.as<float>(), R_dec);
  HIP_CHECK(hipGetLastError());
  if (h->opq)
    run_transform(nullptr, h->opq_At.as<float>(), nq * k, R_dec, h->d,
                  h->d_in, R_dev, (hipStream_t)stream);
  API_END
}

extern "C" int dfann_set_nprobe(dfann_index *h, int nprobe) {
  API_BEGIN
  h->nprobe = nprobe;
  API_END
}

extern "C" int dfann_set_k_factor(dfann_index *h, float k_factor) {
  API_BEGIN
  if (!h->refine)
    throw std::runtime_error("set_k_factor: index has no refine stage");
  if (!(k_factor >= 1.0f)) throw std::runtime_error("k_factor must be >= 1");
  h->k_factor = (double)k_factor;
  API_END
}

extern "C" int dfann_refine_info(dfann_index *h, int64_t out[3]) {
  API_BEGIN
  out[0] = h->refine;
  out[1] = h->refine ? h->refine_arena.stride : 0;
  out[2] = h->refine ? h->refine_arena.rows : 0;
  API_END
}

extern "C" int dfann_get_refine_rows(dfann_index *h, int64_t row0, int64_t n,
                                     void *out_host) {
  API_BEGIN
  if (!h->refine) throw std::runtime_error("index has no refine store");
  if (row0 < 0 || n < 0 || row0 + n > h->refine_arena.rows)
    throw std::runtime_error("get_refine_rows: range outside the store");
  HIP_CHECK(hipDeviceSynchronize());
  if (n) h->refine_arena.copy_rows_to_host(out_host, row0, n);
  API_END
}

extern "C" int64_t dfann_ntotal(dfann_index *h) { return h->ntotal; }
extern "C" int64_t dfann_nlive(dfann_index *h) { return h->nlive(); }
extern "C" int dfann_nlist(dfann_index *h) { return h->nlist; }
extern "C" int dfann_is_trained(dfann_index *h) { return h->trained ? 1 : 0; }
extern "C" int dfann_dim(dfann_index *h) { return h->d_in; }
extern "C" const char *dfann_spec_json(dfann_index *h) {
  return h->spec_json.c_str();
}

extern "C" int dfann_get_centroids(dfann_index *h, float *out_host) {
  API_BEGIN
  if (h->type == T_FLAT)
    throw std::runtime_error("'flat' index has no quantizer");
  if (h->type == T_HNSW)
    throw std::runtime_error(
        "hnswsq index has no quantizer (reference AttributeError)");
  if (!h->trained) throw std::runtime_error("index not trained");
  HIP_CHECK(hipMemcpy(out_host, h->centroids.p, (size_t)h->nlist * h->d * 4,
                      hipMemcpyDeviceToHost));
  API_END
}

extern "C" int dfann_get_codebooks(dfann_index *h, float *out_host) {
  API_BEGIN
  if (h->type != T_IVFPQ) throw std::runtime_error("not an ivfpq index");
  HIP_CHECK(hipMemcpy(out_host, h->codebooks.p,
                      (size_t)h->m * pq_ksub(h) * h->dsub * 4,
                      hipMemcpyDeviceToHost));
  API_END
}

extern "C" int dfann_get_lists(dfann_index *h, int64_t *off_host,
                               int64_t *ids_host, uint8_t *codes_host) {
  API_BEGIN
  if (h->type == T_FLAT) throw std::runtime_error("flat index has no lists");
  if (h->type == T_HNSW)
    throw std::runtime_error("hnswsq index has no inverted lists");
  finalize_csr(h, 0);
  memcpy(off_host, h->h_off.data(), (size_t)(h->nlist + 1) * 8);
  if (h->csr_rows) {  // == nlive once finalized
    HIP_CHECK(hipMemcpy(ids_host, h->cr_ids.p, (size_t)h->csr_rows * 8,
                        hipMemcpyDeviceToHost));
    h->csr_arena.copy_rows_to_host(codes_host, 0, h->csr_rows);
  }
  API_END
}

extern "C" int dfann_code_stride(dfann_index *h) { return h->stride; }

extern "C" int dfann_get_sq_params(dfann_index *h, float *vmin_host,
                                   float *vdiff_host) {
  API_BEGIN
  if (!((h->type == T_IVFSQ || h->type == T_HNSW) && h->sq_int()))
    throw std::runtime_error("not an 8 / 6 / 4-bit ivfsq index");
  HIP_CHECK(hipMemcpy(vmin_host, h->sq_vmin.p, (size_t)h->d * 4,
                      hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(vdiff_host, h->sq_vdiff.p, (size_t)h->d * 4,
                      hipMemcpyDeviceToHost));
  API_END
}

extern "C" int dfann_set_trained(dfann_index *h, const float *centroids_host,
                                 const float *codebooks_host,
                                 const float *vmin_host,
                                 const float *vdiff_host) {
  API_BEGIN
  if (h->type == T_FLAT) { h->trained = true; return 0; }
  if (h->opq && !h->opq_set)
    throw std::runtime_error(
        "set_trained on an opq index needs the transform first "
        "(dfann_set_transform)");
  if (!centroids_host) throw std::runtime_error("centroids required");
  h->centroids.ensure((size_t)h->nlist * h->d * 4);
  h->cnorm.ensure((size_t)h->nlist * 4);
  HIP_CHECK(hipMemcpy(h->centroids.p, centroids_host,
                      (size_t)h->nlist * h->d * 4, hipMemcpyHostToDevice));
  rownorms(h->centroids.as<float>(), h->nlist, h->d, h->cnorm.as<float>(), 0);
  if (h->type == T_IVFPQ) {
    if (!codebooks_host) throw std::runtime_error("codebooks required");
    h->codebooks.ensure((size_t)h->m * pq_ksub(h) * h->dsub * 4);
    HIP_CHECK(hipMemcpy(h->codebooks.p, codebooks_host,
                        (size_t)h->m * pq_ksub(h) * h->dsub * 4,
                        hipMemcpyHostToDevice));
  }
  if (h->type == T_IVFSQ && h->sq_int()) {
    if (!vmin_host || !vdiff_host) throw std::runtime_error("sq params required");
    h->sq_vmin.ensure((size_t)h->d * 4);
    h->sq_vdiff.ensure((size_t)h->d * 4);
    h->sq_scale.ensure((size_t)h->d * 4);
    HIP_CHECK(hipMemcpy(h->sq_vmin.p, vmin_host, (size_t)h->d * 4,
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(h->sq_vdiff.p, vdiff_host, (size_t)h->d * 4,
                        hipMemcpyHostToDevice));
    std::vector<float> sc(h->d);
    std::vector<float> vd(h->d);
    memcpy(vd.data(), vdiff_host, (size_t)h->d * 4);
    for (int t = 0; t < h->d; ++t) sc[t] = vd[t] / h->sq_q();
    HIP_CHECK(hipMemcpy(h->sq_scale.p, sc.data(), (size_t)h->d * 4,
                        hipMemcpyHostToDevice));
  }
  refresh_cent_bf16(h, 0);
  HIP_CHECK(hipDeviceSynchronize());
  h->trained = true;
  API_END
}

// ---------------------------------------------------------------------------
// OPQ transform exchange
// ---------------------------------------------------------------------------

extern "C" int dfann_transform_info(dfann_index *h, int64_t out[3]) {
  API_BEGIN
  out[0] = h->opq ? 1 : 0;
  out[1] = h->d_in;
  out[2] = h->d;
  API_END
}

extern "C" int dfann_get_transform(dfann_index *h, float *A_host) {
  API_BEGIN
  opq_require(h);
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpy(A_host, h->opq_A.p, (size_t)h->d * h->d_in * 4,
                      hipMemcpyDeviceToHost));
  API_END
}

extern "C" int dfann_set_transform(dfann_index *h, const float *A_host) {
  API_BEGIN
  if (!h->opq) throw std::runtime_error("index has no opq transform");
  if (!A_host) throw std::runtime_error("set_transform: null matrix");
  if (h->ntotal > 0)
    throw std::runtime_error(
        "set_transform: the index already holds vectors encoded behind the "
        "current transform");
  HIP_CHECK(hipDeviceSynchronize());
  h->opq_A.ensure((size_t)h->d * h->d_in * 4);
  HIP_CHECK(hipMemcpy(h->opq_A.p, A_host, (size_t)h->d * h->d_in * 4,
                      hipMemcpyHostToDevice));
  opq_install(h, 0);
  API_END
}

extern "C" int dfann_apply_transform(dfann_index *h, int64_t n,
                                     const float *x_dev, float *y_dev,
                                     dfann_stream stream) {
  API_BEGIN
  opq_require(h);
  run_transform(h, h->opq_A.as<float>(), n, x_dev, h->d_in, h->d, y_dev,
                (hipStream_t)stream);
  API_END
}

// ---------------------------------------------------------------------------
// shard merge
// ---------------------------------------------------------------------------

extern "C" int dfann_merge_topk(int64_t nq, int S, int k, const float *D_dev,
                                const int64_t *I_dev, int maximize,
                                float *Dout_dev, int64_t *Iout_dev,
                                dfann_stream stream) {
  API_BEGIN
  (void)I_dev;  // slots map to metadata host-side (ref client.py:297-298)
  if (k > 512) throw std::runtime_error("k > 512 unsupported");
  const MergeLaunch m = merge_launch(nq, k, (int64_t)S * k);
  auto kern = m.path == MERGE_WAVE ? k_merge_shards_w
              : m.path == MERGE_RK ? k_merge_shards_rk
                                   : k_merge_shards;
  hipLaunchKernelGGL(kern, m.grid, dim3(256), m.lds, (hipStream_t)stream,
                     D_dev, nq, S, k, maximize, Dout_dev, Iout_dev);
  HIP_CHECK(hipGetLastError());
  API_END
}

// ---------------------------------------------------------------------------
// persistence (our own format, version 1)
// ---------------------------------------------------------------------------

static void fwrite_chk(const void *p, size_t n, FILE *f) {
  if (fwrite(p, 1, n, f) != n) throw std::runtime_error("short write");
}
static void fread_chk(void *p, size_t n, FILE *f) {
  if (fread(p, 1, n, f) != n) throw std::runtime_error("short read");
}

static void dump_dev(FILE *f, DevBuf &b, size_t bytes) {
  std::vector<char> tmp(bytes);
  if (bytes) HIP_CHECK(hipMemcpy(tmp.data(), b.p, bytes, hipMemcpyDeviceToHost));
  fwrite_chk(tmp.data(), bytes, f);
}
static void load_dev(FILE *f, DevBuf &b, size_t bytes) {
  std::vector<char> tmp(bytes);
  fread_chk(tmp.data(), bytes, f);
  b.ensure(std::max(bytes, (size_t)16));
  if (bytes) HIP_CHECK(hipMemcpy(b.p, tmp.data(), bytes, hipMemcpyHostToDevice));
}

extern "C" int dfann_save(dfann_index *h, const char *path) {
  API_BEGIN
  finalize_csr(h, 0);
  FILE *f = fopen(path, "wb");
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  try {
    // "DFANN01" as ever until something was removed; "DFANN02" after
    // (DESIGN.md §6j): nlive follows ntotal, the CSR sections hold nlive
    // rows, flat appends its live bitmap, the refine store keeps ntotal rows
    const bool v2 = h->nremoved > 0;
    const uint64_t magic = v2 ? 0x32304E4E414644ULL : 0x31304E4E414644ULL;
    fwrite_chk(&magic, 8, f);
    uint64_t jlen = h->spec_json.size();
    fwrite_chk(&jlen, 8, f);
    fwrite_chk(h->spec_json.data(), jlen, f);
    int32_t hdr[8] = {h->type, h->metric, h->d, h->nlist, h->m,
                      h->nprobe,
                      // informational (the loader takes the width from the
                      // spec): 0 fp16, 1 8-bit as ever, else the width
                      h->sq_bits == 16 ? 0 : h->sq_bits == 8 ? 1 : h->sq_bits,
                      h->stride};
    fwrite_chk(hdr, sizeof(hdr), f);
    uint8_t tr = h->trained ? 1 : 0;
    fwrite_chk(&tr, 1, f);
    fwrite_chk(&h->ntotal, 8, f);
    if (v2) {
      const int64_t nlive = h->nlive();
      fwrite_chk(&nlive, 8, f);
    }
    if (h->trained && h->type != T_FLAT) {
      if (h->type != T_HNSW)
        dump_dev(f, h->centroids, (size_t)h->nlist * h->d * 4);
      if (h->type == T_IVFPQ)
        dump_dev(f, h->codebooks, (size_t)h->m * pq_ksub(h) * h->dsub * 4);
      if (h->opq)  // only when the spec carries "opq": older files are as before
        dump_dev(f, h->opq_A, (size_t)h->d * h->d_in * 4);
      if ((h->type == T_IVFSQ || h->type == T_HNSW) && h->sq_int()) {
        dump_dev(f, h->sq_vmin, (size_t)h->d * 4);
        dump_dev(f, h->sq_vdiff, (size_t)h->d * 4);
      }
    }
    if (h->type == T_HNSW) {
      // codes (arrival order) + the graph
      const int64_t CHROWS =
          std::max<int64_t>(1, ((int64_t)64 << 20) / h->stride);
      std::vector<char> tmp((size_t)CHROWS * h->stride);
      for (int64_t r = 0; r < h->ntotal; r += CHROWS) {
        int64_t c = std::min(CHROWS, h->ntotal - r);
        h->csr_arena.copy_rows_to_host(tmp.data(), r, c);
        fwrite_chk(tmp.data(), (size_t)c * h->stride, f);
      }
      int32_t meta[4] = {h->hnsw_entry, h->hnsw_maxlevel, h->hnsw_nslots,
                         h->hnsw_efc};
      fwrite_chk(meta, sizeof(meta), f);
      fwrite_chk(h->h_levels.data(), (size_t)h->ntotal * 4, f);
      fwrite_chk(h->h_upslot.data(), (size_t)h->ntotal * 4, f);
      dump_dev(f, h->hn_cnt0, (size_t)h->ntotal * 4);
      dump_dev(f, h->hn_nbr0, (size_t)h->ntotal * 2 * h->m * 4);
      dump_dev(f, h->hn_cntU, (size_t)h->hnsw_nslots * HNSW_MAXL * 4);
      dump_dev(f, h->hn_nbrU, (size_t)h->hnsw_nslots * HNSW_MAXL * h->m * 4);
    } else if (h->type == T_FLAT) {
      dump_dev(f, h->flat, (size_t)h->ntotal * h->d * 4);
      if (v2)
        fwrite_chk(h->h_flat_live.data(), (size_t)((h->ntotal + 31) / 32) * 4,
                   f);
    } else if (h->ntotal) {
      fwrite_chk(h->h_off.data(), (size_t)(h->nlist + 1) * 8, f);
      dump_dev(f, h->cr_ids, (size_t)h->csr_rows * 8);
      // codes: slab arena -> file in CSR row order (same byte layout as
      // the round-1 contiguous image)
      const int64_t CHROWS = std::max<int64_t>(1, ((int64_t)64 << 20) / h->stride);
      std::vector<char> tmp((size_t)CHROWS * h->stride);
      for (int64_t r = 0; r < h->csr_rows; r += CHROWS) {
        int64_t c = std::min(CHROWS, h->csr_rows - r);
        h->csr_arena.copy_rows_to_host(tmp.data(), r, c);
        fwrite_chk(tmp.data(), (size_t)c * h->stride, f);
      }
    }
    if (h->refine && h->ntotal) {
      // refine payload (only when the spec carries "refine", which the
      // loader reads back from the same file): the store's ntotal rows
      // in row (= arrival id) order
      const SlabArena &ra = h->refine_arena;
      const int64_t CHROWS = std::max<int64_t>(1, ((int64_t)64 << 20) / ra.stride);
      std::vector<char> tmp((size_t)std::min(CHROWS, h->ntotal) * ra.stride);
      for (int64_t r = 0; r < h->ntotal; r += CHROWS) {
        int64_t c = std::min(CHROWS, h->ntotal - r);
        ra.copy_rows_to_host(tmp.data(), r, c);
        fwrite_chk(tmp.data(), (size_t)c * ra.stride, f);
      }
    }
  } catch (...) {
    fclose(f);
    throw;
  }
  fclose(f);
  API_END
}

extern "C" int dfann_load(const char *path, dfann_index **out) {
  API_BEGIN
  FILE *f = fopen(path, "rb");
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  dfann_index *h = nullptr;
  try {
    uint64_t magic;
    fread_chk(&magic, 8, f);
    const bool v2 = magic == 0x32304E4E414644ULL;  // "DFANN02": see dfann_save
    if (magic != 0x31304E4E414644ULL && !v2)
      throw std::runtime_error("bad dfann file magic");
    uint64_t jlen;
    fread_chk(&jlen, 8, f);
    std::string js(jlen, 0);
    fread_chk(&js[0], jlen, f);
    h = create_from_spec(js);
    int32_t hdr[8];
    fread_chk(hdr, sizeof(hdr), f);
    h->nprobe = hdr[5];
    uint8_t tr;
    fread_chk(&tr, 1, f);
    fread_chk(&h->ntotal, 8, f);
    int64_t nlive = h->ntotal;
    if (v2) fread_chk(&nlive, 8, f);
    if (nlive < 0 || nlive > h->ntotal)
      throw std::runtime_error("dfann file: nlive outside 0..ntotal");
    h->nremoved = h->ntotal - nlive;
    h->trained = tr != 0;
    if (h->trained && h->type == T_HNSW) {
      load_dev(f, h->sq_vmin, (size_t)h->d * 4);
      load_dev(f, h->sq_vdiff, (size_t)h->d * 4);
      std::vector<float> vd(h->d), sc(h->d);
      HIP_CHECK(hipMemcpy(vd.data(), h->sq_vdiff.p, (size_t)h->d * 4,
                          hipMemcpyDeviceToHost));
      for (int t = 0; t < h->d; ++t) sc[t] = vd[t] / 255.0f;
      h->sq_scale.ensure((size_t)h->d * 4);
      HIP_CHECK(hipMemcpy(h->sq_scale.p, sc.data(), (size_t)h->d * 4,
                          hipMemcpyHostToDevice));
    } else if (h->trained && h->type != T_FLAT) {
      load_dev(f, h->centroids, (size_t)h->nlist * h->d * 4);
      h->cnorm.ensure((size_t)h->nlist * 4);
      rownorms(h->centroids.as<float>(), h->nlist, h->d, h->cnorm.as<float>(), 0);
      if (h->type == T_IVFPQ)
        load_dev(f, h->codebooks, (size_t)h->m * pq_ksub(h) * h->dsub * 4);
      if (h->opq) {
        load_dev(f, h->opq_A, (size_t)h->d * h->d_in * 4);
        opq_install(h, 0);
      }
      refresh_cent_bf16(h, 0);
      if (h->type == T_IVFSQ && h->sq_int()) {
        load_dev(f, h->sq_vmin, (size_t)h->d * 4);
        load_dev(f, h->sq_vdiff, (size_t)h->d * 4);
        std::vector<float> vd(h->d), sc(h->d);
        HIP_CHECK(hipMemcpy(vd.data(), h->sq_vdiff.p, (size_t)h->d * 4,
                            hipMemcpyDeviceToHost));
        for (int t = 0; t < h->d; ++t) sc[t] = vd[t] / h->sq_q();
        h->sq_scale.ensure((size_t)h->d * 4);
        HIP_CHECK(hipMemcpy(h->sq_scale.p, sc.data(), (size_t)h->d * 4,
                            hipMemcpyHostToDevice));
      }
    }
    if (h->type == T_HNSW) {
      if (h->ntotal) {
        const int64_t CHROWS =
            std::max<int64_t>(1, ((int64_t)64 << 20) / h->stride);
        std::vector<char> tmp((size_t)CHROWS * h->stride);
        for (int64_t r = 0; r < h->ntotal; r += CHROWS) {
          int64_t c = std::min(CHROWS, h->ntotal - r);
          fread_chk(tmp.data(), (size_t)c * h->stride, f);
          h->csr_arena.copy_rows_from_host(tmp.data(), r, c);
        }
        h->csr_arena.rows = h->ntotal;
        int32_t meta[4];
        fread_chk(meta, sizeof(meta), f);
        h->hnsw_entry = meta[0];
        h->hnsw_maxlevel = meta[1];
        h->hnsw_nslots = meta[2];
        h->hnsw_efc = meta[3];
        h->h_levels.resize(h->ntotal);
        h->h_upslot.resize(h->ntotal);
        fread_chk(h->h_levels.data(), (size_t)h->ntotal * 4, f);
        fread_chk(h->h_upslot.data(), (size_t)h->ntotal * 4, f);
        h->hn_levels.ensure((size_t)h->ntotal * 4);
        HIP_CHECK(hipMemcpy(h->hn_levels.p, h->h_levels.data(),
                            (size_t)h->ntotal * 4, hipMemcpyHostToDevice));
        h->hn_upslot.ensure((size_t)h->ntotal * 4);
        HIP_CHECK(hipMemcpy(h->hn_upslot.p, h->h_upslot.data(),
                            (size_t)h->ntotal * 4, hipMemcpyHostToDevice));
        load_dev(f, h->hn_cnt0, (size_t)h->ntotal * 4);
        load_dev(f, h->hn_nbr0, (size_t)h->ntotal * 2 * h->m * 4);
        load_dev(f, h->hn_cntU, (size_t)h->hnsw_nslots * HNSW_MAXL * 4);
        load_dev(f, h->hn_nbrU,
                 (size_t)h->hnsw_nslots * HNSW_MAXL * h->m * 4);
        HIP_CHECK(hipDeviceSynchronize());
      }
    } else if (h->type == T_FLAT) {
      load_dev(f, h->flat, (size_t)h->ntotal * h->d * 4);
      if (v2) {
        h->h_flat_live.resize((size_t)((h->ntotal + 31) / 32));
        fread_chk(h->h_flat_live.data(), h->h_flat_live.size() * 4, f);
        flat_live_extend(h, h->ntotal);  // uploads; sets nothing
      }
    } else if (h->ntotal) {
      h->h_off.resize(h->nlist + 1);
      fread_chk(h->h_off.data(), (size_t)(h->nlist + 1) * 8, f);
      if (h->h_off[0] != 0 || h->h_off[h->nlist] != nlive)
        throw std::runtime_error("dfann file: list offsets do not end at nlive");
      load_dev(f, h->cr_ids, (size_t)nlive * 8);
      {
        // codes: file (CSR row order) -> slab arena
        const int64_t CHROWS =
            std::max<int64_t>(1, ((int64_t)64 << 20) / h->stride);
        std::vector<char> tmp((size_t)CHROWS * h->stride);
        for (int64_t r = 0; r < nlive; r += CHROWS) {
          int64_t c = std::min(CHROWS, nlive - r);
          fread_chk(tmp.data(), (size_t)c * h->stride, f);
          h->csr_arena.copy_rows_from_host(tmp.data(), r, c);
        }
        h->csr_arena.rows = nlive;
        h->csr_rows = nlive;
      }
      h->cr_off.ensure((size_t)(h->nlist + 1) * 8);
      HIP_CHECK(hipMemcpy(h->cr_off.p, h->h_off.data(),
                          (size_t)(h->nlist + 1) * 8, hipMemcpyHostToDevice));
      h->id2pos.ensure((size_t)h->ntotal * 4);
      std::vector<int64_t> ids(nlive);
      if (nlive)
        HIP_CHECK(hipMemcpy(ids.data(), h->cr_ids.p, (size_t)nlive * 8,
                            hipMemcpyDeviceToHost));
      // removed ids keep the sentinel
      std::vector<unsigned> i2p(h->ntotal, 0xFFFFFFFFu);
      for (int64_t j = 0; j < nlive; ++j) {
        if ((uint64_t)ids[j] >= (uint64_t)h->ntotal)
          throw std::runtime_error("dfann file: stored id outside 0..ntotal");
        i2p[ids[j]] = (unsigned)j;
      }
      HIP_CHECK(hipMemcpy(h->id2pos.p, i2p.data(), (size_t)h->ntotal * 4,
                          hipMemcpyHostToDevice));
      HIP_CHECK(hipDeviceSynchronize());
    }
    if (h->refine && h->ntotal) {
      SlabArena &ra = h->refine_arena;
      const int64_t CHROWS = std::max<int64_t>(1, ((int64_t)64 << 20) / ra.stride);
      std::vector<char> tmp((size_t)std::min(CHROWS, h->ntotal) * ra.stride);
      for (int64_t r = 0; r < h->ntotal; r += CHROWS) {
        int64_t c = std::min(CHROWS, h->ntotal - r);
        if (fread(tmp.data(), 1, (size_t)c * ra.stride, f) !=
            (size_t)c * ra.stride)
          throw std::runtime_error(
              "dfann file truncated inside the refine payload (rows " +
              std::to_string(r) + ".." + std::to_string(r + c) + " of " +
              std::to_string(h->ntotal) + ")");
        ra.copy_rows_from_host(tmp.data(), r, c);
      }
      ra.rows = h->ntotal;
      HIP_CHECK(hipDeviceSynchronize());
    }
  } catch (...) {
    fclose(f);
    delete h;
    throw;
  }
  fclose(f);
  *out = h;
  API_END
}

// ---------------------------------------------------------------------------
// HNSW introspection (test plumbing: graph determinism + oracle-shared
// search parity — DESIGN.md §hnsw)
// ---------------------------------------------------------------------------

extern "C" int dfann_hnsw_info(dfann_index *h, int64_t out[6]) {
  API_BEGIN
  if (h->type != T_HNSW) throw std::runtime_error("not an hnswsq index");
  out[0] = h->m;
  out[1] = 2 * h->m;
  out[2] = h->hnsw_nslots;
  out[3] = h->hnsw_entry;
  out[4] = h->hnsw_maxlevel;
  out[5] = h->hnsw_efc;
  API_END
}

extern "C" int dfann_hnsw_dump(dfann_index *h, int32_t *levels_host,
                               int32_t *cnt0_host, int32_t *nbr0_host,
                               int32_t *upslot_host, int32_t *cntU_host,
                               int32_t *nbrU_host) {
  API_BEGIN
  if (h->type != T_HNSW) throw std::runtime_error("not an hnswsq index");
  int64_t n = h->ntotal;
  memcpy(levels_host, h->h_levels.data(), (size_t)n * 4);
  memcpy(upslot_host, h->h_upslot.data(), (size_t)n * 4);
  HIP_CHECK(hipMemcpy(cnt0_host, h->hn_cnt0.p, (size_t)n * 4,
                      hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(nbr0_host, h->hn_nbr0.p, (size_t)n * 2 * h->m * 4,
                      hipMemcpyDeviceToHost));
  if (h->hnsw_nslots) {
    HIP_CHECK(hipMemcpy(cntU_host, h->hn_cntU.p,
                        (size_t)h->hnsw_nslots * HNSW_MAXL * 4,
                        hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(nbrU_host, h->hn_nbrU.p,
                        (size_t)h->hnsw_nslots * HNSW_MAXL * h->m * 4,
                        hipMemcpyDeviceToHost));
  }
  API_END
}

// ---------------------------------------------------------------------------
// timing
// ---------------------------------------------------------------------------

extern "C" int dfann_set_timing(dfann_index *h, int enabled) {
  API_BEGIN
  h->timing = enabled != 0;
  API_END
}

static double sum_events(std::vector<TimingEv> &v) {
  double ms = 0;
  for (auto &e : v) {
    HIP_CHECK(hipEventSynchronize(e.b));
    float el = 0;
    HIP_CHECK(hipEventElapsedTime(&el, e.a, e.b));
    ms += el;
    (void)hipEventDestroy(e.a);
    (void)hipEventDestroy(e.b);
  }
  v.clear();
  return ms;
}

extern "C" int dfann_get_timing(dfann_index *h, dfann_timing *out) {
  API_BEGIN
  out->scan_launches = (int64_t)h->ev_scan.size();
  out->merge_launches = (int64_t)h->ev_merge.size();
  out->lut_launches = (int64_t)h->ev_lut.size();
  out->scan_ms = sum_events(h->ev_scan);
  out->gemm_ms = sum_events(h->ev_gemm);
  out->merge_ms = sum_events(h->ev_merge);
  out->lut_ms = sum_events(h->ev_lut);
  out->scan_rows = h->scan_rows;
  out->scan_bytes = h->scan_bytes;
  out->gemm_flops = h->gemm_flops;
  h->scan_rows = h->scan_bytes = h->gemm_flops = 0;
  API_END
}
