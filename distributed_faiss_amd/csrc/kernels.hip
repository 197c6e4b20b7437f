// dfann — gfx950 (MI355X/CDNA4) kernels for the sharded ANN hot path.
//
// Built from scratch for CDNA4: wave64 everywhere, MFMA f32
// (v_mfma_f32_32x32x2_f32) for the coarse-quantizer / flat distance GEMM,
// inverted-list scans with PQ LUTs / SQ codecs staged in LDS over packed
// HBM code reads, and a threshold-filtered LDS candidate buffer with
// block-wide bitonic selection for every top-k stage.
//
// Numeric contract with the CPU oracle (oracle/core.py header): list-scan
// accumulations are sequential over the reduced axis with fp contraction
// off, so distances are bitwise equal to the oracle given shared trained
// artifacts (PQ ADC, SQ8, SQfp16 paths). The IVF-Flat scan uses a
// 16-lane-tree reduction (documented tolerance path).
//
// Tie-break everywhere: (distance, ascending id); minimize-keys internally
// (IP negated), faiss sign conventions restored at the output edge.

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <type_traits>

#define DFANN_BLOCK 256
#define SEL_CAP 1024            // candidate buffer entries (k <= 512)
#define PAD_POS 0xFFFFFFFFu
#define DFANN_FLT_MAX 3.402823466e+38f

// ---------------------------------------------------------------------------
// slab-arena addressing: code images live in fixed-size slabs of
// (1 << rlog) rows each (DESIGN.md §2 memory plan: the arena grows by
// whole slabs and is recycled slab-by-slab during CSR rebuilds, so the
// engine never holds a 2x contiguous copy). `pos` stays the global CSR
// row index; kernels translate through the device slab-pointer table
// (a few hundred entries, L1-resident).
// ---------------------------------------------------------------------------

__device__ __forceinline__ const uint8_t *slab_row(
    const uint8_t *const *__restrict__ slabs, int rlog, long long pos,
    int stride) {
  return slabs[pos >> rlog] +
         (size_t)(pos & ((1LL << rlog) - 1)) * (size_t)stride;
}

__device__ __forceinline__ uint8_t *slab_row_mut(
    uint8_t *const *__restrict__ slabs, int rlog, long long pos, int stride) {
  return slabs[pos >> rlog] +
         (size_t)(pos & ((1LL << rlog) - 1)) * (size_t)stride;
}

typedef __attribute__((ext_vector_type(16))) float f32x16;

// allow-bitmap test (filtered search): uint32 words, bit i&31 of word
// i>>5. Used with CSR positions (scan, bitmap from k_filter_id2pos) and
// with arrival ids (flat top-k, the caller's bitmap as is).
__device__ __forceinline__ bool pos_allowed(const unsigned *__restrict__ bits,
                                            long long i) {
  return (bits[i >> 5] >> (unsigned)(i & 31)) & 1u;
}

// ---------------------------------------------------------------------------
// selection machinery: threshold-filtered append + block bitonic compact
// LDS carve (16B aligned): float selD[SEL_CAP]; unsigned selP[SEL_CAP];
// int ctrl[4] = {cnt, pad, thrP, 0}; float thrD in ctrl-adjacent slot.
// ---------------------------------------------------------------------------

struct Sel {
  float *d;       // SEL_CAP
  unsigned *p;    // SEL_CAP
  int *cnt;
  float *thrD;
  unsigned *thrP;
};

__device__ __forceinline__ Sel sel_carve(char *base) {
  Sel s;
  s.d = reinterpret_cast<float *>(base);
  s.p = reinterpret_cast<unsigned *>(base + SEL_CAP * 4);
  s.cnt = reinterpret_cast<int *>(base + SEL_CAP * 8);
  s.thrD = reinterpret_cast<float *>(base + SEL_CAP * 8 + 4);
  s.thrP = reinterpret_cast<unsigned *>(base + SEL_CAP * 8 + 8);
  return s;
}
#define SEL_LDS_BYTES (SEL_CAP * 8 + 16)

__device__ __forceinline__ void sel_init(Sel s) {
  if (threadIdx.x == 0) {
    *s.cnt = 0;
    *s.thrD = DFANN_FLT_MAX;
    *s.thrP = PAD_POS;
  }
  for (int i = threadIdx.x; i < SEL_CAP; i += blockDim.x) {
    s.d[i] = DFANN_FLT_MAX;
    s.p[i] = PAD_POS;
  }
}

// lexicographic (dist, pos) — pads (FLT_MAX, PAD_POS) sort last
__device__ __forceinline__ bool sel_less(float d0, unsigned p0, float d1, unsigned p1) {
  return d0 < d1 || (d0 == d1 && p0 < p1);
}

__device__ __forceinline__ void sel_try(Sel s, float dist, unsigned pos) {
  // caller guarantees capacity headroom; threshold is stable between compacts
  if (sel_less(dist, pos, *s.thrD, *s.thrP)) {
    int slot = atomicAdd(s.cnt, 1);
    s.d[slot] = dist;
    s.p[slot] = pos;
  }
}

// block-wide: pad [cnt, CAP), bitonic sort CAP entries, truncate to k.
// Requires a preceding __syncthreads() by the caller.
__device__ void sel_compact(Sel s, int k) {
  int cnt = *s.cnt;
  __syncthreads();
  for (int i = threadIdx.x; i < SEL_CAP; i += blockDim.x) {
    if (i >= cnt) {
      s.d[i] = DFANN_FLT_MAX;
      s.p[i] = PAD_POS;
    }
  }
  for (int kk = 2; kk <= SEL_CAP; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < SEL_CAP; i += blockDim.x) {
        int ixj = i ^ j;
        if (ixj > i) {
          bool asc = ((i & kk) == 0);
          float di = s.d[i], dj = s.d[ixj];
          unsigned pi = s.p[i], pj = s.p[ixj];
          bool swap_needed = asc ? sel_less(dj, pj, di, pi) : sel_less(di, pi, dj, pj);
          if (swap_needed) {
            s.d[i] = dj; s.d[ixj] = di;
            s.p[i] = pj; s.p[ixj] = pi;
          }
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int newcnt = cnt < k ? cnt : k;
    *s.cnt = newcnt;
    if (newcnt >= k) {
      *s.thrD = s.d[k - 1];
      *s.thrP = s.p[k - 1];
    }
  }
  __syncthreads();
}

// returns true if a compact happened (callers re-sync on their own)
__device__ __forceinline__ void sel_guard(Sel s, int k, int max_appends) {
  __syncthreads();
  if (*s.cnt > SEL_CAP - max_appends) sel_compact(s, k);
}

// ---------------------------------------------------------------------------
// register-resident per-thread top-K (K <= 16) — the fast selection path.
// Each thread keeps an ascending (dist, pos) array in registers (static
// indices via full unroll); most elements fail the single arr[K-1] compare.
// Block-wide result: K extraction rounds over the threads' heads.
// ---------------------------------------------------------------------------

template <int K>
struct RegTopK {
  float d[K];
  unsigned p[K];

  __device__ __forceinline__ void init() {
#pragma unroll
    for (int i = 0; i < K; ++i) {
      d[i] = DFANN_FLT_MAX;
      p[i] = PAD_POS;
    }
  }

  __device__ __forceinline__ void push(float nd, unsigned np) {
    if (!sel_less(nd, np, d[K - 1], p[K - 1])) return;
    d[K - 1] = nd;
    p[K - 1] = np;
#pragma unroll
    for (int i = K - 1; i > 0; --i) {
      if (sel_less(d[i], p[i], d[i - 1], p[i - 1])) {
        float td = d[i]; d[i] = d[i - 1]; d[i - 1] = td;
        unsigned tp = p[i]; p[i] = p[i - 1]; p[i - 1] = tp;
      }
    }
  }

  // drop the current head (after it won an extraction round)
  __device__ __forceinline__ void pop_head() {
#pragma unroll
    for (int i = 0; i < K - 1; ++i) {
      d[i] = d[i + 1];
      p[i] = p[i + 1];
    }
    d[K - 1] = DFANN_FLT_MAX;
    p[K - 1] = PAD_POS;
  }
};

// Block-wide merge of per-thread RegTopK heads. Phase 1: each wave
// extracts its own top-k with pure shfl rounds (no barriers); phase 2:
// one barrier, then thread 0 merges the per-wave sorted lists.
// lds: 8*16*8 = 1 KiB scratch. Supports blockDim 256 or 512 (4/8 waves).
#define REGSEL_LDS_BYTES 1152
template <int K>
__device__ void regtopk_block_extract(RegTopK<K> &loc, int k, char *lds,
                                      float *out_d, unsigned *out_p) {
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int nw = blockDim.x >> 6;  // 4 or 8 waves
  float *wvd = reinterpret_cast<float *>(lds);             // [8][K]
  unsigned *wvp = reinterpret_cast<unsigned *>(lds + 8 * K * 4);
  for (int round = 0; round < k; ++round) {
    float cd = loc.d[0];
    unsigned cp = loc.p[0];
    unsigned cl = (unsigned)lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      float od = __shfl_down(cd, o, 64);
      unsigned op = __shfl_down(cp, o, 64);
      unsigned ol = __shfl_down(cl, o, 64);
      if (sel_less(od, op, cd, cp)) { cd = od; cp = op; cl = ol; }
    }
    cd = __shfl(cd, 0, 64);
    cp = __shfl(cp, 0, 64);
    cl = __shfl(cl, 0, 64);
    if (lane == 0) {
      wvd[w * K + round] = cd;
      wvp[w * K + round] = cp;
    }
    if ((unsigned)lane == cl) loc.pop_head();
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int cur[8] = {};
    for (int round = 0; round < k; ++round) {
      int bw = 0;
      float bd = DFANN_FLT_MAX;
      unsigned bp = PAD_POS;
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        if (v < nw) {
          // a wave list holds exactly k entries; exhausted reads as pad
          float bv = cur[v] < k ? wvd[v * K + cur[v]] : DFANN_FLT_MAX;
          unsigned pv = cur[v] < k ? wvp[v * K + cur[v]] : PAD_POS;
          if (v == 0 || sel_less(bv, pv, bd, bp)) { bd = bv; bp = pv; bw = v; }
        }
      }
      out_d[round] = bd;
      out_p[round] = bp;
#pragma unroll
      for (int v = 0; v < 8; ++v)
        if (v == bw) ++cur[v];  // static index (rule 20: no scratch)
    }
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------
// GEMM (fp32 MFMA): C[i][j] = sum_k A[i][k] * B[j][k]   (A: MxK, B: NxK)
// 128x128 tile, 4 waves x (2x2 of 32x32) on v_mfma_f32_32x32x2_f32.
// Operand map (cdna_hip_programming.md §3): lane l feeds A[i=l&31][k=l>>5],
// B[k=l>>5][j=l&31]; C/D: col=lane&31, row=(reg&3)+8*(reg>>2)+4*(lane>>5).
// ---------------------------------------------------------------------------

#define GT 128
#define GK 32

__device__ __forceinline__ float gemm_key(float v, int row, int col,
                                          const float *qn, const float *bn,
                                          int mode) {
  if (mode == 0) return -v;
  if (mode == 1) return bn[col] - 2.0f * v;
  if (mode == 2) return (qn[row] - 2.0f * v) + bn[col];
  return v;
}

// mode: -1 raw ip; 0 key=-ip; 1 key=bn[col]-2ip; 2 key=(qn[row]-2ip)+bn[col]
// (fused epilogue)
extern "C" __global__ __launch_bounds__(256) void k_gemm_nt(
    const float *__restrict__ A, const float *__restrict__ B,
    float *__restrict__ C, int M, int N, int K, int lda, int ldb, int ldc,
    const float *__restrict__ qn, const float *__restrict__ bn, int mode) {
  __shared__ float sA[GT][GK + 1];
  __shared__ float sB[GT][GK + 1];
  int bi = blockIdx.y * GT;
  int bj = blockIdx.x * GT;
  int tid = threadIdx.x;
  int lane = tid & 63, w = tid >> 6;
  int wr = (w >> 1) * 64, wc = (w & 1) * 64;
  f32x16 acc00 = {}, acc01 = {}, acc10 = {}, acc11 = {};
  int rl = lane & 31;
  int klane = lane >> 5;
  for (int k0 = 0; k0 < K; k0 += GK) {
    for (int e = tid; e < GT * GK; e += 256) {
      int r = e >> 5, c = e & 31;  // GK == 32
      sA[r][c] = (bi + r < M && k0 + c < K) ? A[(size_t)(bi + r) * lda + k0 + c] : 0.f;
      sB[r][c] = (bj + r < N && k0 + c < K) ? B[(size_t)(bj + r) * ldb + k0 + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GK; kk += 2) {
      float a0 = sA[wr + rl][kk + klane];
      float a1 = sA[wr + 32 + rl][kk + klane];
      float b0 = sB[wc + rl][kk + klane];
      float b1 = sB[wc + 32 + rl][kk + klane];
      acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
      acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
      acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc10, 0, 0, 0);
      acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc11, 0, 0, 0);
    }
    __syncthreads();
  }
  int row_in_tile_base = (lane >> 5) * 4;
  int col_in_tile = lane & 31;
#pragma unroll
  for (int rg = 0; rg < 16; ++rg) {
    int rit = (rg & 3) + 8 * (rg >> 2) + row_in_tile_base;
    {
      int row = bi + wr + rit, col = bj + wc + col_in_tile;
      if (row < M && col < N)
        C[(size_t)row * ldc + col] = gemm_key(acc00[rg], row, col, qn, bn, mode);
      col = bj + wc + 32 + col_in_tile;
      if (row < M && col < N)
        C[(size_t)row * ldc + col] = gemm_key(acc01[rg], row, col, qn, bn, mode);
      row = bi + wr + 32 + rit;
      col = bj + wc + col_in_tile;
      if (row < M && col < N)
        C[(size_t)row * ldc + col] = gemm_key(acc10[rg], row, col, qn, bn, mode);
      col = bj + wc + 32 + col_in_tile;
      if (row < M && col < N)
        C[(size_t)row * ldc + col] = gemm_key(acc11[rg], row, col, qn, bn, mode);
    }
  }
}

// ---------------------------------------------------------------------------
// bf16 GEMM: C[i][j] = sum_k A[i][k]*B[j][k], A/B bf16 (pre-converted),
// C fp32. v_mfma_f32_16x16x32_bf16, 128x128 tile, 4 waves x (4x4 of
// 16x16). Used for the APPROXIMATE assign/coarse path on huge nlist
// (spec "coarse_bf16") — ~16x the f32 MFMA rate.
// Fragment maps (verified on hardware by tests/test_gpu_parity.py):
//   A: lane l supplies A[i = l&15][k = (l>>4)*8 + e], e in 0..7
//   B: lane l supplies B[k = (l>>4)*8 + e][j = l&15]
//   C/D: col = lane&15, row = (lane>>4)*4 + reg, reg in 0..3
// ---------------------------------------------------------------------------

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) short bf16x8;

extern "C" __global__ void k_f32_to_bf16(const float *__restrict__ in,
                                         long long n,
                                         unsigned short *__restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (long long)gridDim.x * blockDim.x) {
    union { float f; unsigned u; } v;
    v.f = in[i];
    // round-to-nearest-even bf16 truncation
    unsigned lsb = (v.u >> 16) & 1u;
    out[i] = (unsigned short)((v.u + 0x7FFFu + lsb) >> 16);
  }
}

#define GB_T 128
#define GB_K 64

// Store epilogue of the four bf16 GEMM kernels below: the wave's
// acc[TI][4], its tile at (bi + wr, bj + wc) of C, goes out through
// gemm_key (C/D fragment map above). A macro for the same reason as the
// GLDS_* ones further down; #undef-ed with them after the last kernel.
#define GEMM_BF16_STORE_KEYS(TI)                                               \
  int rrow = (lane >> 4) * 4;                                                  \
  _Pragma("unroll") for (int ti = 0; ti < TI; ++ti) {                          \
    _Pragma("unroll") for (int tj = 0; tj < 4; ++tj) {                         \
      _Pragma("unroll") for (int rg = 0; rg < 4; ++rg) {                       \
        int row = bi + wr + ti * 16 + rrow + rg;                               \
        int col = bj + wc + tj * 16 + li;                                      \
        if (row < M && col < N)                                                \
          C[(size_t)row * ldc + col] =                                         \
              gemm_key(acc[ti][tj][rg], row, col, qn, bn, mode);               \
      }                                                                        \
    }                                                                          \
  }

// Double-buffered, T14-scheduled (cdna_hip_programming.md §5.5 T14 /
// Guideline 15): tile t+1's global loads are ISSUED before tile t's MFMA
// phase and their LDS write lands after, behind the other buffer — HBM
// latency hides under the MFMAs, one barrier per K-tile.
extern "C" __global__ __launch_bounds__(256) void k_gemm_bf16_nt(
    const unsigned short *__restrict__ A, const unsigned short *__restrict__ B,
    float *__restrict__ C, int M, int N, int K, int lda, int ldb, int ldc,
    const float *__restrict__ qn, const float *__restrict__ bn, int mode) {
  __shared__ unsigned short sA[2][GB_T][GB_K + 8];
  __shared__ unsigned short sB[2][GB_T][GB_K + 8];
  int bi = blockIdx.y * GB_T;
  int bj = blockIdx.x * GB_T;
  int tid = threadIdx.x;
  int lane = tid & 63, w = tid >> 6;
  int wr = (w >> 1) * 64, wc = (w & 1) * 64;
  f32x4 acc[4][4] = {};
  int li = lane & 15;
  int ke = (lane >> 4) * 8;
  // each thread stages 4 16-B groups per operand per tile
  int r_[4], c8_[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    int e8 = tid + g * 256;
    r_[g] = e8 >> 3;
    c8_[g] = (e8 & 7) * 8;
  }
  uint4 va[4], vb[4];

#define GB_LOAD(K0)                                                            \
  _Pragma("unroll") for (int g = 0; g < 4; ++g) {                              \
    int r = r_[g], c8 = c8_[g];                                                \
    uint4 x = {0, 0, 0, 0}, y = {0, 0, 0, 0};                                  \
    if (bi + r < M) {                                                          \
      if ((K0) + c8 + 7 < K) {                                                 \
        x = *reinterpret_cast<const uint4 *>(                                  \
            &A[(size_t)(bi + r) * lda + (K0) + c8]);                           \
      } else {                                                                 \
        unsigned short tmp[8] = {};                                            \
        for (int t = 0; t < 8; ++t)                                            \
          if ((K0) + c8 + t < K)                                               \
            tmp[t] = A[(size_t)(bi + r) * lda + (K0) + c8 + t];                \
        x = *reinterpret_cast<const uint4 *>(tmp);                             \
      }                                                                        \
    }                                                                          \
    if (bj + r < N) {                                                          \
      if ((K0) + c8 + 7 < K) {                                                 \
        y = *reinterpret_cast<const uint4 *>(                                  \
            &B[(size_t)(bj + r) * ldb + (K0) + c8]);                           \
      } else {                                                                 \
        unsigned short tmp[8] = {};                                            \
        for (int t = 0; t < 8; ++t)                                            \
          if ((K0) + c8 + t < K)                                               \
            tmp[t] = B[(size_t)(bj + r) * ldb + (K0) + c8 + t];                \
        y = *reinterpret_cast<const uint4 *>(tmp);                             \
      }                                                                        \
    }                                                                          \
    va[g] = x;                                                                 \
    vb[g] = y;                                                                 \
  }

#define GB_WRITE(BUF)                                                          \
  _Pragma("unroll") for (int g = 0; g < 4; ++g) {                              \
    *reinterpret_cast<uint4 *>(&sA[BUF][r_[g]][c8_[g]]) = va[g];               \
    *reinterpret_cast<uint4 *>(&sB[BUF][r_[g]][c8_[g]]) = vb[g];               \
  }

#define GB_MFMA(BUF)                                                           \
  _Pragma("unroll") for (int kk = 0; kk < GB_K; kk += 32) {                    \
    _Pragma("unroll") for (int ti = 0; ti < 4; ++ti) {                         \
      bf16x8 a0 = *reinterpret_cast<const bf16x8 *>(                           \
          &sA[BUF][wr + ti * 16 + li][kk + ke]);                               \
      _Pragma("unroll") for (int tj = 0; tj < 4; ++tj) {                       \
        bf16x8 b0 = *reinterpret_cast<const bf16x8 *>(                         \
            &sB[BUF][wc + tj * 16 + li][kk + ke]);                             \
        acc[ti][tj] =                                                          \
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[ti][tj],       \
                                                    0, 0, 0);                  \
      }                                                                        \
    }                                                                          \
  }

  GB_LOAD(0)
  GB_WRITE(0)
  __syncthreads();
  int cur = 0;
  for (int k0 = GB_K; k0 < K; k0 += GB_K) {
    GB_LOAD(k0)      // in flight during the MFMAs below
    GB_MFMA(cur)
    GB_WRITE(cur ^ 1)  // waits the loads; other buffer, so no barrier first
    __syncthreads();
    cur ^= 1;
  }
  GB_MFMA(cur)

  GEMM_BF16_STORE_KEYS(4)
#undef GB_LOAD
#undef GB_WRITE
#undef GB_MFMA
}

// ---------------------------------------------------------------------------
// glds-staged bf16 GEMMs (cdna_hip_programming.md §5 ladder step 3 /
// Guideline 15): global->LDS DMA (16-B wide) stages the next tile while
// the MFMAs run; ONE __shared__ object (a second one de-pipelines glds —
// §5 ".s-level traps" (a)); LDS image is lane-linear, so the bank
// swizzle lives on the SOURCE address and the fragment-read offset
// (rule 21): byte ^= (row&7)<<4 cuts the 16-lane ds_read_b128 group from
// 8-way to 2-way. Requires K % 8 == 0 (host falls back otherwise); ragged
// M/N/K are handled by the stage guards (out-of-range positions stage
// zeros).
//
// The GLDS_* macros below are the one copy of the stage, the MFMA step and
// the double-buffered main loop, for a square tile of edge TILE = 128 or
// 256: TILE/32 waves as 2(M) x TILE/64(N), wave tile (TILE/2) x 64, acc
// [TILE/32][4] f32x4. They are macros, not function templates, because
// the template form changed the register allocation of all three kernels
// (profiles/select_gemm); they are #undef-ed after the last kernel.
// ---------------------------------------------------------------------------

// [buf][operand][row][col] bf16, linear (swizzle on source/read)
#define GLDS_SETUP(TILE)                                                       \
  __shared__ unsigned short smem2[2][2][TILE][GB_K];                           \
  int bi = blockIdx.y * TILE;                                                  \
  int bj = blockIdx.x * TILE;                                                  \
  int tid = threadIdx.x;                                                       \
  int lane = tid & 63, w = tid >> 6;                                           \
  int wr = (w / (TILE / 64)) * (TILE / 2), wc = (w % (TILE / 64)) * 64;        \
  f32x4 acc[TILE / 32][4] = {};                                                \
  int li = lane & 15;                                                          \
  int ke = (lane >> 4) * 8;

// wave w stages rows [w*32, w*32+32) of each operand: 4 glds per operand,
// each covering 64 consecutive 16-B groups (8 rows); TILE*8 groups per
// operand = TILE/32 waves x 4 glds x 64 lanes
#define GLDS_STAGE(BUF, K0)                                                    \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) {                              \
    int g = (w * 4 + i) * 64 + lane; /* group index, lane-linear */            \
    int r = g >> 3;                                                            \
    int c8 = (g & 7) * 8;                                                      \
    int c8s = c8 ^ ((r & 7) << 3); /* source-side XOR swizzle (elements) */    \
    unsigned short *ldst =                                                     \
        &smem2[BUF][0][0][0] + ((size_t)(w * 4 + i) * 64) * 8;                 \
    const unsigned short *ga = &A[(size_t)(bi + r) * lda + (K0) + c8s];        \
    const unsigned short *gb = &B[(size_t)(bj + r) * ldb + (K0) + c8s];        \
    bool oka = (bi + r < M) && ((K0) + c8s + 7 < K);                           \
    bool okb = (bj + r < N) && ((K0) + c8s + 7 < K);                           \
    if (oka)                                                                   \
      __builtin_amdgcn_global_load_lds(                                        \
          (const __attribute__((address_space(1))) unsigned int *)ga,          \
          (__attribute__((address_space(3))) unsigned int *)ldst, 16, 0, 0);   \
    else                                                                       \
      *reinterpret_cast<uint4 *>(                                              \
          &smem2[BUF][0][0][0] + (size_t)g * 8) = uint4{0, 0, 0, 0};           \
    unsigned short *ldstB =                                                    \
        &smem2[BUF][1][0][0] + ((size_t)(w * 4 + i) * 64) * 8;                 \
    if (okb)                                                                   \
      __builtin_amdgcn_global_load_lds(                                        \
          (const __attribute__((address_space(1))) unsigned int *)gb,          \
          (__attribute__((address_space(3))) unsigned int *)ldstB, 16, 0, 0);  \
    else                                                                       \
      *reinterpret_cast<uint4 *>(                                              \
          &smem2[BUF][1][0][0] + (size_t)g * 8) = uint4{0, 0, 0, 0};           \
  }

#define GLDS_MFMA(TILE, BUF)                                                   \
  _Pragma("unroll") for (int kk = 0; kk < GB_K; kk += 32) {                    \
    _Pragma("unroll") for (int tj = 0; tj < 4; ++tj) {                         \
      int rb = wc + tj * 16 + li;                                              \
      int cbx = (kk + ke) ^ ((rb & 7) << 3);                                   \
      bf16x8 b0 = *reinterpret_cast<const bf16x8 *>(&smem2[BUF][1][rb][cbx]);  \
      _Pragma("unroll") for (int ti = 0; ti < TILE / 32; ++ti) {               \
        int ra = wr + ti * 16 + li;                                            \
        int ca = (kk + ke) ^ ((ra & 7) << 3);                                  \
        bf16x8 a0 = *reinterpret_cast<const bf16x8 *>(&smem2[BUF][0][ra][ca]); \
        acc[ti][tj] =                                                          \
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[ti][tj],       \
                                                    0, 0, 0);                  \
      }                                                                        \
    }                                                                          \
  }

#define GLDS_MAINLOOP(TILE)                                                    \
  GLDS_STAGE(0, 0)                                                             \
  __syncthreads();                                                             \
  int cur = 0;                                                                 \
  for (int k0 = GB_K; k0 < K; k0 += GB_K) {                                    \
    GLDS_STAGE(cur ^ 1, k0) /* DMA in flight during the MFMAs */               \
    GLDS_MFMA(TILE, cur)                                                       \
    __syncthreads(); /* drains the glds queue (vmcnt(0) inside) */             \
    cur ^= 1;                                                                  \
  }                                                                            \
  GLDS_MFMA(TILE, cur)

// 128^2 tile, 4 waves: every K % 8 == 0 shape the 256^2 kernel does not
// take
extern "C" __global__ __launch_bounds__(256) void k_gemm_bf16_glds(
    const unsigned short *__restrict__ A, const unsigned short *__restrict__ B,
    float *__restrict__ C, int M, int N, int K, int lda, int ldb, int ldc,
    const float *__restrict__ qn, const float *__restrict__ bn, int mode) {
  GLDS_SETUP(GB_T)
  GLDS_MAINLOOP(GB_T)
  GEMM_BF16_STORE_KEYS(4)
}

// 256^2 tile, 8 waves (cdna_hip_programming.md §5 glds table: 256² BK=64
// 2-buffer glds is the top tier for large GEMMs — the 128² tile peaks
// ~620 TF, this shape ~1.2 PF). Used for the big coarse/assign GEMMs
// (N = nlist >= 2048).
extern "C" __global__ __launch_bounds__(512) void k_gemm_bf16_256(
    const unsigned short *__restrict__ A, const unsigned short *__restrict__ B,
    float *__restrict__ C, int M, int N, int K, int lda, int ldb, int ldc,
    const float *__restrict__ qn, const float *__restrict__ bn, int mode) {
  GLDS_SETUP(256)
  GLDS_MAINLOOP(256)
  GEMM_BF16_STORE_KEYS(8)
}

// ---------------------------------------------------------------------------
// k_gemm_bf16_256 with the coarse select fused into the epilogue: same
// staging, swizzle, MFMA loop and accumulator layout (GLDS_SETUP and
// GLDS_MAINLOOP), same gemm_key() on the same accumulators — but C is never
// stored. Each block reduces its 256x256 key tile to the NP smallest
// (key, col) pairs per row (sel_less order) and writes them to a
// candidate buffer laid out (row, n_tile, NP); k_coarse_reduce_rk picks
// the final nprobe. Slots without a valid column stay (FLT_MAX, PAD_POS);
// rows >= M write nothing.
//
// Epilogue: the 128 KB operand buffer is reused as a 256x128 fp32 tile,
// filled in two passes (tj 0-1, then tj 2-3, so all 8 waves store in
// both). Thread t owns row t>>1, 64-column chunk t&1, and streams it
// through a RegTopK<NP> with ds_read_b128; the start slot is rotated by
// t so the 16 lanes of a read group (distinct t mod 16) hit 16 distinct
// 16-B slots of the 256-B bank row. Push order does not matter: (key,
// col) is a strict total order. The two threads of a row then exchange
// their lists by shuffle.
// ---------------------------------------------------------------------------
template <int NP>
__global__ __launch_bounds__(512) void k_gemm_bf16_256_topk(
    const unsigned short *__restrict__ A, const unsigned short *__restrict__ B,
    int M, int N, int K, int lda, int ldb, const float *__restrict__ qn,
    const float *__restrict__ bn, int mode, float *__restrict__ cand_d,
    unsigned *__restrict__ cand_p) {
  GLDS_SETUP(256)
  GLDS_MAINLOOP(256)
  __syncthreads();  // every wave is done with the operand tiles

  float *tile = reinterpret_cast<float *>(&smem2[0][0][0][0]);  // [256][128]
  int rrow = (lane >> 4) * 4;
  int srow = tid >> 1, sch = tid & 1;
  int grow = bi + srow;
  RegTopK<NP> loc;
  loc.init();
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
    if (hf) __syncthreads();  // first half consumed
#pragma unroll
    for (int ti = 0; ti < 8; ++ti) {
#pragma unroll
      for (int tjl = 0; tjl < 2; ++tjl) {
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          int lrow = wr + ti * 16 + rrow + rg;
          int row = bi + lrow;
          int col = bj + wc + (hf * 2 + tjl) * 16 + li;
          float key = DFANN_FLT_MAX;
          if (row < M && col < N)
            key = gemm_key(acc[ti][hf * 2 + tjl][rg], row, col, qn, bn, mode);
          tile[lrow * 128 + (w & 3) * 32 + tjl * 16 + li] = key;
        }
      }
    }
    __syncthreads();
    const float4 *rp =
        reinterpret_cast<const float4 *>(tile + srow * 128 + sch * 64);
#pragma unroll 4
    for (int j = 0; j < 16; ++j) {
      int s = (j + tid) & 15;
      float4 v = rp[s];
      // tile column -> global column (4 consecutive share a 16-col group)
      int lc = sch * 64 + s * 4;
      int col = bj + (lc >> 5) * 64 + (hf * 2 + ((lc >> 4) & 1)) * 16 +
                (lc & 15);
      if (grow < M) {
        if (col + 0 < N) loc.push(v.x, (unsigned)(col + 0));
        if (col + 1 < N) loc.push(v.y, (unsigned)(col + 1));
        if (col + 2 < N) loc.push(v.z, (unsigned)(col + 2));
        if (col + 3 < N) loc.push(v.w, (unsigned)(col + 3));
      }
    }
  }
  // merge the row's two 64-column chunks (lanes t, t^1)
  float od[NP];
  unsigned op[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    od[i] = __shfl_xor(loc.d[i], 1, 64);
    op[i] = __shfl_xor(loc.p[i], 1, 64);
  }
#pragma unroll
  for (int i = 0; i < NP; ++i) loc.push(od[i], op[i]);
  if (sch == 0 && grow < M) {
    size_t o = ((size_t)grow * gridDim.x + blockIdx.x) * NP;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      cand_d[o + i] = loc.d[i];
      cand_p[o + i] = loc.p[i];
    }
  }
}

#undef GEMM_BF16_STORE_KEYS
#undef GLDS_SETUP
#undef GLDS_STAGE
#undef GLDS_MFMA
#undef GLDS_MAINLOOP

// ---------------------------------------------------------------------------
// row norms ||x_i||^2, one block per row
// ---------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(256) void k_rownorm(
    const float *__restrict__ x, long long n, int d, float *__restrict__ out) {
  long long row = blockIdx.x;
  if (row >= n) return;
  const float *xp = x + row * d;
  float acc = 0.f;
  for (int t = threadIdx.x; t < d; t += blockDim.x) {
    float v = xp[t];
    acc += v * v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  __shared__ float ws[4];
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) ws[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[row] = ws[0] + ws[1] + ws[2] + ws[3];
}

// ---------------------------------------------------------------------------
// top-k per row over a key matrix (stream-select), pos = base + col.
// out_d/out_p: (rows, k). grid.x = rows. dynamic LDS: SEL_LDS_BYTES.
// ---------------------------------------------------------------------------

#define TOPK_TRY(V, POS)                                                       \
  do {                                                                         \
    unsigned p_ = (POS);                                                       \
    if (!FILT || pos_allowed(allow, p_)) sel_try(s, V, p_);                    \
  } while (0)
#define TOPK_PUSH(V, POS)                                                      \
  do {                                                                         \
    unsigned p_ = (POS);                                                       \
    if (!FILT || pos_allowed(allow, p_)) loc.push(V, p_);                      \
  } while (0)
// FILT: each offer is gated on the ID-space allow bit of pos = col + base
// (flat ids are positions — no translation); rejected columns are skipped.
template <bool FILT>
__device__ __forceinline__ void topk_rows_body(
    const float *__restrict__ keys, long long rows, long long cols,
    long long ldk, int k, unsigned base, long long ldo,
    float *__restrict__ out_d, unsigned *__restrict__ out_p,
    const unsigned *__restrict__ allow) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Sel s = sel_carve(smem);
  long long row = blockIdx.x;
  if (row >= rows) return;
  sel_init(s);
  __syncthreads();
  const float *kp = keys + row * ldk;
  const int BS = blockDim.x;
  if ((ldk & 3) == 0) {
    // float4 row reads (see k_topk_rows_rk) — Sel is order-invariant.
    // Appends are split into TWO guarded half-batches of 2*BS: a single
    // 4*BS batch can exceed the Sel headroom (SEL_CAP - k) at large k —
    // at k=512 the buffer overflowed its LDS carve (caught by
    // test_engine_caps_and_filtered_overfetch).
    const float4 *kp4 = reinterpret_cast<const float4 *>(kp);
    long long c4n = cols >> 2;
    for (long long c0 = 0; c0 < c4n; c0 += BS) {
      long long c4 = c0 + threadIdx.x;
      bool v = c4 < c4n;
      float4 v4 = v ? kp4[c4] : float4{0.f, 0.f, 0.f, 0.f};
      sel_guard(s, k, 2 * BS);
      if (v) {
        TOPK_TRY(v4.x, (unsigned)(c4 * 4 + 0) + base);
        TOPK_TRY(v4.y, (unsigned)(c4 * 4 + 1) + base);
      }
      sel_guard(s, k, 2 * BS);
      if (v) {
        TOPK_TRY(v4.z, (unsigned)(c4 * 4 + 2) + base);
        TOPK_TRY(v4.w, (unsigned)(c4 * 4 + 3) + base);
      }
    }
    sel_guard(s, k, BS);
    for (long long c = (c4n << 2) + threadIdx.x; c < cols; c += BS)
      TOPK_TRY(kp[c], (unsigned)c + base);
  } else {
    for (long long c0 = 0; c0 < cols; c0 += (long long)2 * BS) {
      sel_guard(s, k, 2 * BS);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        long long c = c0 + u * BS + threadIdx.x;
        if (c < cols) TOPK_TRY(kp[c], (unsigned)c + base);
      }
    }
  }
  __syncthreads();
  sel_compact(s, k);
  int cnt = *s.cnt;
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    bool v = j < cnt;
    out_d[row * ldo + j] = v ? s.d[j] : DFANN_FLT_MAX;
    out_p[row * ldo + j] = v ? s.p[j] : PAD_POS;
  }
}

// register-path top-k per row (k <= 16): no LDS buffer, no bitonic
template <bool FILT>
__device__ __forceinline__ void topk_rows_rk_body(
    const float *__restrict__ keys, long long rows, long long cols,
    long long ldk, int k, unsigned base, long long ldo,
    float *__restrict__ out_d, unsigned *__restrict__ out_p,
    const unsigned *__restrict__ allow) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  long long row = blockIdx.x;
  if (row >= rows) return;
  RegTopK<16> loc;
  loc.init();
  const float *kp = keys + row * ldk;
  // float4 row reads (1 KB per wave-load instead of 256 B) + 2 vectors
  // in flight: the 4 B/lane version capped the 8192x65536 coarse top-k
  // at ~1.5 TB/s. Lane->element assignment changes, result does not
  // (RegTopK extraction orders globally by (dist, id)).
  const long long BS = blockDim.x;
  if ((ldk & 3) == 0) {  // float4-aligned rows
    const float4 *kp4 = reinterpret_cast<const float4 *>(kp);
    long long c4n = cols >> 2;
    long long c4 = threadIdx.x;
    for (; c4 + BS < c4n; c4 += 2 * BS) {
      float4 v0 = kp4[c4], v1 = kp4[c4 + BS];
      TOPK_PUSH(v0.x, (unsigned)(c4 * 4 + 0) + base);
      TOPK_PUSH(v0.y, (unsigned)(c4 * 4 + 1) + base);
      TOPK_PUSH(v0.z, (unsigned)(c4 * 4 + 2) + base);
      TOPK_PUSH(v0.w, (unsigned)(c4 * 4 + 3) + base);
      TOPK_PUSH(v1.x, (unsigned)((c4 + BS) * 4 + 0) + base);
      TOPK_PUSH(v1.y, (unsigned)((c4 + BS) * 4 + 1) + base);
      TOPK_PUSH(v1.z, (unsigned)((c4 + BS) * 4 + 2) + base);
      TOPK_PUSH(v1.w, (unsigned)((c4 + BS) * 4 + 3) + base);
    }
    for (; c4 < c4n; c4 += BS) {
      float4 v0 = kp4[c4];
      TOPK_PUSH(v0.x, (unsigned)(c4 * 4 + 0) + base);
      TOPK_PUSH(v0.y, (unsigned)(c4 * 4 + 1) + base);
      TOPK_PUSH(v0.z, (unsigned)(c4 * 4 + 2) + base);
      TOPK_PUSH(v0.w, (unsigned)(c4 * 4 + 3) + base);
    }
    for (long long c = (c4n << 2) + threadIdx.x; c < cols; c += BS)
      TOPK_PUSH(kp[c], (unsigned)c + base);
  } else {
    for (long long c = threadIdx.x; c < cols; c += BS)
      TOPK_PUSH(kp[c], (unsigned)c + base);
  }
  __syncthreads();
  regtopk_block_extract<16>(loc, k, smem, out_d + row * ldo,
                            out_p + row * ldo);
}

#undef TOPK_TRY
#undef TOPK_PUSH

extern "C" __global__ __launch_bounds__(256) void k_topk_rows(
    const float *__restrict__ keys, long long rows, long long cols,
    long long ldk, int k, unsigned base, long long ldo,
    float *__restrict__ out_d, unsigned *__restrict__ out_p) {
  topk_rows_body<false>(keys, rows, cols, ldk, k, base, ldo, out_d, out_p,
                        nullptr);
}

extern "C" __global__ __launch_bounds__(256) void k_topk_rows_f(
    const float *__restrict__ keys, long long rows, long long cols,
    long long ldk, int k, unsigned base, long long ldo,
    float *__restrict__ out_d, unsigned *__restrict__ out_p,
    const unsigned *__restrict__ allow) {
  topk_rows_body<true>(keys, rows, cols, ldk, k, base, ldo, out_d, out_p,
                       allow);
}

extern "C" __global__ __launch_bounds__(256) void k_topk_rows_rk(
    const float *__restrict__ keys, long long rows, long long cols,
    long long ldk, int k, unsigned base, long long ldo,
    float *__restrict__ out_d, unsigned *__restrict__ out_p) {
  topk_rows_rk_body<false>(keys, rows, cols, ldk, k, base, ldo, out_d, out_p,
                           nullptr);
}

extern "C" __global__ __launch_bounds__(256) void k_topk_rows_rk_f(
    const float *__restrict__ keys, long long rows, long long cols,
    long long ldk, int k, unsigned base, long long ldo,
    float *__restrict__ out_d, unsigned *__restrict__ out_p,
    const unsigned *__restrict__ allow) {
  topk_rows_rk_body<true>(keys, rows, cols, ldk, k, base, ldo, out_d, out_p,
                          allow);
}

// second stage of the fused coarse select: per query row, the top k of
// the ncand = n_tile * NP candidates by (key, pos); pads are skipped.
// Output layout as k_topk_rows_rk with ldo = k. blockDim: 64..256.
extern "C" __global__ __launch_bounds__(256) void k_coarse_reduce_rk(
    const float *__restrict__ cand_d, const unsigned *__restrict__ cand_p,
    long long rows, int ncand, int k, float *__restrict__ out_d,
    unsigned *__restrict__ out_p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  long long row = blockIdx.x;
  if (row >= rows) return;
  RegTopK<16> loc;
  loc.init();
  const float *cd = cand_d + row * ncand;
  const unsigned *cp = cand_p + row * ncand;
  for (int c = threadIdx.x; c < ncand; c += blockDim.x) {
    unsigned p = cp[c];
    if (p != PAD_POS) loc.push(cd[c], p);
  }
  __syncthreads();
  regtopk_block_extract<16>(loc, k, smem, out_d + row * k, out_p + row * k);
}

// ---------------------------------------------------------------------------
// running argmin across key-matrix chunks (assignment). rows = points.
// best_v/best_i persist across chunk calls (init by k_assign_init).
// Ties: lowest global column (chunks ascending, strict <).
// ---------------------------------------------------------------------------

extern "C" __global__ void k_assign_init(float *best_v, int *best_i, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    best_v[i] = DFANN_FLT_MAX;
    best_i[i] = -1;
  }
}

// block-per-row running argmin: 256 threads reduce a row of the key
// matrix (a serial per-thread variant was the train-time bottleneck at
// nlist=65536: 1 thread x 65536 sequential reads).
// Ties: lowest column; running compare strict < keeps the earlier
// (lower-col) chunk on ties.
extern "C" __global__ __launch_bounds__(256) void k_assign_rowblock(
    const float *__restrict__ keys, long long rows, long long cols,
    long long ldk, int col_base, float *__restrict__ best_v,
    int *__restrict__ best_i) {
  long long r = blockIdx.x;
  if (r >= rows) return;
  const float *kp = keys + r * ldk;
  float bv = DFANN_FLT_MAX;
  int bi = 0x7FFFFFFF;
  // float4 row reads where aligned (1 KB/wave-load; see k_topk_rows_rk).
  // (value, column) tie-break everywhere -> lane assignment irrelevant.
  if ((ldk & 3) == 0) {
    const float4 *kp4 = reinterpret_cast<const float4 *>(kp);
    long long c4n = cols >> 2;
    long long c4 = threadIdx.x;
    for (; c4 < c4n; c4 += blockDim.x) {
      float4 v4 = kp4[c4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float v = t == 0 ? v4.x : t == 1 ? v4.y : t == 2 ? v4.z : v4.w;
        int c = (int)(c4 * 4 + t);
        if (v < bv || (v == bv && c < bi)) { bv = v; bi = c; }
      }
    }
    for (long long c = (c4n << 2) + threadIdx.x; c < cols; c += blockDim.x) {
      float v = kp[c];
      if (v < bv || (v == bv && (int)c < bi)) { bv = v; bi = (int)c; }
    }
  } else {
    for (long long c = threadIdx.x; c < cols; c += blockDim.x) {
      float v = kp[c];
      if (v < bv || (v == bv && (int)c < bi)) { bv = v; bi = (int)c; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    float ov = __shfl_down(bv, o, 64);
    int oi = __shfl_down(bi, o, 64);
    if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  __shared__ float wv[4];
  __shared__ int wi[4];
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { wv[w] = bv; wi[w] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i)
      if (wv[i] < bv || (wv[i] == bv && wi[i] < bi)) { bv = wv[i]; bi = wi[i]; }
    if (bv < best_v[r]) {
      best_v[r] = bv;
      best_i[r] = col_base + bi;
    }
  }
}

// ---------------------------------------------------------------------------
// IVF list scan. One block per (query, probe). FAM: 0=PQ, 1=IVF-Flat,
// 2=SQ8 / SQ6 / SQ4 (SQB), 3=SQfp16. IP: minimize-key = -(bias + sum).
// LDS: [fam region (fam_floats)] [SEL].
// cand_d/cand_p: (nq, nprobe, k); pos = CSR row (uint32).
// keys_dev: coarse minimize-keys (IP bias = -key); null for L2.
// ---------------------------------------------------------------------------

// per-row distance (shared by both selection paths); fam = staged LDS
// region (FAM 0: LUT; FAM 2: [target][vmin][scale]; FAM 3: target).
// Loads are issued in 64-byte batches (4x uint4 up front) so the HBM
// latency of a row's chunks overlaps instead of chaining — the
// accumulation ORDER is unchanged (sequential over the reduced axis,
// contract off), so the oracle bit-exactness contract holds.

// (float) cast: identity for f32 LUTs, h->f32 convert for the fp16-LUT
// approximation path (pq_lut_f16) — the accumulation itself stays f32
#define DFANN_PROC16_PQ(WV, G)                                                 \
  if ((G) < m) {                                                               \
    unsigned w0_ = (WV).x, w1_ = (WV).y, w2_ = (WV).z, w3_ = (WV).w;           \
    _Pragma("unroll") for (int b = 0; b < 16; ++b) {                           \
      if ((G) + b < m) {                                                       \
        unsigned word = (b < 4) ? w0_ : (b < 8) ? w1_ : (b < 12) ? w2_ : w3_;  \
        unsigned c = (word >> ((b & 3) * 8)) & 0xFFu;                          \
        acc = acc + (float)lut[((G) + b) * 256 + c];                           \
      }                                                                        \
    }                                                                          \
  }

// m % 16 == 0: no per-code guard can fire, so a group is straight-line
// code — the 16 lookups are issued back to back and summed afterwards
// (the guarded form's branches made every lookup wait out its own LDS
// round trip). Same ascending-order f32 sum -> same bits.
#define DFANN_PROC16_PQ_FULL(WV, G)                                            \
  if ((G) < m) {                                                               \
    unsigned w0_ = (WV).x, w1_ = (WV).y, w2_ = (WV).z, w3_ = (WV).w;           \
    float v_[16];                                                              \
    _Pragma("unroll") for (int b = 0; b < 16; ++b) {                           \
      unsigned word = (b < 4) ? w0_ : (b < 8) ? w1_ : (b < 12) ? w2_ : w3_;    \
      unsigned c = (word >> ((b & 3) * 8)) & 0xFFu;                            \
      v_[b] = (float)lut[((G) + b) * 256 + c];                                 \
    }                                                                          \
    _Pragma("unroll") for (int b = 0; b < 16; ++b) acc = acc + v_[b];          \
  }

// 4-bit PQ (nbits=4): a 16-byte word carries 32 codes,
// code b in nibble (b & 7) of dword b / 8 (byte b/2, even code low —
// the faiss ProductQuantizer bit order). LUT rows are 16 floats, so a
// lane's lookup lands on bank (j*16 + c) % 64: at most 16 distinct
// addresses on 16 distinct banks per sub-quantizer.
#define DFANN_PQ4_CODE(W0, W1, W2, W3, B)                                      \
  (((((B) < 8) ? (W0) : ((B) < 16) ? (W1) : ((B) < 24) ? (W2) : (W3)) >>       \
    (((B) & 7) * 4)) & 0xFu)

#define DFANN_PROC32_PQ4(WV, G)                                                \
  if ((G) < m) {                                                               \
    unsigned w0_ = (WV).x, w1_ = (WV).y, w2_ = (WV).z, w3_ = (WV).w;           \
    _Pragma("unroll") for (int b = 0; b < 32; ++b) {                           \
      if ((G) + b < m) {                                                       \
        unsigned c = DFANN_PQ4_CODE(w0_, w1_, w2_, w3_, b);                    \
        acc = acc + lut[((G) + b) * 16 + c];                                   \
      }                                                                        \
    }                                                                          \
  }

// m % 32 == 0: straight-line group, as DFANN_PROC16_PQ_FULL — the 32
// lookups are issued back to back, then summed in ascending order.
#define DFANN_PROC32_PQ4_FULL(WV, G)                                           \
  if ((G) < m) {                                                               \
    unsigned w0_ = (WV).x, w1_ = (WV).y, w2_ = (WV).z, w3_ = (WV).w;           \
    float v_[32];                                                              \
    _Pragma("unroll") for (int b = 0; b < 32; ++b) {                           \
      unsigned c = DFANN_PQ4_CODE(w0_, w1_, w2_, w3_, b);                      \
      v_[b] = lut[((G) + b) * 16 + c];                                         \
    }                                                                          \
    _Pragma("unroll") for (int b = 0; b < 32; ++b) acc = acc + v_[b];          \
  }

// SQ8 distance with the decode algebra FOLDED:
// L2:  diff = u[t] - c*v[t],  u = (q-cent-vmin) - 0.5*scale, v = scale
// IP:  acc += u[t] + c*v[t],  u = q*vmin + 0.5*(q*scale),   v = q*scale
// — mathematically the faiss codec, op-for-op mirrored by the oracle
// (oracle/core.py OracleIVFSQ._scan_one) so distances stay bitwise equal.
// v_cvt_f32_ubyteN converts the byte exactly (one instruction).
// (float)((w >> 8n) & 0xff) — LLVM selects v_cvt_f32_ubyteN for this
#define DFANN_CVT_UB(WORD, B) ((float)(((WORD) >> (((B) & 3) * 8)) & 0xFFu))

#define DFANN_PROC16_SQ8(WV, G)                                                \
  if ((G) < d) {                                                               \
    unsigned w0_ = (WV).x, w1_ = (WV).y, w2_ = (WV).z, w3_ = (WV).w;           \
    _Pragma("unroll") for (int b = 0; b < 16; ++b) {                           \
      if ((G) + b < d) {                                                       \
        unsigned word = (b < 4) ? w0_ : (b < 8) ? w1_ : (b < 12) ? w2_ : w3_;  \
        float cf = DFANN_CVT_UB(word, b);                                      \
        int t = (G) + b;                                                       \
        if (IS_IP) {                                                           \
          acc = acc + (ubuf[t] + cf * vbuf[t]);                                \
        } else {                                                               \
          float diff = ubuf[t] - cf * vbuf[t];                                 \
          acc = acc + diff * diff;                                             \
        }                                                                      \
      }                                                                        \
    }                                                                          \
  }

#define DFANN_PROC8_F16(WV, G)                                                 \
  if ((G) < d) {                                                               \
    _Pragma("unroll") for (int b = 0; b < 8; ++b) {                            \
      if ((G) + b < d) {                                                       \
        unsigned word = (b < 2) ? (WV).x : (b < 4) ? (WV).y                    \
                                 : (b < 6) ? (WV).z : (WV).w;                  \
        unsigned hv = (word >> ((b & 1) * 16)) & 0xFFFFu;                      \
        float dec = __half2float(__ushort_as_half((unsigned short)hv));        \
        int t = (G) + b;                                                       \
        if (IS_IP) acc = acc + rbuf[t] * dec;                                  \
        else {                                                                 \
          float diff = rbuf[t] - dec;                                          \
          acc = acc + diff * diff;                                             \
        }                                                                      \
      }                                                                        \
    }                                                                          \
  }

template <int FAM, bool IS_IP, bool L16 = false, bool N4 = false>
__device__ __forceinline__ float scan_row_dist(const uint8_t *__restrict__ cp,
                                               const float *__restrict__ fam,
                                               int d, int m) {
  float acc = 0.f;
  const uint4 zero4 = {0, 0, 0, 0};
  if (FAM == 0 && N4) {
    // 64-byte batches = 128 codes; word w is loaded iff it holds a code
    // (32w < m), and then lies wholly inside the row: stride is
    // ceil16((m + 1) / 2) > 16w
    const float *lut = fam;
    if ((m & 31) == 0) {  // wave-uniform
      for (int g0 = 0; g0 < m; g0 += 128) {
#pragma clang fp contract(off)
        const uint8_t *rp = cp + (g0 >> 1);
        uint4 wa = *reinterpret_cast<const uint4 *>(rp);
        uint4 wb = (g0 + 32 < m) ? *reinterpret_cast<const uint4 *>(rp + 16) : zero4;
        uint4 wc = (g0 + 64 < m) ? *reinterpret_cast<const uint4 *>(rp + 32) : zero4;
        uint4 wd4 = (g0 + 96 < m) ? *reinterpret_cast<const uint4 *>(rp + 48) : zero4;
        DFANN_PROC32_PQ4_FULL(wa, g0)
        DFANN_PROC32_PQ4_FULL(wb, g0 + 32)
        DFANN_PROC32_PQ4_FULL(wc, g0 + 64)
        DFANN_PROC32_PQ4_FULL(wd4, g0 + 96)
      }
      return acc;
    }
    for (int g0 = 0; g0 < m; g0 += 128) {
#pragma clang fp contract(off)
      const uint8_t *rp = cp + (g0 >> 1);
      uint4 wa = *reinterpret_cast<const uint4 *>(rp);
      uint4 wb = (g0 + 32 < m) ? *reinterpret_cast<const uint4 *>(rp + 16) : zero4;
      uint4 wc = (g0 + 64 < m) ? *reinterpret_cast<const uint4 *>(rp + 32) : zero4;
      uint4 wd4 = (g0 + 96 < m) ? *reinterpret_cast<const uint4 *>(rp + 48) : zero4;
      DFANN_PROC32_PQ4(wa, g0)
      DFANN_PROC32_PQ4(wb, g0 + 32)
      DFANN_PROC32_PQ4(wc, g0 + 64)
      DFANN_PROC32_PQ4(wd4, g0 + 96)
    }
  } else if (FAM == 0) {
    using LT = typename std::conditional<L16, __half, float>::type;
    const LT *lut = reinterpret_cast<const LT *>(fam);
    if ((m & 15) == 0) {  // wave-uniform
      for (int g0 = 0; g0 < m; g0 += 64) {
#pragma clang fp contract(off)
        uint4 wa = *reinterpret_cast<const uint4 *>(cp + g0);
        uint4 wb = (g0 + 16 < m) ? *reinterpret_cast<const uint4 *>(cp + g0 + 16) : zero4;
        uint4 wc = (g0 + 32 < m) ? *reinterpret_cast<const uint4 *>(cp + g0 + 32) : zero4;
        uint4 wd4 = (g0 + 48 < m) ? *reinterpret_cast<const uint4 *>(cp + g0 + 48) : zero4;
        DFANN_PROC16_PQ_FULL(wa, g0)
        DFANN_PROC16_PQ_FULL(wb, g0 + 16)
        DFANN_PROC16_PQ_FULL(wc, g0 + 32)
        DFANN_PROC16_PQ_FULL(wd4, g0 + 48)
      }
      return acc;
    }
    for (int g0 = 0; g0 < m; g0 += 64) {
#pragma clang fp contract(off)
      uint4 wa = *reinterpret_cast<const uint4 *>(cp + g0);
      uint4 wb = (g0 + 16 < m) ? *reinterpret_cast<const uint4 *>(cp + g0 + 16) : zero4;
      uint4 wc = (g0 + 32 < m) ? *reinterpret_cast<const uint4 *>(cp + g0 + 32) : zero4;
      uint4 wd4 = (g0 + 48 < m) ? *reinterpret_cast<const uint4 *>(cp + g0 + 48) : zero4;
      DFANN_PROC16_PQ(wa, g0)
      DFANN_PROC16_PQ(wb, g0 + 16)
      DFANN_PROC16_PQ(wc, g0 + 32)
      DFANN_PROC16_PQ(wd4, g0 + 48)
    }
  } else if (FAM == 2) {
    // full-cacheline batches: a row is one 128-B line (stride 128 for
    // d=128); reading it in one 8x-uint4 burst touches the line once —
    // split batches re-fetched it after L1 eviction (229 KB of rows in
    // flight per CU >> 32 KB L1)
    const float *ubuf = fam, *vbuf = fam + d;
    for (int g0 = 0; g0 < d; g0 += 128) {
#pragma clang fp contract(off)
      uint4 wa = *reinterpret_cast<const uint4 *>(cp + g0);
      uint4 wb = (g0 + 16 < d) ? *reinterpret_cast<const uint4 *>(cp + g0 + 16) : zero4;
      uint4 wc = (g0 + 32 < d) ? *reinterpret_cast<const uint4 *>(cp + g0 + 32) : zero4;
      uint4 wd4 = (g0 + 48 < d) ? *reinterpret_cast<const uint4 *>(cp + g0 + 48) : zero4;
      uint4 we = (g0 + 64 < d) ? *reinterpret_cast<const uint4 *>(cp + g0 + 64) : zero4;
      uint4 wf = (g0 + 80 < d) ? *reinterpret_cast<const uint4 *>(cp + g0 + 80) : zero4;
      uint4 wg = (g0 + 96 < d) ? *reinterpret_cast<const uint4 *>(cp + g0 + 96) : zero4;
      uint4 wh = (g0 + 112 < d) ? *reinterpret_cast<const uint4 *>(cp + g0 + 112) : zero4;
      DFANN_PROC16_SQ8(wa, g0)
      DFANN_PROC16_SQ8(wb, g0 + 16)
      DFANN_PROC16_SQ8(wc, g0 + 32)
      DFANN_PROC16_SQ8(wd4, g0 + 48)
      DFANN_PROC16_SQ8(we, g0 + 64)
      DFANN_PROC16_SQ8(wf, g0 + 80)
      DFANN_PROC16_SQ8(wg, g0 + 96)
      DFANN_PROC16_SQ8(wh, g0 + 112)
    }
  } else {  // FAM 3: fp16 codes, 8 dims per 16 B
    const float *rbuf = fam;
    for (int g0 = 0; g0 < d; g0 += 64) {  // 128 B = one line per batch
#pragma clang fp contract(off)
      uint4 wa = *reinterpret_cast<const uint4 *>(cp + (size_t)g0 * 2);
      uint4 wb = (g0 + 8 < d) ? *reinterpret_cast<const uint4 *>(cp + (size_t)(g0 + 8) * 2) : zero4;
      uint4 wc = (g0 + 16 < d) ? *reinterpret_cast<const uint4 *>(cp + (size_t)(g0 + 16) * 2) : zero4;
      uint4 wd4 = (g0 + 24 < d) ? *reinterpret_cast<const uint4 *>(cp + (size_t)(g0 + 24) * 2) : zero4;
      uint4 we = (g0 + 32 < d) ? *reinterpret_cast<const uint4 *>(cp + (size_t)(g0 + 32) * 2) : zero4;
      uint4 wf = (g0 + 40 < d) ? *reinterpret_cast<const uint4 *>(cp + (size_t)(g0 + 40) * 2) : zero4;
      uint4 wg = (g0 + 48 < d) ? *reinterpret_cast<const uint4 *>(cp + (size_t)(g0 + 48) * 2) : zero4;
      uint4 wh = (g0 + 56 < d) ? *reinterpret_cast<const uint4 *>(cp + (size_t)(g0 + 56) * 2) : zero4;
      DFANN_PROC8_F16(wa, g0)
      DFANN_PROC8_F16(wb, g0 + 8)
      DFANN_PROC8_F16(wc, g0 + 16)
      DFANN_PROC8_F16(wd4, g0 + 24)
      DFANN_PROC8_F16(we, g0 + 32)
      DFANN_PROC8_F16(wf, g0 + 40)
      DFANN_PROC8_F16(wg, g0 + 48)
      DFANN_PROC8_F16(wh, g0 + 56)
    }
  }
  return acc;
}

// row sets in flight per wave in the SQ4 / SQ6 scans (ivf_scan_body)
#ifndef DFANN_SQ4_UR
#define DFANN_SQ4_UR 4
#endif
#ifndef DFANN_SQ6_UR
#define DFANN_SQ6_UR 4
#endif

// SQ4 / SQ6 rows: a packed little-endian bit stream, B
// bits per dimension. A lane's chunk is the 16 dims [t0, t0 + 16), t0 a
// multiple of 16: 8 bytes at byte t0 / 2 (B = 4) or 12 bytes at byte
// 3 * t0 / 4 (B = 6), i.e. 2 or 3 aligned dwords holding code b at bit
// B * b. A dword is loaded only if it starts inside the row's code bytes
// (ceil(d * B / 8)); the stride is a multiple of 16, so such a dword lies
// wholly inside the row. That matters for B = 6: at d = 40 the row is 30
// bytes in a 32-byte stride and lane 2's chunk would be bytes 24..35.
template <int B>
__device__ __forceinline__ void sqn_load(const uint8_t *__restrict__ cp, int t0,
                                         int d, unsigned (&w)[3]) {
  const int o = (t0 * B) >> 3;
  if (B == 4) {
    // o is a multiple of 8 below ceil(d / 2): the 8 bytes are in the stride
    uint2 v = *reinterpret_cast<const uint2 *>(cp + o);
    w[0] = v.x;
    w[1] = v.y;
    w[2] = 0u;
    return;
  }
  const int cbytes = (d * B + 7) >> 3;
  const unsigned *wp = reinterpret_cast<const unsigned *>(cp + o);
  if (o + 12 <= cbytes) {  // the common case: one 12-byte load
    w[0] = wp[0];
    w[1] = wp[1];
    w[2] = wp[2];
  } else {  // the row's last chunk: only the dwords that hold a code
    w[0] = wp[0];
    w[1] = (o + 4 < cbytes) ? wp[1] : 0u;
    w[2] = (o + 8 < cbytes) ? wp[2] : 0u;
  }
}

// code b (compile-time) of a chunk: shift and mask, which the compiler
// selects as v_bfe_u32; a 6-bit field that straddles two dwords (b = 5, 10)
// takes the funnel of both
template <int B>
__device__ __forceinline__ unsigned sqn_code(const unsigned (&w)[3], int b) {
  const int bit = B * b, lo = bit >> 5, sh = bit & 31;
  unsigned v = w[lo] >> sh;
  if (sh + B > 32) v |= w[lo + 1] << (32 - sh);
  return v & ((1u << B) - 1u);
}

// one chunk's 16 terms added to `part` in ascending dimension order: the
// SQ8 folded algebra (DFANN_PROC16_SQ8) with cf from the narrower code
template <int B, bool IS_IP>
__device__ __forceinline__ float sqn_accum(const unsigned (&w)[3], int t0,
                                           int d, const float *ubuf,
                                           const float *vbuf, float part) {
#pragma clang fp contract(off)
#pragma unroll
  for (int b = 0; b < 16; ++b) {
    if (t0 + b < d) {
      float cf = (float)sqn_code<B>(w, b);
      int t = t0 + b;
      if (IS_IP) {
        part = part + (ubuf[t] + cf * vbuf[t]);
      } else {
        float diff = ubuf[t] - cf * vbuf[t];
        part = part + diff * diff;
      }
    }
  }
  return part;
}

// The d <= 128 form: a lane's 16 dims never change, so its u / v terms sit
// in registers (0 past d) and the 16 terms are straight-line code, with no
// LDS read and no per-dimension branch. A dimension past d contributes
// u = v = cf = 0 (pad bits are zero, unloaded dwords too): its term is +0,
// and part + (+0) == part bitwise (part starts at +0 and +0 + -0 == +0, so
// it is never -0). Same ascending order, same bits as the guarded form.
template <int B, bool IS_IP>
__device__ __forceinline__ float sqn_accum_reg(const unsigned (&w)[3],
                                               const float (&ur)[16],
                                               const float (&vr)[16],
                                               float part) {
#pragma clang fp contract(off)
#pragma unroll
  for (int b = 0; b < 16; ++b) {
    float cf = (float)sqn_code<B>(w, b);
    if (IS_IP) {
      part = part + (ur[b] + cf * vr[b]);
    } else {
      float diff = ur[b] - cf * vr[b];
      part = part + diff * diff;
    }
  }
  return part;
}

// Range selector: every row whose distance passes the
// radius test, in ascending CSR position. A wave owns a contiguous run of
// rows and its lanes hold them in ascending order, so a hit's rank is the
// wave's running count plus the hits in the lanes below it (ballot +
// masked popcount): no LDS, no atomics, no barrier. Pass 0 counts, pass 1
// writes (value, id) at the offset the exclusive scan of the counts gave.
struct RangeSel {
  float radius;
  int fill;            // 0 = count pass, 1 = fill pass (wave-uniform)
  const int64_t *ids;  // cr_ids
  float *D;
  int64_t *I;
  int *err;            // count / fill disagreement
  long long run, end;  // next output slot; end of this wave's segment
};

// Called by all 64 lanes of a wave together. `val` is the faiss-convention
// value (L2 distance, un-negated dot product).
template <bool IS_IP>
__device__ __forceinline__ void range_offer(RangeSel &r, bool valid, float val,
                                            long long pos) {
  bool hit = valid && (IS_IP ? val > r.radius : val < r.radius);
  unsigned long long b = __ballot(hit);
  if (r.fill && hit) {
    long long slot =
        r.run + __builtin_amdgcn_mbcnt_hi(
                    (unsigned)(b >> 32),
                    __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
    if (slot < r.end) {
      r.D[slot] = val;
      r.I[slot] = r.ids[pos];
    } else {
      *r.err = 1;  // never store outside the counted segment
    }
  }
  r.run += __popcll(b);
}

template <int FAM, bool IS_IP, bool REGSEL, bool PRE, bool GLUT, bool L16,
          bool N4, bool FILT, bool RANGE, int SQB>
__device__ void ivf_scan_body(
    const float *__restrict__ q, const float *__restrict__ cent,
    const float *__restrict__ cb, const float *__restrict__ sq_vmin,
    const float *__restrict__ sq_scale, const int *__restrict__ probes,
    const float *__restrict__ keys, const uint8_t *const *__restrict__ codes,
    const int64_t *__restrict__ off, int nlist, int nq, int nprobe, int d,
    int m, int dsub, int k, int stride, int rlog, float *__restrict__ cand_d,
    unsigned *__restrict__ cand_p, int fam_floats,
    const float *__restrict__ term2, const float *__restrict__ term3,
    const float *__restrict__ qn, int fan, const float *__restrict__ glut,
    const unsigned *__restrict__ posbits, float radius, int range_fill,
    int *__restrict__ range_cnt, const long long *__restrict__ range_off,
    const int64_t *__restrict__ range_lims, const int64_t *__restrict__ cr_ids,
    float *__restrict__ range_D, int64_t *__restrict__ range_I,
    int *__restrict__ range_err) {
  // RANGE: the selector is a RangeSel. The block's rows are split into one
  // contiguous run per wave (row -> lane mapping inside a wave is the
  // top-k scans' with a 64-thread "block"), the counts / offsets are per
  // (query, probe, wave), and the kernel ends after the scan loop.
  // FILT: posbits is the allow-bitmap in CSR-POSITION space (built per
  // call by k_filter_id2pos); a row whose bit is clear is never offered
  // to the selector. The word load is issued next to the row's code load
  // (independent of it), so the test adds no dependent round trip; the
  // row's arithmetic is untouched, so surviving distances are bitwise
  // the unfiltered ones.
  // fan > 1: each (query, probe) list is split into `fan` segments, one
  // block per segment — long-list tail imbalance at low block counts.
  // EXACT results: every segment's top-k contains the segment's global
  // winners; the candidate merge sees (nprobe*fan*k) entries per query.
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *fam = reinterpret_cast<float *>(smem);
  // REGSEL extraction scratch is used only AFTER the scan loop (behind
  // a __syncthreads), so it ALIASES the fam region — the block's LDS is
  // max(fam, scratch), not the sum (m=64 fp16 LUT: 33.4 -> 32 KB,
  // 4 -> 5 blocks/CU; the scan measured occupancy-proportional). The
  // LDS-buffer selection path uses its region DURING the scan: offset.
  char *selbase = REGSEL ? smem : smem + (size_t)fam_floats * 4;
  long long blk = blockIdx.x;
  int bq = (int)(blk / ((long long)nprobe * fan));
  int rest = (int)(blk % ((long long)nprobe * fan));
  int bp = rest / fan, seg = rest % fan;
  int L = probes[(long long)bq * nprobe + bp];
  long long out_base = (((long long)bq * nprobe + bp) * fan + seg) * k;
  // A probe outside [0, nlist) is an empty slot: one
  // unsigned compare, and the empty-list exits below end the block before
  // keys, cent or term2 are read for it.
  long long l0 = 0, l1 = 0;
  if ((unsigned)L < (unsigned)nlist) {
    l0 = off[L];
    l1 = off[L + 1];
  }
  long long len = l1 - l0;
  long long s0 = l0 + len * seg / fan;
  long long s1 = l0 + len * (seg + 1) / fan;
  // (query, probe, wave) slot of the range counts / offsets
  long long ridx = 0;
  if (RANGE)
    ridx = ((long long)bq * nprobe + bp) * (blockDim.x >> 6) +
           (threadIdx.x >> 6);
  if (RANGE && s0 == s1) {
    if (!range_fill && (threadIdx.x & 63) == 0) range_cnt[ridx] = 0;
    return;
  }
  if (s0 == s1) {
    for (int j = threadIdx.x; j < k; j += blockDim.x) {
      cand_d[out_base + j] = DFANN_FLT_MAX;
      cand_p[out_base + j] = PAD_POS;
    }
    return;
  }
  const float *qp = q + (long long)bq * d;
  float bias = 0.f;
  if (IS_IP) bias = -keys[(long long)bq * nprobe + bp];  // q . centroid
  if (PRE)   // full coarse L2 distance: ||q||^2 + (|c|^2 - 2 q.c)
    bias = qn[bq] + keys[(long long)bq * nprobe + bp];

  // --- stage FAM region ---
  if (FAM == 0 && PRE) {
    // LUT from the precomputed tables: 2 row reads instead of the whole
    // codebook; dist = bias + sum_j LUT
    float *lut = fam;
    const float *t2 = term2 + (size_t)L * m * 256;
    const float *t3 = term3 + (size_t)bq * m * 256;
    for (int e = threadIdx.x; e < m * 256; e += blockDim.x)
      lut[e] = t2[e] - 2.0f * t3[e];
  } else if (FAM == 0 && GLUT) {
    // LUT precomputed in HBM by k_pq_lut (one 1-KiB row per (query,
    // probe, subspace)): stage it with coalesced float4 copies instead
    // of recomputing it from the codebook — at m=64 the in-kernel build
    // re-reads the whole 786-KB codebook from L2 per block and is
    // latency-bound (measured: the scan launch runs at ~125 GB/s of
    // algorithmic code bytes at the configs[3] shape). Values are
    // BIT-IDENTICAL to the in-kernel path: k_pq_lut uses the same
    // sequential-t accumulation with contract off.
    // L16: the LUT row is __half (pq_lut_f16 approximation — half the
    // HBM round-trip and half the LDS, 4 blocks/CU at m=64)
    size_t row_elems = (size_t)m * 256;
    uint4 *dst = reinterpret_cast<uint4 *>(fam);
    const uint4 *src = reinterpret_cast<const uint4 *>(
        reinterpret_cast<const char *>(glut) +
        ((size_t)bq * nprobe + bp) * row_elems * (L16 ? 2 : 4));
    int n4 = (int)(row_elems * (L16 ? 2 : 4) / 16);
    // glds: 16-B global->LDS DMA, no VGPR round-trip — the copy is
    // lane-linear (lane i of each pass writes base + i*16), exactly the
    // wave-uniform-base + lane x size form the DMA requires; the
    // staging barrier below drains it (vmcnt(0) under outstanding glds)
    for (int e = threadIdx.x; e < n4; e += blockDim.x) {
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int *)(src + e),
          (__attribute__((address_space(3))) unsigned int *)(dst + e), 16, 0,
          0);
    }
  } else if (FAM == 0) {
    // rbuf (d floats) AFTER the LUT. N4: 16 codewords per sub-quantizer
    // (codebook (m, 16, dsub), LUT m*16 floats), same arithmetic.
    constexpr int KSH = N4 ? 4 : 8, KSUB = 1 << KSH;
    float *lut = fam;
    float *rbuf = fam + (size_t)m * KSUB;
    for (int t = threadIdx.x; t < d; t += blockDim.x)
      rbuf[t] = IS_IP ? qp[t] : qp[t] - cent[(long long)L * d + t];
    __syncthreads();
    for (int e = threadIdx.x; e < m * KSUB; e += blockDim.x) {
      int j = e >> KSH, c = e & (KSUB - 1);
      const float *cbe = cb + ((size_t)j * KSUB + c) * dsub;
      const float *rs = rbuf + j * dsub;
      float acc = 0.f;
      if ((dsub & 3) == 0 && dsub <= 32) {
        // float4 codebook loads (up to 8 in flight); accumulation order
        // unchanged (t ascending, mul+add, contract off) — bit-exact
        float4 cv[8];
        int nv = dsub >> 2;
#pragma unroll
        for (int v = 0; v < 8; ++v)
          if (v < nv) cv[v] = reinterpret_cast<const float4 *>(cbe)[v];
#pragma unroll
        for (int v = 0; v < 8; ++v) {
          if (v < nv) {
#pragma clang fp contract(off)
            for (int tt = 0; tt < 4; ++tt) {
              float cbv = tt == 0 ? cv[v].x : tt == 1 ? cv[v].y
                          : tt == 2 ? cv[v].z : cv[v].w;
              int t = v * 4 + tt;
              if (IS_IP) {
                acc = acc + rs[t] * cbv;
              } else {
                float diff = rs[t] - cbv;
                acc = acc + diff * diff;
              }
            }
          }
        }
      } else {
        for (int t = 0; t < dsub; ++t) {
#pragma clang fp contract(off)
          if (IS_IP) {
            acc = acc + rs[t] * cbe[t];
          } else {
            float diff = rs[t] - cbe[t];
            acc = acc + diff * diff;
          }
        }
      }
      lut[e] = acc;
    }
  } else if (FAM == 1) {
    for (int t = threadIdx.x; t < d; t += blockDim.x) fam[t] = qp[t];
  } else if (FAM == 2) {
    // folded SQ8 terms (see DFANN_PROC16_SQ8); exact op order mirrored in
    // the oracle: 0.5f*scale is an exact exponent decrement
    float *ubuf = fam, *vbuf = fam + d;
    for (int t = threadIdx.x; t < d; t += blockDim.x) {
      float sct = sq_scale[t];
      if (IS_IP) {
        float qsc = qp[t] * sct;
        vbuf[t] = qsc;
        ubuf[t] = qp[t] * sq_vmin[t] + 0.5f * qsc;
      } else {
        float r = qp[t] - cent[(long long)L * d + t];
        ubuf[t] = (r - sq_vmin[t]) - 0.5f * sct;
        vbuf[t] = sct;
      }
    }
  } else {  // SQfp16
    for (int t = threadIdx.x; t < d; t += blockDim.x)
      fam[t] = IS_IP ? qp[t] : qp[t] - cent[(long long)L * d + t];
  }

  RegTopK<16> loc;
  Sel s;
  RangeSel rs;
  // Rows [SCAN_R0, SCAN_R1) are shared by SCAN_NT threads, this one being
  // SCAN_TID: the block's segment, or in range mode the wave's part of it.
  // (Macros, so that the top-k kernels see the expressions they always had
  // and compile to what they compiled to before range mode existed.)
  long long rw0 = 0, rw1 = 0;
#define SCAN_R0 (RANGE ? rw0 : s0)
#define SCAN_R1 (RANGE ? rw1 : s1)
#define SCAN_NT (RANGE ? 64u : blockDim.x)
#define SCAN_TID (RANGE ? (threadIdx.x & 63u) : threadIdx.x)
  if (RANGE) {
    const int W = blockDim.x >> 6, w = threadIdx.x >> 6;
    rw0 = s0 + len * w / W;
    rw1 = s0 + len * (w + 1) / W;
    rs.radius = radius;
    rs.fill = range_fill;
    rs.ids = cr_ids;
    rs.D = range_D;
    rs.I = range_I;
    rs.err = range_err;
    rs.run = 0;
    rs.end = 0;
    if (range_fill) {
      rs.run = range_lims[bq] + range_off[ridx];
      rs.end = rs.run + range_cnt[ridx];
    }
  } else if (REGSEL) {
    loc.init();
  } else {
    s = sel_carve(selbase);
    sel_init(s);
  }
  __syncthreads();

  // --- scan ---
  if (FAM == 1) {
    // 16-lane-per-vector tree reduction (tolerance parity path)
    int sub = threadIdx.x & 15, grp = SCAN_TID >> 4;
    const int NG16 = SCAN_NT >> 4;  // row groups per block (RANGE: wave)
    for (long long base = SCAN_R0; base < SCAN_R1; base += (long long)NG16 * 8) {
      if (!REGSEL) sel_guard(s, k, NG16 * 8);
      for (int u = 0; u < 8; ++u) {
        long long pos = base + (long long)u * NG16 + grp;
        float dist = 0.f;
        bool valid = pos < SCAN_R1;
        bool allow = true;
        if (FILT && valid) allow = pos_allowed(posbits, pos);
        if (valid) {
          const float *vp = reinterpret_cast<const float *>(slab_row(codes, rlog, pos, stride));
          float part = 0.f;
          for (int t = sub; t < d; t += 16) {
#pragma clang fp contract(off)
            if (IS_IP) part = part + fam[t] * vp[t];
            else {
              float diff = fam[t] - vp[t];
              part = part + diff * diff;
            }
          }
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) part += __shfl_xor(part, o, 16);
          dist = IS_IP ? -part : part;
        }
        if (RANGE) {
          range_offer<IS_IP>(rs, valid && allow && sub == 0,
                             IS_IP ? -dist : dist, pos);
        } else if (valid && allow && sub == 0) {
          if (REGSEL) loc.push(dist, (unsigned)pos);
          else sel_try(s, dist, (unsigned)pos);
        }
      }
    }
  } else if (FAM == 2 && SQB != 8) {
    // SQ4 / SQ6: the SQ8 layout below with narrower rows.
    // 8 lanes per row, lane l owning dims {16l + 128c + b}; a wave reads 8
    // consecutive rows as 8 * stride contiguous bytes, 8 B (SQ4) or 12 B
    // (SQ6) per lane and chunk. Same per-lane order, same butterfly, so the
    // sum is bitwise the SQ8 one for the same cf.
    const float *ubuf = fam, *vbuf = fam + d;
    int g8 = threadIdx.x & 7, grp = SCAN_TID >> 3;
    const bool onechunk = d <= 128;
    const int NG8 = SCAN_NT >> 3;
    // row sets in flight per wave (BASELINE.md "SQ4 / SQ6")
    constexpr int UR = SQB == 4 ? DFANN_SQ4_UR : DFANN_SQ6_UR;
    const int t0 = g8 * 16;
    float ur[16], vr[16];  // d <= 128: the lane's terms, see sqn_accum_reg
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      bool in = onechunk && t0 + b < d;
      ur[b] = in ? ubuf[t0 + b] : 0.f;
      vr[b] = in ? vbuf[t0 + b] : 0.f;
    }
    for (long long base = SCAN_R0; base < SCAN_R1; base += (long long)NG8 * UR) {
      if (!REGSEL) sel_guard(s, k, NG8 * UR);
      unsigned wv[UR][3];
      bool val[UR], ok[UR];  // FILT: ok = valid AND allowed (else == val)
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        long long pos = base + (long long)u * NG8 + grp;
        val[u] = pos < SCAN_R1;
        ok[u] = val[u];
        if (FILT && val[u]) ok[u] = pos_allowed(posbits, pos);
        wv[u][0] = wv[u][1] = wv[u][2] = 0u;
        // d <= 128: every row set's loads are issued before any is used
        if (onechunk && val[u] && t0 < d)
          sqn_load<SQB>(slab_row(codes, rlog, pos, stride), t0, d, wv[u]);
      }
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        long long pos = base + (long long)u * NG8 + grp;
        float part = 0.f;
        if (onechunk) {
          part = sqn_accum_reg<SQB, IS_IP>(wv[u], ur, vr, part);
        } else if (val[u]) {
          const uint8_t *cp = slab_row(codes, rlog, pos, stride);
          for (int tc = t0; tc < d; tc += 128) {
            sqn_load<SQB>(cp, tc, d, wv[u]);
            part = sqn_accum<SQB, IS_IP>(wv[u], tc, d, ubuf, vbuf, part);
          }
        }
        part += __shfl_xor(part, 4, 8);
        part += __shfl_xor(part, 2, 8);
        part += __shfl_xor(part, 1, 8);
        float dist = IS_IP ? -(bias + part) : part;
        if (RANGE) {
          range_offer<IS_IP>(rs, ok[u] && g8 == 0, IS_IP ? -dist : dist, pos);
        } else if (ok[u] && g8 == 0) {
          if (REGSEL) loc.push(dist, (unsigned)pos);
          else sel_try(s, dist, (unsigned)pos);
        }
      }
    }
  } else if (FAM == 2) {
    // SQ8: 8 lanes per row — a wave reads 8 consecutive rows as 1 KiB of
    // CONTIGUOUS lines (the streaming-copy access pattern) instead of 64
    // scattered line fragments. Reduction: fixed 3-step butterfly over the
    // 8 lanes, mirrored op-for-op by the oracle (OracleIVFSQ._scan_one) —
    // all lanes converge to the same bitwise sum.
    {
      const float *ubuf = fam, *vbuf = fam + d;
      int g8 = threadIdx.x & 7, grp = SCAN_TID >> 3;  // 32 row-groups
      const bool onechunk = d <= 128;  // lane covers one 16-B chunk
      const int NG8 = SCAN_NT >> 3;  // row groups per block (RANGE: wave)
      // row sets per iteration (8 measured 1.9 -> 1.1 TB/s)
      constexpr int UR = 4;
      for (long long base = SCAN_R0; base < SCAN_R1; base += (long long)NG8 * UR) {
        if (!REGSEL) sel_guard(s, k, NG8 * UR);
        if (onechunk) {
          // issue all UR row-set loads up front: UR independent HBM
          // requests in flight per wave instead of 1 (latency hiding)
          uint4 wv4[UR];
          bool val4[UR];
          bool ok4[UR];  // FILT: row valid AND allowed (else == val4)
#pragma unroll
          for (int u = 0; u < UR; ++u) {
            long long pos = base + (long long)u * NG8 + grp;
            val4[u] = pos < SCAN_R1;
            ok4[u] = val4[u];
            if (FILT && val4[u]) ok4[u] = pos_allowed(posbits, pos);
            int t0 = g8 * 16;
            wv4[u] = (val4[u] && t0 < d)
                         ? *reinterpret_cast<const uint4 *>(
                               slab_row(codes, rlog, pos, stride) + t0)
                         : uint4{0, 0, 0, 0};
          }
#pragma unroll
          for (int u = 0; u < UR; ++u) {
            long long pos = base + (long long)u * NG8 + grp;
            float part = 0.f;
            int t0 = g8 * 16;
            if (t0 < d) {
#pragma clang fp contract(off)
              unsigned w0_ = wv4[u].x, w1_ = wv4[u].y, w2_ = wv4[u].z,
                       w3_ = wv4[u].w;
#pragma unroll
              for (int b = 0; b < 16; ++b) {
                if (t0 + b < d) {
                  unsigned word = (b < 4) ? w0_ : (b < 8) ? w1_ : (b < 12) ? w2_ : w3_;
                  float cf = DFANN_CVT_UB(word, b);
                  int t = t0 + b;
                  if (IS_IP) {
                    part = part + (ubuf[t] + cf * vbuf[t]);
                  } else {
                    float diff = ubuf[t] - cf * vbuf[t];
                    part = part + diff * diff;
                  }
                }
              }
            }
            part += __shfl_xor(part, 4, 8);
            part += __shfl_xor(part, 2, 8);
            part += __shfl_xor(part, 1, 8);
            float dist = IS_IP ? -(bias + part) : part;
            if (RANGE) {
              range_offer<IS_IP>(rs, ok4[u] && g8 == 0, IS_IP ? -dist : dist,
                                 pos);
            } else if (ok4[u] && g8 == 0) {
              if (REGSEL) loc.push(dist, (unsigned)pos);
              else sel_try(s, dist, (unsigned)pos);
            }
          }
        } else {
#pragma unroll
          for (int u = 0; u < UR; ++u) {
            long long pos = base + (long long)u * NG8 + grp;
            bool valid = pos < SCAN_R1;
            bool allow = true;
            if (FILT && valid) allow = pos_allowed(posbits, pos);
            float part = 0.f;
            if (valid) {
              const uint8_t *cp = slab_row(codes, rlog, pos, stride);
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
                    if (IS_IP) {
                      part = part + (ubuf[t] + cf * vbuf[t]);
                    } else {
                      float diff = ubuf[t] - cf * vbuf[t];
                      part = part + diff * diff;
                    }
                  }
                }
              }
            }
            part += __shfl_xor(part, 4, 8);
            part += __shfl_xor(part, 2, 8);
            part += __shfl_xor(part, 1, 8);
            float dist = IS_IP ? -(bias + part) : part;
            if (RANGE) {
              range_offer<IS_IP>(rs, valid && allow && g8 == 0,
                                 IS_IP ? -dist : dist, pos);
            } else if (valid && allow && g8 == 0) {
              if (REGSEL) loc.push(dist, (unsigned)pos);
              else sel_try(s, dist, (unsigned)pos);
            }
          }
        }
      }
    }
  } else if (REGSEL) {
    // independent rows per thread per iteration: their load batches
    // overlap, hiding HBM/L2 latency without any block synchronization.
    // FAM 0 rows are 16-64 B (4 in flight, cheap); FAM 2/3 rows are a
    // full cache line each (8 uint4 in registers), so 2 in flight keeps
    // VGPRs ~100 (5 waves/SIMD) instead of 161 (3 waves).
    // 4-bit PQ (N4) also takes 2: its 32-lookup groups on top of 4 rows'
    // load batches cost 183 VGPRs (2 waves/SIMD); 2 rows are 90 (5 waves)
    // and measured 1.7-2.6x the scan rate (BASELINE.md "4-bit PQ").
    const int UROWS = (FAM == 0 && !N4) ? 4 : 2;
    const int BS = SCAN_NT;
    for (long long base = SCAN_R0; base < SCAN_R1; base += (long long)UROWS * BS) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (u >= UROWS) break;
        long long pos = base + (long long)u * BS + SCAN_TID;
        bool hit = false;  // RANGE: valid and allowed
        float dist = 0.f;
        if (pos < SCAN_R1) {
          bool allow = true;
          if (FILT) allow = pos_allowed(posbits, pos);
          const uint8_t *cp = slab_row(codes, rlog, pos, stride);
          float acc = scan_row_dist<FAM, IS_IP, L16, N4>(cp, fam, d, m);
          dist = IS_IP ? -(bias + acc) : (PRE ? bias + acc : acc);
          if (RANGE) hit = allow;
          else if (allow) loc.push(dist, (unsigned)pos);
        }
        if (RANGE) range_offer<IS_IP>(rs, hit, IS_IP ? -dist : dist, pos);
      }
    }
  } else {
    const int BS = blockDim.x;
    for (long long base = s0; base < s1; base += (long long)2 * BS) {
      sel_guard(s, k, 2 * BS);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        long long pos = base + (long long)u * BS + threadIdx.x;
        if (pos < s1) {
          bool allow = true;
          if (FILT) allow = pos_allowed(posbits, pos);
          const uint8_t *cp = slab_row(codes, rlog, pos, stride);
          float acc = scan_row_dist<FAM, IS_IP, L16, N4>(cp, fam, d, m);
          float dist = IS_IP ? -(bias + acc) : (PRE ? bias + acc : acc);
          if (allow) sel_try(s, dist, (unsigned)pos);
        }
      }
    }
  }
  if (RANGE) {
    // count pass: the wave's total. Fill pass: it must have written
    // exactly the counted segment.
    if ((threadIdx.x & 63) == 0) {
      if (!range_fill) range_cnt[ridx] = (int)rs.run;
      else if (rs.run != rs.end) *range_err = 1;
    }
    return;
  }
#undef SCAN_R0
#undef SCAN_R1
#undef SCAN_NT
#undef SCAN_TID
  __syncthreads();
  if (REGSEL) {
    regtopk_block_extract<16>(loc, k, selbase, cand_d + out_base,
                              cand_p + out_base);
  } else {
    sel_compact(s, k);
    int cnt = *s.cnt;
    for (int j = threadIdx.x; j < k; j += blockDim.x) {
      bool v = j < cnt;
      cand_d[out_base + j] = v ? s.d[j] : DFANN_FLT_MAX;
      cand_p[out_base + j] = v ? s.p[j] : PAD_POS;
    }
  }
}

// ---------------------------------------------------------------------------
// The scan kernels: one signature, one table.
//
// Every scan takes a ScanArgs by value. A kernel reads only the fields its
// mode uses; scan_entry hands ivf_scan_body literal nullptr / 1 for the
// rest, so each instantiation compiles against exactly the constants it
// needs (fan is forced to 1 for PRE / GLUT, which never split a list).
//
// DFANN_SCAN_MODES is the table, one row per mode:
//   row(MODE, NAME, SUFFIX, FAM, PRE, GLUT, L16, N4, SQB)
// A row expands to k_scan_<NAME>_<l2|ip><SUFFIX>[_rk][_f]: metric x
// {LDS-buffer selection, _rk register top-k (k <= 16)} x {plain, _f
// filtered: FILT=true, rows tested against a.posbits}. XL2 rows have no
// IP kernels (the precomputed tables are an L2 decomposition). The host
// builds its [mode][ip][rk][filt] kernel table and the ScanMode enum from
// the same list (dfann.hip scan_kernel), so a new scan dimension is one
// row here plus its rule in plan_scan.
//   PRE:  LUT = term2 - 2 * term3 from the precomputed tables
//   GLUT: LUT staged from HBM (built by k_pq_lut) instead of computed in
//         the scan prologue; L16: those rows are __half (pq_lut_f16)
//   N4:   4-bit PQ (nbits=4), in-kernel fp32 LUT only
//   SQB:  bits per dimension of an integer SQ row (FAM 2): 8, or the
//         packed 6 / 4; 8 on every other row, unread
// _rg[_f]: range mode (RANGE=true). One kernel serves the
// count and the fill pass (a.range_fill); it has the register path's row
// loop (REGSEL=true) but no top-k state and no LDS beyond the fam region.
// ---------------------------------------------------------------------------
struct ScanArgs {
  const float *q, *cent, *cb, *sq_vmin, *sq_scale;
  const int *probes;
  const float *keys;
  const uint8_t *const *codes;
  const int64_t *off;
  int nlist;  // probes outside [0, nlist) are empty slots
  int nq, nprobe, d, m, dsub, k, stride, rlog;
  float *cand_d;
  unsigned *cand_p;
  int fam_floats;
  const float *term2, *term3, *qn;  // PRE
  int fan;                          // base modes (not PRE / GLUT)
  const float *glut;                // GLUT
  const unsigned *posbits;          // _f
  // _rg (range mode)
  float radius;
  int range_fill;             // 0 = count pass, 1 = fill pass
  int *range_cnt;             // (nq, nprobe, W) hits per wave, W = block / 64
  const long long *range_off; // exclusive scan of range_cnt inside a query
  const int64_t *range_lims;  // (nq + 1) first output slot per query
  const int64_t *cr_ids;
  float *range_D;
  int64_t *range_I;
  int *range_err;
};

template <int FAM, bool IS_IP, bool REGSEL, bool PRE, bool GLUT, bool L16,
          bool N4, bool FILT, bool RANGE, int SQB>
__device__ __forceinline__ void scan_entry(const ScanArgs &a) {
  ivf_scan_body<FAM, IS_IP, REGSEL, PRE, GLUT, L16, N4, FILT, RANGE, SQB>(
      a.q, a.cent, a.cb, a.sq_vmin, a.sq_scale, a.probes, a.keys, a.codes,
      a.off, a.nlist, a.nq, a.nprobe, a.d, a.m, a.dsub, a.k, a.stride, a.rlog,
      a.cand_d, a.cand_p, a.fam_floats, PRE ? a.term2 : nullptr,
      PRE ? a.term3 : nullptr, PRE ? a.qn : nullptr,
      (PRE || GLUT || RANGE) ? 1 : a.fan, GLUT ? a.glut : nullptr,
      FILT ? a.posbits : nullptr, RANGE ? a.radius : 0.f,
      RANGE ? a.range_fill : 0, RANGE ? a.range_cnt : nullptr,
      RANGE ? a.range_off : nullptr, RANGE ? a.range_lims : nullptr,
      RANGE ? a.cr_ids : nullptr, RANGE ? a.range_D : nullptr,
      RANGE ? a.range_I : nullptr, RANGE ? a.range_err : nullptr);
}

//  (MODE, NAME, SUFFIX, FAM, PRE, GLUT, L16, N4, SQB)
#define DFANN_SCAN_MODES(X, XL2)                                               \
  X(PQ, pq, , 0, false, false, false, false, 8)      /* PQ8 in-kernel LUT */   \
  XL2(PQ_PRE, pq, _pre, 0, true, false, false, false, 8) /* PQ8 precomputed */ \
  X(PQ_G, pq, _g, 0, false, true, false, false, 8)   /* PQ8 GLUT f32 */        \
  X(PQ_GH, pq, _gh, 0, false, true, true, false, 8)  /* PQ8 GLUT f16 */        \
  X(PQ4, pq4, , 0, false, false, false, true, 8)     /* 4-bit PQ */            \
  X(IVFFLAT, ivfflat, , 1, false, false, false, false, 8)                      \
  X(SQ8, sq8, , 2, false, false, false, false, 8)                              \
  X(SQ6, sq6, , 2, false, false, false, false, 6)    /* packed 6-bit SQ */     \
  X(SQ4, sq4, , 2, false, false, false, false, 4)    /* packed 4-bit SQ */     \
  X(SQF, sqf, , 3, false, false, false, false, 8)    /* SQ fp16 */

#define DFANN_SCAN_KERNEL(KNAME, FAM, IS_IP, REGSEL, PRE, GLUT, L16, N4, FILT, \
                          RANGE, SQB)                                          \
  extern "C" __global__ __launch_bounds__(512) void KNAME(ScanArgs a) {        \
    scan_entry<FAM, IS_IP, REGSEL, PRE, GLUT, L16, N4, FILT, RANGE, SQB>(a);   \
  }
#define DFANN_SCAN_METRIC(NAME, MET, SUFFIX, FAM, IS_IP, PRE, GLUT, L16, N4,   \
                          SQB)                                                 \
  DFANN_SCAN_KERNEL(k_scan_##NAME##_##MET##SUFFIX, FAM, IS_IP, false, PRE,     \
                    GLUT, L16, N4, false, false, SQB)                          \
  DFANN_SCAN_KERNEL(k_scan_##NAME##_##MET##SUFFIX##_f, FAM, IS_IP, false, PRE, \
                    GLUT, L16, N4, true, false, SQB)                           \
  DFANN_SCAN_KERNEL(k_scan_##NAME##_##MET##SUFFIX##_rk, FAM, IS_IP, true, PRE, \
                    GLUT, L16, N4, false, false, SQB)                          \
  DFANN_SCAN_KERNEL(k_scan_##NAME##_##MET##SUFFIX##_rk_f, FAM, IS_IP, true,    \
                    PRE, GLUT, L16, N4, true, false, SQB)                      \
  DFANN_SCAN_KERNEL(k_scan_##NAME##_##MET##SUFFIX##_rg, FAM, IS_IP, true, PRE, \
                    GLUT, L16, N4, false, true, SQB)                           \
  DFANN_SCAN_KERNEL(k_scan_##NAME##_##MET##SUFFIX##_rg_f, FAM, IS_IP, true,    \
                    PRE, GLUT, L16, N4, true, true, SQB)
#define DFANN_SCAN_DEF_L2(MODE, NAME, SUFFIX, FAM, PRE, GLUT, L16, N4, SQB)    \
  DFANN_SCAN_METRIC(NAME, l2, SUFFIX, FAM, false, PRE, GLUT, L16, N4, SQB)
#define DFANN_SCAN_DEF(MODE, NAME, SUFFIX, FAM, PRE, GLUT, L16, N4, SQB)       \
  DFANN_SCAN_DEF_L2(MODE, NAME, SUFFIX, FAM, PRE, GLUT, L16, N4, SQB)          \
  DFANN_SCAN_METRIC(NAME, ip, SUFFIX, FAM, true, PRE, GLUT, L16, N4, SQB)
DFANN_SCAN_MODES(DFANN_SCAN_DEF, DFANN_SCAN_DEF_L2)
#undef DFANN_SCAN_DEF
#undef DFANN_SCAN_DEF_L2
#undef DFANN_SCAN_METRIC
#undef DFANN_SCAN_KERNEL

// Range search offsets: fixed-order integer exclusive scans.
// block_excl_scan: out[i] = sum(in[0 .. i-1]) for i < n, returns the total
// to every thread. 256 threads, each owning a contiguous chunk.
template <typename TIn>
__device__ long long block_excl_scan(const TIn *__restrict__ in, long long n,
                                     long long *__restrict__ out) {
  __shared__ long long part[256];
  long long per = (n + 255) / 256;
  long long i0 = min((long long)threadIdx.x * per, n);
  long long i1 = min(i0 + per, n);
  long long sum = 0;
  for (long long i = i0; i < i1; ++i) sum += (long long)in[i];
  part[threadIdx.x] = sum;
  __syncthreads();
  long long before = 0, total = 0;
  for (int t = 0; t < 256; ++t) {
    if (t == (int)threadIdx.x) before = total;
    total += part[t];
  }
  for (long long i = i0; i < i1; ++i) {
    out[i] = before;
    before += (long long)in[i];
  }
  return total;
}

// one block per query: its nprobe * W wave counts -> offsets inside the
// query, and the query's total
__global__ __launch_bounds__(256) void k_range_offsets(
    const int *__restrict__ cnt, int n, long long *__restrict__ off,
    long long *__restrict__ total) {
  long long qb = (long long)blockIdx.x * n;
  long long t = block_excl_scan<int>(cnt + qb, n, off + qb);
  if (threadIdx.x == 0) total[blockIdx.x] = t;
}

// single block: per-query totals -> lims (nq + 1)
__global__ __launch_bounds__(256) void k_range_lims(
    const long long *__restrict__ total, long long nq,
    long long *__restrict__ lims) {
  long long t = block_excl_scan<long long>(total, nq, lims);
  if (threadIdx.x == 0) lims[nq] = t;
}
// ---------------------------------------------------------------------------
// k_pq_lut: ADC lookup tables to HBM, one 256-entry row per (query,
// probe, subspace) at out[(qp)*m*256 + j*256 + c] — the scan's GLUT
// staging then reads its (query, probe) block as one contiguous,
// perfectly-coalesced m-KiB slab. grid = (qp tiles, m subspaces),
// 256 threads = one code c each. The subspace codebook is staged ONCE
// per block in LDS (odd row stride -> conflict-free reads), so the
// codebook leaves L2 ~QPT times less often than the in-kernel build.
// Residual and accumulation are op-for-op the ones the in-kernel build
// uses (sequential t, mul+add, contract off) -> bit-identical LUTs,
// oracle parity preserved (oracle/core.py adc_scan).
// ---------------------------------------------------------------------------
#define PQ_LUT_QPT 64
// DSUB > 0: compile-time subspace width — the thread's codebook row is
// held in REGISTERS across the row loop (the runtime-dsub build left it
// in LDS and re-read it per row: 12-VGPR kernel, ~2.2 ms/step at the
// configs[3] shape). DSUB == 0: runtime fallback.
// PAIRED (f16 only, DSUB>0): each thread computes TWO adjacent codes
// and stores one __half2 — the 2-B per-lane stores of the plain f16
// variant measured 1.7x slower per byte than 4-B stores (1.3 vs
// 2.3 TB/s); half the wave covers row rr, the other half rr+1, so LDS
// and occupancy are unchanged.
template <typename LUTT, int DSUB, bool PAIRED, bool IS_IP>
__device__ __forceinline__ void pq_lut_body(
    const float *__restrict__ q, const float *__restrict__ cent,
    const float *__restrict__ cb, const int *__restrict__ probes, int nlist,
    int nq, int nprobe, int d, int m, int dsub_rt, LUTT *__restrict__ out) {
  const int dsub = DSUB > 0 ? DSUB : dsub_rt;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int pad = dsub | 1;  // odd stride -> gcd(pad, banks) == 1
  float *cb_sm = reinterpret_cast<float *>(smem);  // 256 * pad
  float *r_sm = cb_sm + 256 * pad;                 // PQ_LUT_QPT * pad
  int j = blockIdx.y;
  const float *cbj = cb + (size_t)j * 256 * dsub;
  for (int e = threadIdx.x; e < 256 * dsub; e += blockDim.x)
    cb_sm[(e / dsub) * pad + (e % dsub)] = cbj[e];
  long long qpn = (long long)nq * nprobe;
  long long qp0 = (long long)blockIdx.x * PQ_LUT_QPT;
  long long qp1 = qp0 + PQ_LUT_QPT;
  if (qp1 > qpn) qp1 = qpn;
  int nrow = (int)(qp1 - qp0);
  for (int e = threadIdx.x; e < nrow * dsub; e += blockDim.x) {
    int rr = e / dsub, t = e % dsub;
    long long qp = qp0 + rr;
    int bq = (int)(qp / nprobe);
    float qv = q[(size_t)bq * d + (size_t)j * dsub + t];
    if (IS_IP) {
      r_sm[rr * pad + t] = qv;
    } else {
      // a probe outside [0, nlist) is an empty slot: its table is built
      // from the bare query and the scan never stages it
      int L = probes[qp];
      float cv = 0.f;
      if ((unsigned)L < (unsigned)nlist)
        cv = cent[(size_t)L * d + (size_t)j * dsub + t];
      r_sm[rr * pad + t] = qv - cv;
    }
  }
  __syncthreads();
  if (PAIRED && DSUB > 0) {
    // four adjacent codes per thread = four INDEPENDENT accumulation
    // chains (the 2-chain variant measured 63% issue-stall — the
    // contract-off sequential adds are a 4-cycle VALU dependency chain)
    // and one 8-B store; wave w covers row rr4+w. Per-entry op order
    // unchanged (sequential t) — values identical to the scalar build.
    int w4 = threadIdx.x >> 6;            // wave id: row within rr group
    int c0 = (threadIdx.x & 63) * 4;      // four adjacent codes
    float cr[4][DSUB > 0 ? DSUB : 1];
#pragma unroll
    for (int cc = 0; cc < 4; ++cc)
#pragma unroll
      for (int t = 0; t < DSUB; ++t) cr[cc][t] = cb_sm[(c0 + cc) * pad + t];
    for (int rr4 = 0; rr4 < nrow; rr4 += 4) {
      int rr = rr4 + w4;
      if (rr < nrow) {
        const float *rs = r_sm + rr * pad;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < DSUB; ++t) {
#pragma clang fp contract(off)
#pragma unroll
          for (int cc = 0; cc < 4; ++cc) {
            if (IS_IP) {
              a[cc] = a[cc] + rs[t] * cr[cc][t];
            } else {
              float dd = rs[t] - cr[cc][t];
              a[cc] = a[cc] + dd * dd;
            }
          }
        }
        __half2 lo, hi;
        lo.x = (__half)a[0];  // round-nearest-even, same values as the
        lo.y = (__half)a[1];  // unpaired variant
        hi.x = (__half)a[2];
        hi.y = (__half)a[3];
        uint2 pk;
        pk.x = *reinterpret_cast<unsigned *>(&lo);
        pk.y = *reinterpret_cast<unsigned *>(&hi);
        reinterpret_cast<uint2 *>(out)[((size_t)(qp0 + rr) * m + j) * 64 +
                                       (threadIdx.x & 63)] = pk;
      }
    }
    return;
  }
  int c = threadIdx.x;
  const float *crow = cb_sm + c * pad;
  if (DSUB > 0) {
    // codebook row in registers (fully unrolled: no dynamic indexing);
    // rs[t] reads are wave-broadcast (all lanes the same address).
    // Same op order (sequential t, mul+add, contract off) — bit-exact.
    float creg[DSUB > 0 ? DSUB : 1];
#pragma unroll
    for (int t = 0; t < DSUB; ++t) creg[t] = crow[t];
    for (int rr = 0; rr < nrow; ++rr) {
      const float *rs = r_sm + rr * pad;
      float acc = 0.f;
#pragma unroll
      for (int t = 0; t < DSUB; ++t) {
#pragma clang fp contract(off)
        if (IS_IP) {
          acc = acc + rs[t] * creg[t];
        } else {
          float diff = rs[t] - creg[t];
          acc = acc + diff * diff;
        }
      }
      out[(size_t)(qp0 + rr) * ((size_t)m * 256) + (size_t)j * 256 + c] =
          (LUTT)acc;  // __half: round-nearest-even
    }
  } else {
    for (int rr = 0; rr < nrow; ++rr) {
      const float *rs = r_sm + rr * pad;
      float acc = 0.f;
      for (int t = 0; t < dsub; ++t) {
#pragma clang fp contract(off)
        if (IS_IP) {
          acc = acc + rs[t] * crow[t];
        } else {
          float diff = rs[t] - crow[t];
          acc = acc + diff * diff;
        }
      }
      out[(size_t)(qp0 + rr) * ((size_t)m * 256) + (size_t)j * 256 + c] =
          (LUTT)acc;  // __half: round-nearest-even
    }
  }
}

// IS_IP is a compile-time flag: a runtime test inside the unrolled loops
// gets if-converted, i.e. BOTH metrics computed per entry, then selected.
#define DFANN_PQ_LUT_CASE(LUTT, DS, PAIRED, IP, OUT)                           \
  pq_lut_body<LUTT, DS, PAIRED, IP>(q, cent, cb, probes, nlist, nq, nprobe, d, \
                                    m, dsub, OUT)
#define DFANN_PQ_LUT_DISPATCH(LUTT, PAIRED, IP, OUT)                           \
  switch (dsub) {                                                              \
    case 2: DFANN_PQ_LUT_CASE(LUTT, 2, PAIRED, IP, OUT); break;                \
    case 4: DFANN_PQ_LUT_CASE(LUTT, 4, PAIRED, IP, OUT); break;                \
    case 6: DFANN_PQ_LUT_CASE(LUTT, 6, PAIRED, IP, OUT); break;                \
    case 8: DFANN_PQ_LUT_CASE(LUTT, 8, PAIRED, IP, OUT); break;                \
    case 12: DFANN_PQ_LUT_CASE(LUTT, 12, PAIRED, IP, OUT); break;              \
    case 16: DFANN_PQ_LUT_CASE(LUTT, 16, PAIRED, IP, OUT); break;              \
    default: DFANN_PQ_LUT_CASE(LUTT, 0, false, IP, OUT); break;                \
  }

extern "C" __global__ __launch_bounds__(256) void k_pq_lut(
    const float *q, const float *cent, const float *cb, const int *probes,
    int nlist, int nq, int nprobe, int d, int m, int dsub, int is_ip,
    float *out) {
  if (is_ip) {
    DFANN_PQ_LUT_DISPATCH(float, false, true, out)
  } else {
    DFANN_PQ_LUT_DISPATCH(float, false, false, out)
  }
}

extern "C" __global__ __launch_bounds__(256) void k_pq_lut_f16(
    const float *q, const float *cent, const float *cb, const int *probes,
    int nlist, int nq, int nprobe, int d, int m, int dsub, int is_ip,
    __half *out) {
  if (is_ip) {
    DFANN_PQ_LUT_DISPATCH(__half, true, true, out)
  } else {
    DFANN_PQ_LUT_DISPATCH(__half, true, false, out)
  }
}
// id-space allow-bitmap -> CSR-position-space bitmap: one thread per
// position p, bit = allow[cr_ids[p]], packed with the 64-lane ballot;
// lane 0 stores the wave's two words. The tail wave masks p >= ntotal to
// 0, and waves wholly past ntotal store nothing, so posbits needs exactly
// 2 * ceil(ntotal / 64) words. The scans then test one bit per row
// instead of reading cr_ids[pos] (8 B next to a 16-B PQ code).
extern "C" __global__ __launch_bounds__(256) void k_filter_id2pos(
    const unsigned *__restrict__ allow, const int64_t *__restrict__ cr_ids,
    long long ntotal, unsigned *__restrict__ posbits) {
  long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool bit = false;
  if (p < ntotal) bit = pos_allowed(allow, cr_ids[p]);
  unsigned long long b = __ballot(bit);
  if ((threadIdx.x & 63) == 0 && p < ntotal) {
    long long w = p >> 6;
    posbits[2 * w] = (unsigned)b;
    posbits[2 * w + 1] = (unsigned)(b >> 32);
  }
}

// ---------------------------------------------------------------------------
// merge scan candidates -> final (D, I) per query.
// cand entries: (minimize-key, pos); pos PAD_POS = skip.
// ids: CSR ids array (pos -> arrival id); tie-break on arrival id.
// If ids == nullptr, pos IS the id (flat chunk winners).
// Output: faiss conventions (IP distances un-negated, pads).
// ---------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(256) void k_merge_cand(
    const float *__restrict__ cand_d, const unsigned *__restrict__ cand_p,
    long long nq, int C, int k, const int64_t *__restrict__ ids, int is_ip,
    float *__restrict__ D, int64_t *__restrict__ I) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Sel s = sel_carve(smem);
  long long qi = blockIdx.x;
  if (qi >= nq) return;
  sel_init(s);
  __syncthreads();
  const float *cd = cand_d + qi * C;
  const unsigned *cp = cand_p + qi * C;
  const int BSm = blockDim.x;
  for (int c0 = 0; c0 < C; c0 += 2 * BSm) {
    sel_guard(s, k, 2 * BSm);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      int c = c0 + u * BSm + threadIdx.x;
      if (c < C) {
        unsigned pos = cp[c];
        if (pos != PAD_POS) {
          unsigned idu = ids ? (unsigned)ids[pos] : pos;
          sel_try(s, cd[c], idu);
        }
      }
    }
  }
  __syncthreads();
  sel_compact(s, k);
  int cnt = *s.cnt;
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    bool v = j < cnt;
    if (v) {
      D[qi * k + j] = is_ip ? -s.d[j] : s.d[j];
      I[qi * k + j] = (long long)s.p[j];
    } else {
      D[qi * k + j] = is_ip ? -DFANN_FLT_MAX : DFANN_FLT_MAX;
      I[qi * k + j] = -1;
    }
  }
}

// ---------------------------------------------------------------------------
// shard-result merge (client-side heap semantics, ref client.py:265-310):
// inputs (S, nq, k) faiss-convention D + ids; maximize negates on the way
// in and the OUTPUT KEEPS the negation (reference quirk 2). Output ids =
// slot s*nq*k + q*k + j (caller maps to shard metadata). Every input slot
// is a candidate (pads carry FLT_MAX and can win, as in the reference).
// Tie-break: ascending slot (= shard order, then rank).
// ---------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(256) void k_merge_shards(
    const float *__restrict__ Dall, long long nq, int S, int k, int maximize,
    float *__restrict__ Dout, int64_t *__restrict__ Iout) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Sel s = sel_carve(smem);
  long long qi = blockIdx.x;
  if (qi >= nq) return;
  sel_init(s);
  __syncthreads();
  int C = S * k;
  const int BSm = blockDim.x;
  for (int c0 = 0; c0 < C; c0 += 2 * BSm) {
    sel_guard(s, k, 2 * BSm);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      int c = c0 + u * BSm + threadIdx.x;
      if (c < C) {
        int sh = c / k, j = c % k;
        float v = Dall[((long long)sh * nq + qi) * k + j];
        float key = maximize ? -v : v;
        unsigned slot = (unsigned)(sh * k + j);  // dense per-query slot
        sel_try(s, key, slot);
      }
    }
  }
  __syncthreads();
  sel_compact(s, k);
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    unsigned slot = s.p[j];
    int sh = slot / k, jj = slot % k;
    Dout[qi * k + j] = s.d[j];  // negated for maximize — quirk 2 kept
    Iout[qi * k + j] = ((long long)sh * nq + qi) * k + jj;  // global slot
  }
}

// register-path candidate merge (k <= 16)
extern "C" __global__ __launch_bounds__(256) void k_merge_cand_rk(
    const float *__restrict__ cand_d, const unsigned *__restrict__ cand_p,
    long long nq, int C, int k, const int64_t *__restrict__ ids, int is_ip,
    float *__restrict__ D, int64_t *__restrict__ I) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  long long qi = blockIdx.x;
  if (qi >= nq) return;
  RegTopK<16> loc;
  loc.init();
  const float *cd = cand_d + qi * C;
  const unsigned *cp = cand_p + qi * C;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    unsigned pos = cp[c];
    if (pos != PAD_POS) {
      unsigned idu = ids ? (unsigned)ids[pos] : pos;
      loc.push(cd[c], idu);
    }
  }
  __syncthreads();
  float *od = reinterpret_cast<float *>(smem + REGSEL_LDS_BYTES);
  unsigned *op = reinterpret_cast<unsigned *>(smem + REGSEL_LDS_BYTES + 16 * 4);
  regtopk_block_extract<16>(loc, k, smem, od, op);
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    bool v = op[j] != PAD_POS;
    if (v) {
      D[qi * k + j] = is_ip ? -od[j] : od[j];
      I[qi * k + j] = (long long)op[j];
    } else {
      D[qi * k + j] = is_ip ? -DFANN_FLT_MAX : DFANN_FLT_MAX;
      I[qi * k + j] = -1;
    }
  }
}

// register-path shard merge (k <= 16)
extern "C" __global__ __launch_bounds__(256) void k_merge_shards_rk(
    const float *__restrict__ Dall, long long nq, int S, int k, int maximize,
    float *__restrict__ Dout, int64_t *__restrict__ Iout) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  long long qi = blockIdx.x;
  if (qi >= nq) return;
  RegTopK<16> loc;
  loc.init();
  int C = S * k;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    int sh = c / k, j = c % k;
    float v = Dall[((long long)sh * nq + qi) * k + j];
    loc.push(maximize ? -v : v, (unsigned)(sh * k + j));
  }
  __syncthreads();
  float *od = reinterpret_cast<float *>(smem + REGSEL_LDS_BYTES);
  unsigned *op = reinterpret_cast<unsigned *>(smem + REGSEL_LDS_BYTES + 16 * 4);
  regtopk_block_extract<16>(loc, k, smem, od, op);
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    unsigned slot = op[j];
    int sh = slot / k, jj = slot % k;
    Dout[qi * k + j] = od[j];
    Iout[qi * k + j] = ((long long)sh * nq + qi) * k + jj;
  }
}

// ---------------------------------------------------------------------------
// one-wave top-k by rank counting (merges of at most 256 candidates).
// The wave holds n candidates, candidate i = s*64 + lane in (key[s],
// pay[s]); whatever lies at i >= n is ignored and ranks as a pad. Every
// occupied candidate is broadcast once (v_readlane, wave-uniform index)
// and each lane counts those that precede its own in sel_less order;
// exact (key, payload) duplicates and pads are ordered by candidate
// index, so the ranks are a permutation of [0, 64*CPL) and the lane
// whose candidate has rank r < k owns output slot r. No LDS, no barrier,
// no dependent shuffle chain. rank[s] >= k: not among the k smallest.
// ---------------------------------------------------------------------------
template <int CPL>
__device__ __forceinline__ void wave_rank_topk(const float (&key)[CPL],
                                               const unsigned (&pay)[CPL],
                                               int n, int (&rank)[CPL]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int s = 0; s < CPL; ++s) rank[s] = 0;
#pragma unroll
  for (int ss = 0; ss < CPL; ++ss) {
    int cnt = n - ss * 64;
    cnt = cnt > 64 ? 64 : cnt;
    for (int l = 0; l < cnt; ++l) {  // wave-uniform trip count
      float bk = __int_as_float(
          __builtin_amdgcn_readlane(__float_as_int(key[ss]), l));
      unsigned bp = (unsigned)__builtin_amdgcn_readlane((int)pay[ss], l);
      int bi = ss * 64 + l;
#pragma unroll
      for (int s = 0; s < CPL; ++s) {
        bool before = sel_less(bk, bp, key[s], pay[s]) ||
                      (bk == key[s] && bp == pay[s] && bi < s * 64 + lane);
        rank[s] += before ? 1 : 0;
      }
    }
  }
  // an unoccupied candidate follows all n occupied ones and the
  // unoccupied ones below it: its rank is its own index
#pragma unroll
  for (int s = 0; s < CPL; ++s)
    if (s * 64 + lane >= n) rank[s] = s * 64 + lane;
}

// k_merge_cand_rk for C <= 64*CPL on one wave. A candidate the register
// path never admits (pos == PAD_POS, or a key that is not sel_less than
// the (FLT_MAX, PAD_POS) sentinel: +inf / NaN) becomes a pad.
template <int CPL>
__device__ __forceinline__ void merge_cand_wave(
    const float *__restrict__ cd, const unsigned *__restrict__ cp, int C,
    int k, const int64_t *__restrict__ ids, int is_ip, float *__restrict__ D,
    int64_t *__restrict__ I) {
  const int lane = threadIdx.x & 63;
  float key[CPL];
  unsigned pay[CPL];
  int rank[CPL];
#pragma unroll
  for (int s = 0; s < CPL; ++s) {
    int c = s * 64 + lane;
    key[s] = DFANN_FLT_MAX;
    pay[s] = PAD_POS;
    if (c < C) {
      unsigned pos = cp[c];
      if (pos != PAD_POS) {
        unsigned idu = ids ? (unsigned)ids[pos] : pos;
        float kd = cd[c];
        if (sel_less(kd, idu, DFANN_FLT_MAX, PAD_POS)) {
          key[s] = kd;
          pay[s] = idu;
        }
      }
    }
  }
  wave_rank_topk<CPL>(key, pay, C, rank);
#pragma unroll
  for (int s = 0; s < CPL; ++s) {
    int r = rank[s];
    if (r < k) {
      if (pay[s] != PAD_POS) {
        D[r] = is_ip ? -key[s] : key[s];
        I[r] = (long long)pay[s];
      } else {
        D[r] = is_ip ? -DFANN_FLT_MAX : DFANN_FLT_MAX;
        I[r] = -1;
      }
    }
  }
}

// wave-per-query candidate merge (k <= 16, C <= 256): blockDim/64 queries
// per block; inputs, id lookup and outputs as k_merge_cand_rk
extern "C" __global__ __launch_bounds__(256) void k_merge_cand_w(
    const float *__restrict__ cand_d, const unsigned *__restrict__ cand_p,
    long long nq, int C, int k, const int64_t *__restrict__ ids, int is_ip,
    float *__restrict__ D, int64_t *__restrict__ I) {
  long long qi = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (qi >= nq) return;
  const float *cd = cand_d + qi * C;
  const unsigned *cp = cand_p + qi * C;
  float *Dq = D + qi * k;
  int64_t *Iq = I + qi * k;
  if (C <= 64) merge_cand_wave<1>(cd, cp, C, k, ids, is_ip, Dq, Iq);
  else if (C <= 128) merge_cand_wave<2>(cd, cp, C, k, ids, is_ip, Dq, Iq);
  else merge_cand_wave<4>(cd, cp, C, k, ids, is_ip, Dq, Iq);
}

// k_merge_shards_rk for S*k <= 64*CPL on one wave: payload = dense slot
// s*k + j (the tie-break), maximize negation kept in the output (quirk 2)
template <int CPL>
__device__ __forceinline__ void merge_shards_wave(
    const float *__restrict__ Dall, long long nq, long long qi, int S, int k,
    int maximize, float *__restrict__ Dout, int64_t *__restrict__ Iout) {
  const int lane = threadIdx.x & 63;
  const int C = S * k;
  float key[CPL];
  unsigned pay[CPL];
  int rank[CPL];
#pragma unroll
  for (int s = 0; s < CPL; ++s) {
    int c = s * 64 + lane;
    key[s] = DFANN_FLT_MAX;
    pay[s] = PAD_POS;
    if (c < C) {
      int sh = c / k, j = c % k;
      float v = Dall[((long long)sh * nq + qi) * k + j];
      float kd = maximize ? -v : v;
      if (sel_less(kd, (unsigned)c, DFANN_FLT_MAX, PAD_POS)) {
        key[s] = kd;
        pay[s] = (unsigned)c;
      }
    }
  }
  wave_rank_topk<CPL>(key, pay, C, rank);
#pragma unroll
  for (int s = 0; s < CPL; ++s) {
    int r = rank[s];
    if (r < k) {
      unsigned slot = pay[s];
      int sh = slot / k, jj = slot % k;
      Dout[qi * k + r] = key[s];
      Iout[qi * k + r] = ((long long)sh * nq + qi) * k + jj;
    }
  }
}

// wave-per-query shard merge (k <= 16, S*k <= 256)
extern "C" __global__ __launch_bounds__(256) void k_merge_shards_w(
    const float *__restrict__ Dall, long long nq, int S, int k, int maximize,
    float *__restrict__ Dout, int64_t *__restrict__ Iout) {
  long long qi = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (qi >= nq) return;
  int C = S * k;
  if (C <= 64) merge_shards_wave<1>(Dall, nq, qi, S, k, maximize, Dout, Iout);
  else if (C <= 128) merge_shards_wave<2>(Dall, nq, qi, S, k, maximize, Dout, Iout);
  else merge_shards_wave<4>(Dall, nq, qi, S, k, maximize, Dout, Iout);
}

// ---------------------------------------------------------------------------
// encode / build kernels
// ---------------------------------------------------------------------------

// lowest row whose assignment is still k_assign_init's -1 (no key of the
// row was < FLT_MAX: a NaN row, or products that overflowed). *first is
// all ones before launch and stays so when every row has a list. Runs
// before anything indexes by the assignment.
extern "C" __global__ void k_first_unassigned(
    const int *__restrict__ assign, long long n,
    unsigned long long *__restrict__ first) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (long long)gridDim.x * blockDim.x)
    if (assign[i] < 0) atomicMin(first, (unsigned long long)i);
}

// residual: out[i] = x[i] - cent[assign[i]]; the callers have checked that
// every assign[r] is a list (k_first_unassigned, or add_impl's host copy)
extern "C" __global__ void k_residual(const float *__restrict__ x,
                                      const float *__restrict__ cent,
                                      const int *__restrict__ assign,
                                      long long n, int d,
                                      float *__restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = n * d;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    long long r = i / d, t = i % d;
    out[i] = x[i] - cent[(long long)assign[r] * d + t];
  }
}

// write subspace argmin results into the packed code column j (PQ
// encode = per-subspace distance GEMM + k_assign_rowblock + this);
// writes rows [row0, row0+n) of the slab arena
extern "C" __global__ void k_codes_from_best(const int *__restrict__ best,
                                             long long n, int j, int stride,
                                             int rlog, long long row0,
                                             uint8_t *const *__restrict__ codes) {
  long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; p < n; p += (long long)gridDim.x * blockDim.x)
    slab_row_mut(codes, rlog, row0 + p, stride)[j] = (uint8_t)best[p];
}

// 4-bit twin: sub-quantizer j goes to nibble (j & 1) of byte j / 2. The
// per-subspace launches are stream-ordered, so an even j writes the whole
// byte (high nibble 0 — what an odd m leaves in its last byte) and the
// following odd j ORs into it; no two threads of a launch share a byte.
extern "C" __global__ void k_codes_from_best4(const int *__restrict__ best,
                                              long long n, int j, int stride,
                                              int rlog, long long row0,
                                              uint8_t *const *__restrict__ codes) {
  long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; p < n; p += (long long)gridDim.x * blockDim.x) {
    uint8_t *bp = slab_row_mut(codes, rlog, row0 + p, stride) + (j >> 1);
    uint8_t c = (uint8_t)(best[p] & 15);
    *bp = (j & 1) ? (uint8_t)(*bp | (c << 4)) : c;
  }
}

// integer SQ code of one residual component: the 8-bit op sequence with
// Q = 2^bits - 1 in place of 255 (truncation toward zero, then clamp)
__device__ __forceinline__ unsigned sq_code(float v, float vmin, float vdiff,
                                            float Q) {
  float xi = (v - vmin) / vdiff;
  int c = (int)(Q * xi);
  int qi = (int)Q;
  return (unsigned)(c < 0 ? 0 : (c > qi ? qi : c));
}

// SQ encode of residuals. bits: 16 = fp16, 8 = one byte per dimension,
// 4 / 6 = packed little-endian bit stream (faiss Codec4bit / Codec6bit,
// DESIGN.md §6h). The packed forms give each thread a whole byte (4-bit:
// dims 2j, 2j+1) or a whole 3-byte group (6-bit: dims 4g .. 4g+3) of the
// row's STRIDE, so no byte is shared between threads and every bit past
// d * bits, pad bytes included, is written as zero.
extern "C" __global__ void k_sq_encode(const float *__restrict__ resid,
                                       const float *__restrict__ vmin,
                                       const float *__restrict__ vdiff,
                                       long long n, int d, int stride,
                                       int bits, int rlog, long long row0,
                                       uint8_t *const *__restrict__ codes) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (bits == 4 || bits == 6) {
    const int per = bits == 4 ? stride : (stride + 2) / 3;  // units per row
    const int dpu = bits == 4 ? 2 : 4;                      // dims per unit
    const float Q = bits == 4 ? 15.0f : 63.0f;
    long long total = n * per;
    for (; i < total; i += (long long)gridDim.x * blockDim.x) {
      long long r = i / per;
      int j = (int)(i % per);
      const float *rv = resid + r * d;
      unsigned word = 0;
      for (int e = 0; e < dpu; ++e) {
        int t = j * dpu + e;
        if (t < d)
          word |= sq_code(rv[t], vmin[t], vdiff[t], Q) << (e * bits);
      }
      uint8_t *row = slab_row_mut(codes, rlog, row0 + r, stride);
      if (bits == 4) {
        row[j] = (uint8_t)word;
      } else {
        for (int b = 0; b < 3; ++b)
          if (3 * j + b < stride) row[3 * j + b] = (uint8_t)(word >> (8 * b));
      }
    }
    return;
  }
  const int is_fp16 = bits == 16;
  long long total = n * d;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    long long r = i / d;
    int t = (int)(i % d);
    float v = resid[i];
    uint8_t *row = slab_row_mut(codes, rlog, row0 + r, stride);
    if (is_fp16) {
      __half h = __float2half(v);
      reinterpret_cast<unsigned short *>(row)[t] = __half_as_ushort(h);
    } else {
      float xi = (v - vmin[t]) / vdiff[t];
      int c = (int)(255.0f * xi);  // trunc toward zero, as the oracle
      c = c < 0 ? 0 : (c > 255 ? 255 : c);
      row[t] = (uint8_t)c;
    }
  }
}

// PQ-L2 precomputed tables (faiss IndexIVFPQ use_precomputed_table
// restated): dist(q, code | L) = [qn + coarse_key(q,L)] + sum_j LUT[j][k]
// with LUT[j][k] = term2[L][j][k] - 2*term3[q][j][k],
// term2 = ||cb_jk||^2 + 2 c_{L,j}.cb_jk   (per index, nlist*m*256 fp32),
// term3 = q_j . cb_jk                     (per query batch).
// Cuts the scan block's LUT-build traffic from the full m*256*dsub
// codebook (786 KB at m=64,d=768) to 2 table rows (128 KB).
extern "C" __global__ void k_pq_term2(const float *__restrict__ cent,
                                      const float *__restrict__ cb, int nlist,
                                      int m, int dsub,
                                      float *__restrict__ term2) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = (long long)nlist * m * 256;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    int k = (int)(i & 255);
    int j = (int)((i >> 8) % m);
    long long L = i / (256LL * m);
    const float *cbe = cb + ((size_t)j * 256 + k) * dsub;
    const float *cj = cent + L * (size_t)m * dsub + (size_t)j * dsub;
    float nrm = 0.f, dot = 0.f;
    for (int t = 0; t < dsub; ++t) {
      nrm += cbe[t] * cbe[t];
      dot += cj[t] * cbe[t];
    }
    term2[i] = nrm + 2.0f * dot;
  }
}

extern "C" __global__ void k_pq_term3(const float *__restrict__ q,
                                      const float *__restrict__ cb,
                                      long long nq, int m, int dsub,
                                      float *__restrict__ term3) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = nq * m * 256;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    int k = (int)(i & 255);
    int j = (int)((i >> 8) % m);
    long long qi = i / (256LL * m);
    const float *cbe = cb + ((size_t)j * 256 + k) * dsub;
    const float *qs = q + qi * (size_t)m * dsub + (size_t)j * dsub;
    float dot = 0.f;
    for (int t = 0; t < dsub; ++t) dot += qs[t] * cbe[t];
    term3[i] = dot;
  }
}

// pack raw fp32 rows into the pending byte arena (IVF-Flat codes)
extern "C" __global__ void k_pack_rows(const float *__restrict__ x, long long n,
                                       int d, int stride, int rlog,
                                       long long row0,
                                       uint8_t *const *__restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = n * d;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    long long r = i / d;
    int t = (int)(i % d);
    reinterpret_cast<float *>(slab_row_mut(out, rlog, row0 + r, stride))[t] =
        x[i];
  }
}

// two-source CSR rebuild gather (DESIGN.md §2 memory plan): new CSR row j
// of list l is either an OLD CSR row (same list order) or a PENDING row
// (arrival order within the list, via the psrc permutation). Both source
// arenas and the destination are slab-based; the host launches one call
// per new slab in ascending pos order and frees consumed old slabs
// behind the window. ids: old rows keep their ids; pending row p gets
// id_base + p (ids ARE arrival positions). id2pos rewritten for all.
extern "C" __global__ void k_rebuild_gather(
    long long j0, long long j1, const int64_t *__restrict__ new_off,
    const int64_t *__restrict__ old_off, const int64_t *__restrict__ pend_off,
    const unsigned *__restrict__ psrc,
    const uint8_t *const *__restrict__ old_slabs,
    const uint8_t *const *__restrict__ pend_slabs,
    uint8_t *const *__restrict__ new_slabs,
    const int64_t *__restrict__ old_ids, long long id_base,
    int64_t *__restrict__ new_ids, unsigned *__restrict__ id2pos, int nlist,
    int rlog, int stride) {
  long long j = j0 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= j1) return;
  // binary search: largest l with new_off[l] <= j
  int lo = 0, hi = nlist;
  while (lo + 1 < hi) {
    int mid = (lo + hi) >> 1;
    if (new_off[mid] <= j) lo = mid;
    else hi = mid;
  }
  long long r = j - new_off[lo];
  long long old_len = old_off[lo + 1] - old_off[lo];
  const uint8_t *sp;
  long long id;
  if (r < old_len) {
    long long src = old_off[lo] + r;
    sp = slab_row(old_slabs, rlog, src, stride);
    id = old_ids[src];
  } else {
    long long pi = pend_off[lo] + (r - old_len);
    unsigned ps = psrc[pi];
    sp = slab_row(pend_slabs, rlog, (long long)ps, stride);
    id = id_base + (long long)ps;
  }
  uint8_t *dp = slab_row_mut(new_slabs, rlog, j, stride);
  for (int t = 0; t < stride / 16; ++t)
    reinterpret_cast<uint4 *>(dp)[t] = reinterpret_cast<const uint4 *>(sp)[t];
  new_ids[j] = id;
  id2pos[id] = (unsigned)j;
}

// ---------------------------------------------------------------------------
// removal: one global stable stream compaction over CSR
// positions. keep bits -> int64 prefix over the 64-position words -> every
// kept row moves to newpos(p) = prefix[p >> 6] + popc(word & lanes below).
// No per-list work, no atomics: the same input gives the same bytes.
// ---------------------------------------------------------------------------

// k_filter_id2pos with the sense inverted: keep[p] = !remove[cr_ids[p]],
// one 64-bit ballot word per wave plus its popcount (the scan's input). The
// tail wave masks p >= rows to 0; keepw and cnt hold ceil(rows / 64) entries.
extern "C" __global__ __launch_bounds__(256) void k_remove_keep(
    const unsigned *__restrict__ remove, const int64_t *__restrict__ cr_ids,
    long long rows, unsigned long long *__restrict__ keepw,
    int *__restrict__ cnt) {
  long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool bit = false;
  if (p < rows) bit = !pos_allowed(remove, cr_ids[p]);
  unsigned long long b = __ballot(bit);
  if ((threadIdx.x & 63) == 0 && p < rows) {
    keepw[p >> 6] = b;
    cnt[p >> 6] = __popcll(b);
  }
}

// single block: word popcounts -> exclusive int64 prefix, prefix[words] =
// rows kept (fixed order, the range path's scan)
__global__ __launch_bounds__(256) void k_remove_scan(
    const int *__restrict__ cnt, long long words,
    long long *__restrict__ prefix) {
  long long t = block_excl_scan<int>(cnt, words, prefix);
  if (threadIdx.x == 0) prefix[words] = t;
}

// kept rows in front of position p (p == rows included: the total)
__device__ __forceinline__ long long remove_newpos(
    const unsigned long long *__restrict__ keepw,
    const long long *__restrict__ prefix, long long words, long long p) {
  long long w = p >> 6;
  if (w >= words) return prefix[words];
  unsigned long long below = keepw[w] & ((1ULL << (p & 63)) - 1ULL);
  return prefix[w] + __popcll(below);
}

// list offsets after a global stable compaction: off[l] = newpos(off[l]),
// empty lists and l == nlist included (in place, one thread per entry)
extern "C" __global__ void k_remove_off(
    const unsigned long long *__restrict__ keepw,
    const long long *__restrict__ prefix, long long words,
    int64_t *__restrict__ off, int nlist) {
  int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l > nlist) return;
  off[l] = remove_newpos(keepw, prefix, words, off[l]);
}

// Old positions [p0, p1) -> the new arena. `lanes` threads share a row, each
// copying every lanes-th 16-byte unit of its stride (lanes = stride / 16: one
// unit per thread, loads and stores of neighbouring lanes adjacent; lanes =
// 1: one thread per row as in k_rebuild_gather). The row's first thread also
// writes new_ids[newpos] and id2pos[id] (PAD_POS for a removed row).
extern "C" __global__ __launch_bounds__(256) void k_remove_compact(
    long long p0, long long p1, int lanes,
    const unsigned long long *__restrict__ keepw,
    const long long *__restrict__ prefix, long long words,
    const uint8_t *const *__restrict__ old_slabs,
    uint8_t *const *__restrict__ new_slabs,
    const int64_t *__restrict__ old_ids, int64_t *__restrict__ new_ids,
    unsigned *__restrict__ id2pos, int rlog, int stride) {
  unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned r = t / (unsigned)lanes;
  int c0 = (int)(t - r * (unsigned)lanes);
  long long p = p0 + (long long)r;
  if (p >= p1) return;
  bool keep = (keepw[p >> 6] >> (unsigned)(p & 63)) & 1ULL;
  long long np = keep ? remove_newpos(keepw, prefix, words, p) : -1;
  if (c0 == 0) {
    long long id = old_ids[p];
    id2pos[id] = keep ? (unsigned)np : PAD_POS;
    if (keep) new_ids[np] = id;
  }
  if (!keep) return;
  const uint4 *sp =
      reinterpret_cast<const uint4 *>(slab_row(old_slabs, rlog, p, stride));
  uint4 *dp = reinterpret_cast<uint4 *>(slab_row_mut(new_slabs, rlog, np, stride));
  for (int c = c0; c < stride / 16; c += lanes) dp[c] = sp[c];
}

// out = a & b over nbits bits (flat filtered search under tombstones: the
// caller's allow bitmap AND the live bitmap). One thread per 32-bit word; the
// bits of the last word at and past nbits come out 0.
extern "C" __global__ void k_bits_and(const unsigned *__restrict__ a,
                                      const unsigned *__restrict__ b,
                                      long long nbits,
                                      unsigned *__restrict__ out) {
  long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long words = (nbits + 31) >> 5;
  if (w >= words) return;
  unsigned v = a[w] & b[w];
  if (w == words - 1 && (nbits & 31)) v &= (1u << (unsigned)(nbits & 31)) - 1u;
  out[w] = v;
}

// gather rows by index (f32): out[i] = in[idx[i]]
extern "C" __global__ void k_gather_rows(const float *__restrict__ in,
                                         const int64_t *__restrict__ idx,
                                         long long n, int d,
                                         float *__restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = n * d;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    long long r = i / d;
    int t = (int)(i % d);
    out[i] = in[idx[r] * d + t];
  }
}

// strided subsample gather: out[i] = in[(i*n_in)/n_out]  (oracle kmeans)
extern "C" __global__ void k_gather_strided(const float *__restrict__ in,
                                            long long n_in, long long n_out,
                                            int d, float *__restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = n_out * d;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    long long r = i / d;
    int t = (int)(i % d);
    long long sr = (r * n_in) / n_out;
    out[i] = in[sr * d + t];
  }
}

// subspace slice: out[i*dsub + t] = in[i*d + j0 + t]
extern "C" __global__ void k_subspace_slice(const float *__restrict__ in,
                                            long long n, int d, int j0,
                                            int dsub, float *__restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = n * dsub;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    long long r = i / dsub;
    int t = (int)(i % dsub);
    out[i] = in[r * d + j0 + t];
  }
}

// max |x| of the training set, as the bit pattern of a non-negative float
// (monotone as unsigned, so the atomicMax is order-independent). *out = 0
// before launch. Sizes the fixed-point scale of k_centroid_accum.
extern "C" __global__ void k_absmax(const float *__restrict__ x, long long total,
                                    unsigned *__restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned m = 0u;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    unsigned e = __float_as_uint(fabsf(x[i]));
    m = e > m ? e : m;
  }
  if (m) atomicMax(out, m);
}

// k-means accumulation in 64-bit FIXED POINT: x * 2^e rounded to an
// integer, summed with integer atomics. Integer addition is associative,
// so the sums — and with them the trained centroids — are bit-identical
// from run to run whatever order the atomics land in (fp32 atomics were
// not). The host picks e from max|x| and n so that n * max|x| * 2^e <
// 2^62: no overflow, and a resolution of max|x| * n * 2^-62, far below
// one fp32 ulp of any sum.
extern "C" __global__ void k_centroid_accum(const float *__restrict__ x,
                                            const int *__restrict__ assign,
                                            long long n, int d, double scale,
                                            unsigned long long *__restrict__ sums,
                                            int *__restrict__ counts) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = n * d;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    long long r = i / d;
    int t = (int)(i % d);
    // a row no key of which was < FLT_MAX keeps k_assign_init's -1: it
    // joins no cluster, and the host sees sum(counts) != n (kmeans_device)
    int a = assign[r];
    if (a < 0) continue;
    long long v = __double2ll_rn((double)x[i] * scale);
    // two's-complement wrap makes the unsigned add a signed add
    atomicAdd(&sums[(long long)a * d + t], (unsigned long long)v);
    if (t == 0) atomicAdd(&counts[a], 1);
  }
}

extern "C" __global__ void k_centroid_div(float *__restrict__ cent,
                                          const unsigned long long *__restrict__ sums,
                                          const int *__restrict__ counts,
                                          long long kcent, int d,
                                          double inv_scale) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = kcent * d;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    long long c = i / d;
    if (counts[c] > 0)
      cent[i] = (float)((double)(long long)sums[i] * inv_scale /
                        (double)counts[c]);
  }
}

// per-dim min/max via monotone uint encoding (order-independent)
__device__ __forceinline__ unsigned f32_enc(float f) {
  unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f32_dec(unsigned u) {
  unsigned v = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
  return __uint_as_float(v);
}

extern "C" __global__ void k_minmax_init(unsigned *mn, unsigned *mx, int d) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < d) {
    mn[t] = 0xFFFFFFFFu;
    mx[t] = 0u;
  }
}

extern "C" __global__ void k_minmax_dims(const float *__restrict__ x, long long n,
                                         int d, unsigned *__restrict__ mn,
                                         unsigned *__restrict__ mx) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = n * d;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    int t = (int)(i % d);
    unsigned e = f32_enc(x[i]);
    atomicMin(&mn[t], e);
    atomicMax(&mx[t], e);
  }
}

extern "C" __global__ void k_minmax_decode(const unsigned *mn, const unsigned *mx,
                                           int d, float *vmin, float *vdiff,
                                           float *scale, float Q) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < d) {
    float lo = f32_dec(mn[t]), hi = f32_dec(mx[t]);
    float df = hi - lo;
    if (df == 0.f) df = 1.0f;  // degenerate dim guard (oracle parity)
    vmin[t] = lo;
    vdiff[t] = df;
    scale[t] = df / Q;  // Q = 2^bits - 1: 255, 63 or 15
  }
}

// ---------------------------------------------------------------------------
// reconstruction: decode result ids -> vectors. One block per (q, j).
// type: 0 flat/ivfflat raw (flat_src != null uses flat arena directly by id,
// else CSR codes row), 2 pq, 3 sq8, 4 sqfp16, 5 hnsw sq8, 6 pq nbits=4,
// 7 sq4, 8 sq6 (packed bit streams)
// ---------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(64) void k_reconstruct(
    const int64_t *__restrict__ I, long long nq, int k, int type, int d,
    int m, int dsub, int stride, int rlog, const float *__restrict__ flat_src,
    const uint8_t *const *__restrict__ codes,
    const unsigned *__restrict__ id2pos,
    const int64_t *__restrict__ off, int nlist,
    const float *__restrict__ cent, const float *__restrict__ cb,
    const float *__restrict__ vmin, const float *__restrict__ scale,
    float *__restrict__ R) {
  long long e = blockIdx.x;
  if (e >= nq * k) return;
  long long id = I[e];
  float *out = R + e * d;
  if (id < 0) {
    for (int t = threadIdx.x; t < d; t += blockDim.x) out[t] = 0.f;
    return;
  }
  if (flat_src) {
    const float *src = flat_src + id * d;
    for (int t = threadIdx.x; t < d; t += blockDim.x) out[t] = src[t];
    return;
  }
  if (type == 5) {  // hnsw: non-residual SQ8, codes indexed by id
    const uint8_t *cp5 = slab_row(codes, rlog, id, stride);
    for (int t = threadIdx.x; t < d; t += blockDim.x)
      out[t] = vmin[t] + ((float)cp5[t] + 0.5f) * scale[t];
    return;
  }
  unsigned pos = id2pos[id];
  // binary search list containing pos
  int lo = 0, hi = nlist;
  while (lo + 1 < hi) {
    int mid = (lo + hi) >> 1;
    if (off[mid] <= (long long)pos) lo = mid;
    else hi = mid;
  }
  int L = lo;
  const uint8_t *cp = slab_row(codes, rlog, (long long)pos, stride);
  if (type == 0) {  // ivfflat raw
    const float *src = reinterpret_cast<const float *>(cp);
    for (int t = threadIdx.x; t < d; t += blockDim.x) out[t] = src[t];
  } else if (type == 2) {  // pq: centroid + codebook
    for (int t = threadIdx.x; t < d; t += blockDim.x) {
      int j = t / dsub, tt = t % dsub;
      unsigned c = cp[j];
      out[t] = cent[(long long)L * d + t] + cb[((size_t)j * 256 + c) * dsub + tt];
    }
  } else if (type == 6) {  // 4-bit pq: (m, 16, dsub) codebook, nibble codes
    for (int t = threadIdx.x; t < d; t += blockDim.x) {
      int j = t / dsub, tt = t % dsub;
      unsigned c = (cp[j >> 1] >> ((j & 1) * 4)) & 15u;
      out[t] = cent[(long long)L * d + t] + cb[((size_t)j * 16 + c) * dsub + tt];
    }
  } else if (type == 3) {  // sq8
    for (int t = threadIdx.x; t < d; t += blockDim.x) {
      unsigned c = cp[t];
      out[t] = cent[(long long)L * d + t] + (vmin[t] + ((float)c + 0.5f) * scale[t]);
    }
  } else if (type == 7) {  // sq4: dim t in nibble t & 1 of byte t / 2
    // (7 and 8 decode with separate mul and add, so that a reconstruction
    // is bitwise the restated vmin + (c + 0.5) * scale; type 3 keeps the
    // contraction it always had)
    for (int t = threadIdx.x; t < d; t += blockDim.x) {
#pragma clang fp contract(off)
      unsigned c = (cp[t >> 1] >> ((t & 1) * 4)) & 15u;
      out[t] = cent[(long long)L * d + t] + (vmin[t] + ((float)c + 0.5f) * scale[t]);
    }
  } else if (type == 8) {  // sq6: dim t at bit 6 * (t & 3) of 3-byte group t / 4
    for (int t = threadIdx.x; t < d; t += blockDim.x) {
#pragma clang fp contract(off)
      // bytes past the row's last code byte are never read: byte b0 + 1 is
      // needed only when the field crosses into it
      int bit = (t & 3) * 6, b0 = (t >> 2) * 3 + (bit >> 3), sh = bit & 7;
      unsigned w = cp[b0];
      if (sh > 2) w |= (unsigned)cp[b0 + 1] << 8;
      unsigned c = (w >> sh) & 63u;
      out[t] = cent[(long long)L * d + t] + (vmin[t] + ((float)c + 0.5f) * scale[t]);
    }
  } else {  // sqfp16
    const unsigned short *hp = reinterpret_cast<const unsigned short *>(cp);
    for (int t = threadIdx.x; t < d; t += blockDim.x) {
      out[t] = cent[(long long)L * d + t] + __half2float(__ushort_as_half(hp[t]));
    }
  }
}

// ---------------------------------------------------------------------------
// refine stage: exact re-ranking of the base stage's k'
// candidates against the raw store (fp32 or fp16 rows in arrival order,
// row id == arrival id, stride round16(d * sizeof(T)), zero pad bytes).
// ---------------------------------------------------------------------------

// raw-store append, fp16 rows: __float2half is round-to-nearest-even, the
// conversion k_sq_encode uses (fp32 rows are plain copies, no kernel)
extern "C" __global__ void k_refine_store_f16(const float *__restrict__ x,
                                              long long n, int d, int stride,
                                              int rlog, long long row0,
                                              uint8_t *const *__restrict__ store) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = n * d;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    long long r = i / d;
    int t = (int)(i % d);
    uint8_t *row = slab_row_mut(store, rlog, row0 + r, stride);
    reinterpret_cast<unsigned short *>(row)[t] =
        __half_as_ushort(__float2half(x[i]));
  }
}

#define REFINE_KMAX 512   // k' cap (== the engine's k cap)
#define REFINE_SORT_BYTES (REFINE_KMAX * 8)
#define REFINE_UNROLL 8   // 8-element chunks in flight per lane (d <= 1024
                          // per batch; larger d loops over batches)
#define REFINE_LDS_BYTES(d) (REFINE_SORT_BYTES + (((d) + 7) & ~7) * 4)

// one 8-element chunk of a stored row: one 16-B load (fp16), two (fp32)
template <typename T>
__device__ __forceinline__ void refine_load(const uint8_t *__restrict__ row,
                                            int t0, int d, uint4 &a, uint4 &b) {
  if (std::is_same<T, __half>::value) {
    a = *reinterpret_cast<const uint4 *>(row + (size_t)t0 * 2);
  } else {
    a = *reinterpret_cast<const uint4 *>(row + (size_t)t0 * 4);
    // the second half may lie past the row's stride when d - t0 <= 4
    if (t0 + 4 < d)
      b = *reinterpret_cast<const uint4 *>(row + (size_t)t0 * 4 + 16);
  }
}

template <typename T>
__device__ __forceinline__ void refine_widen(const uint4 &a, const uint4 &b,
                                             float *xv) {
  if (std::is_same<T, __half>::value) {
    const unsigned w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      xv[2 * j] = __half2float(__ushort_as_half((unsigned short)(w[j] & 0xFFFFu)));
      xv[2 * j + 1] = __half2float(__ushort_as_half((unsigned short)(w[j] >> 16)));
    }
  } else {
    xv[0] = __uint_as_float(a.x); xv[1] = __uint_as_float(a.y);
    xv[2] = __uint_as_float(a.z); xv[3] = __uint_as_float(a.w);
    xv[4] = __uint_as_float(b.x); xv[5] = __uint_as_float(b.y);
    xv[6] = __uint_as_float(b.z); xv[7] = __uint_as_float(b.w);
  }
}

// part = part + term over t = t0 .. t0+7 with t < d, ascending, no fma
template <int METRIC>
__device__ __forceinline__ float refine_acc(float part, const float *xv,
                                            const float *__restrict__ qs,
                                            int t0, int d) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (t0 + j < d) {
      float qv = qs[t0 + j];
      float term;
      if (METRIC == 0) {
        term = qv * xv[j];
      } else {
        float df = qv - xv[j];
        term = df * df;
      }
      part = part + term;
    }
  }
  return part;
}

// Exact distances of the (nq, kp) base candidates and the top-k of them.
// One 256-thread block per query; 16 lanes per candidate row, 16 rows per
// pass. Lane g of a row owns the 8-element chunks at t0 = 8g, 8g+128, ...
// and sums them in ascending t; the 16 partials meet in an xor butterfly
// (8, 4, 2, 1). That order IS the numeric contract (oracle/refine.py
// restates it op for op). Selection: (key, ascending id) through a
// monotone uint encoding of the minimize key (L2 distance / -dot), packed
// with the id into one u64 and bitonic-sorted in LDS; candidates that are
// -1 (base pads) never enter. METRIC: 0 = IP, 1 = L2.
template <typename T, int METRIC>
__global__ __launch_bounds__(256) void k_refine(
    const float *__restrict__ q, const uint8_t *const *__restrict__ store,
    int rlog, int stride, long long nrows, const int64_t *__restrict__ candI,
    long long nq, int kp, int k, int d, float *__restrict__ D,
    int64_t *__restrict__ I) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long *srt = reinterpret_cast<unsigned long long *>(smem);
  float *qs = reinterpret_cast<float *>(smem + REFINE_SORT_BYTES);
  const long long qi = blockIdx.x;
  if (qi >= nq) return;
  const int d8 = (d + 7) & ~7;
  for (int t = threadIdx.x; t < d8; t += blockDim.x)
    qs[t] = t < d ? q[qi * d + t] : 0.f;
  int P = 16;
  while (P < kp) P <<= 1;  // kp <= REFINE_KMAX
  for (int i = threadIdx.x; i < P; i += blockDim.x) srt[i] = ~0ULL;
  __syncthreads();
  const int g = threadIdx.x & 15, rsub = threadIdx.x >> 4;
  for (int r0 = 0; r0 < kp; r0 += 16) {
    const int r = r0 + rsub;
    const long long id = r < kp ? candI[qi * kp + r] : -1;
    const bool ok = id >= 0 && id < nrows;
    float part = 0.f;
    if (ok) {
      const uint8_t *row = slab_row(store, rlog, id, stride);
      for (int c0 = 8 * g; c0 < d; c0 += 128 * REFINE_UNROLL) {
        uint4 a[REFINE_UNROLL], b[REFINE_UNROLL];
        // all of the lane's loads for this batch are issued first
#pragma unroll
        for (int u = 0; u < REFINE_UNROLL; ++u) {
          a[u] = make_uint4(0u, 0u, 0u, 0u);
          b[u] = make_uint4(0u, 0u, 0u, 0u);
          const int t0 = c0 + 128 * u;
          if (t0 < d) refine_load<T>(row, t0, d, a[u], b[u]);
        }
#pragma unroll
        for (int u = 0; u < REFINE_UNROLL; ++u) {
          const int t0 = c0 + 128 * u;
          if (t0 < d) {
            float xv[8];
            refine_widen<T>(a[u], b[u], xv);
            part = refine_acc<METRIC>(part, xv, qs, t0, d);
          }
        }
      }
    }
    // every lane takes part (rows that are skipped carry 0)
    part = part + __shfl_xor(part, 8, 16);
    part = part + __shfl_xor(part, 4, 16);
    part = part + __shfl_xor(part, 2, 16);
    part = part + __shfl_xor(part, 1, 16);
    // a key the base selectors would not admit either (NaN or +Inf, from a
    // non-finite query) stays out: the slot is a pad, D is never NaN
    const float key = METRIC == 0 ? -part : part;
    if (ok && g == 0 && key < DFANN_FLT_MAX) {
      srt[r] =((unsigned long long)f32_enc(key) << 32) |
               (unsigned long long)(unsigned)id;
    }
  }
  for (int kk = 2; kk <= P; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < P; i += blockDim.x) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long vi = srt[i], vj = srt[ixj];
          const bool asc = (i & kk) == 0;
          if (asc ? vj < vi : vi < vj) {
            srt[i] = vj;
            srt[ixj] = vi;
          }
        }
      }
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    const unsigned long long v = j < P ? srt[j] : ~0ULL;
    if (v != ~0ULL) {
      const float key = f32_dec((unsigned)(v >> 32));
      D[qi * k + j] = METRIC == 0 ? -key : key;
      I[qi * k + j] = (long long)(v & 0xFFFFFFFFULL);
    } else {
      D[qi * k + j] = METRIC == 0 ? -DFANN_FLT_MAX : DFANN_FLT_MAX;
      I[qi * k + j] = -1;
    }
  }
}

// search_reconstruct on a refine index: the STORED rows (fp16 widened,
// fp32 as is), zeros at pads. One 64-thread block per (q, j).
template <typename T>
__global__ __launch_bounds__(64) void k_refine_reconstruct(
    const int64_t *__restrict__ I, long long n_e, int d,
    const uint8_t *const *__restrict__ store, int rlog, int stride,
    long long nrows, float *__restrict__ R) {
  const long long e = blockIdx.x;
  if (e >= n_e) return;
  const long long id = I[e];
  float *out = R + e * d;
  if (id < 0 || id >= nrows) {
    for (int t = threadIdx.x; t < d; t += blockDim.x) out[t] = 0.f;
    return;
  }
  const uint8_t *row = slab_row(store, rlog, id, stride);
  for (int t = threadIdx.x; t < d; t += blockDim.x) {
    if (std::is_same<T, __half>::value)
      out[t] = __half2float(
          __ushort_as_half(reinterpret_cast<const unsigned short *>(row)[t]));
    else
      out[t] = reinterpret_cast<const float *>(row)[t];
  }
}

// ---------------------------------------------------------------------------
// OPQ pre-transform: y = A x, A (d_out x d_in) fp32 row-major.
// ---------------------------------------------------------------------------

// The ONE transform kernel (add, every search entry, dfann_apply_transform,
// the trainer's projection, and with A^T the reconstruct back-rotation).
// Plain fp32 FMA, not MFMA: y[r][o] is a single fmaf chain over j = 0 ..
// d_in-1 in ascending order, so a row's value depends on neither the batch
// shape nor the row's position in it, and a signed-permutation A is exact.
// 64 rows x 64 outputs per block, 4x4 per thread, 16-wide K steps (the zero
// fill of a K tail adds fmaf(0, 0, acc) = acc).
#define TF_T 64
#define TF_K 16
extern "C" __global__ __launch_bounds__(256) void k_transform(
    const float *__restrict__ x, const float *__restrict__ A,
    float *__restrict__ y, long long n, int d_in, int d_out) {
  __shared__ float sX[TF_K][TF_T + 4];
  __shared__ float sA[TF_K][TF_T + 4];
  const long long r0 = (long long)blockIdx.x * TF_T;
  const int o0 = blockIdx.y * TF_T;
  const int tid = threadIdx.x;
  const int tr = (tid >> 4) * 4, tc = (tid & 15) * 4;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int k0 = 0; k0 < d_in; k0 += TF_K) {
    for (int e = tid; e < TF_T * TF_K; e += 256) {
      int r = e >> 4, c = e & 15;  // TF_K == 16
      bool kin = k0 + c < d_in;
      sX[c][r] = (kin && r0 + r < n) ? x[(r0 + r) * d_in + k0 + c] : 0.f;
      sA[c][r] = (kin && o0 + r < d_out)
                     ? A[(long long)(o0 + r) * d_in + k0 + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < TF_K; ++kk) {
      float a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = sX[kk][tr + i];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = sA[kk][tc + j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    long long r = r0 + tr + i;
    if (r >= n) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (o0 + tc + j < d_out) y[r * d_out + o0 + tc + j] = acc[i][j];
  }
}

// ---------------------------------------------------------------------------
// OPQ training (restates faiss OPQMatrix::train; dfann.hip opq_train). All
// of it runs in fp64 with fixed-order reductions: same data + seed give a
// bitwise-identical rotation.
// ---------------------------------------------------------------------------

// fixed-order block reduction of one double per thread (256 threads)
__device__ __forceinline__ double opq_block_sum(double v, double *sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  double r = sh[0];
  __syncthreads();
  return r;
}

// column means of x (n x d), one block per column
extern "C" __global__ __launch_bounds__(256) void k_opq_colmean(
    const float *__restrict__ x, long long n, int d,
    double *__restrict__ mean) {
  __shared__ double sh[256];
  const int c = blockIdx.x;
  double acc = 0.0;
  for (long long r = threadIdx.x; r < n; r += 256) acc += (double)x[r * d + c];
  double s = opq_block_sum(acc, sh);
  if (threadIdx.x == 0) mean[c] = s / (double)n;
}

// centring: x[r][c] -= mean[c]
extern "C" __global__ void k_opq_center(float *__restrict__ x, long long n,
                                        int d,
                                        const double *__restrict__ mean) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = n * d;
  for (; i < total; i += (long long)gridDim.x * blockDim.x)
    x[i] = (float)((double)x[i] - mean[i % d]);
}

// decode gather of one sub-space: yhat[r][j0 + t] = cb[best[r]][t]
extern "C" __global__ void k_opq_decode_sub(const int *__restrict__ best,
                                            const float *__restrict__ cb,
                                            long long n, int d, int j0,
                                            int dsub, int ksub,
                                            float *__restrict__ yhat) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = n * dsub;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    long long r = i / dsub;
    int t = (int)(i % dsub);
    int c = best[r];
    c = c < 0 ? 0 : (c >= ksub ? ksub - 1 : c);
    yhat[r * d + j0 + t] = cb[(long long)c * dsub + t];
  }
}

// C[i][j] = alpha * sum_k A(i,k) B(k,j) + beta * E[i][j]  (R x C, fp64
// accumulation in ascending k), A(i,k) = A[i*sai + k*sak], B(k,j) =
// B[k*sbk + j*sbj]: the strides give the transposed products (Xc^T Yhat,
// X^T X) without a transpose pass; alpha / beta / E are the fused
// Newton-Schulz epilogue X' = 1.5 X - 0.5 X (X^T X). E may be null
// (beta ignored). 32x32 tile, 2x2 per thread.
template <typename TA, typename TB>
__global__ __launch_bounds__(256) void k_opq_dgemm(
    const TA *__restrict__ A, long long sai, long long sak,
    const TB *__restrict__ B, long long sbk, long long sbj, int R, int C,
    long long K, double alpha, double beta, const double *__restrict__ E,
    double *__restrict__ out) {
  __shared__ double sA[16][33];
  __shared__ double sB[16][33];
  const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
  const int tid = threadIdx.x;
  const int ti = (tid >> 4) * 2, tj = (tid & 15) * 2;
  double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;
  for (long long k0 = 0; k0 < K; k0 += 16) {
    for (int e = tid; e < 32 * 16; e += 256) {
      int p = e & 31, k = e >> 5;
      bool kin = k0 + k < K;
      sA[k][p] = (kin && i0 + p < R)
                     ? (double)A[(long long)(i0 + p) * sai + (k0 + k) * sak]
                     : 0.0;
      sB[k][p] = (kin && j0 + p < C)
                     ? (double)B[(k0 + k) * sbk + (long long)(j0 + p) * sbj]
                     : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      double x0 = sA[k][ti], x1 = sA[k][ti + 1];
      double y0 = sB[k][tj], y1 = sB[k][tj + 1];
      a00 = fma(x0, y0, a00);
      a01 = fma(x0, y1, a01);
      a10 = fma(x1, y0, a10);
      a11 = fma(x1, y1, a11);
    }
    __syncthreads();
  }
  const double acc[2][2] = {{a00, a01}, {a10, a11}};
#pragma unroll
  for (int di = 0; di < 2; ++di)
#pragma unroll
    for (int dj = 0; dj < 2; ++dj) {
      int i = i0 + ti + di, j = j0 + tj + dj;
      if (i < R && j < C) {
        double v = alpha * acc[di][dj];
        if (E) v += beta * E[(long long)i * C + j];
        out[(long long)i * C + j] = v;
      }
    }
}

// single block: out[0] = sum x^2 (fixed order)
extern "C" __global__ __launch_bounds__(256) void k_opq_sumsq(
    const double *__restrict__ x, long long total, double *__restrict__ out) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (long long i = threadIdx.x; i < total; i += 256) acc += x[i] * x[i];
  double s = opq_block_sum(acc, sh);
  if (threadIdx.x == 0) out[0] = s;
}

// single block: out[0] = max |G - I| of a C x C matrix (NaN counts as +inf)
extern "C" __global__ __launch_bounds__(256) void k_opq_maxdev(
    const double *__restrict__ G, int C, double *__restrict__ out) {
  __shared__ double sh[256];
  double m = 0.0;
  long long total = (long long)C * C;
  for (long long i = threadIdx.x; i < total; i += 256) {
    double v = fabs(G[i] - ((i / C) == (i % C) ? 1.0 : 0.0));
    if (!(v <= m)) m = (v == v) ? v : 1e300;
  }
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s && sh[threadIdx.x + s] > sh[threadIdx.x])
      sh[threadIdx.x] = sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sh[0];
}

// x = a * x + b * y (y may be null)
extern "C" __global__ void k_opq_axpby(double *__restrict__ x, double a,
                                       const double *__restrict__ y, double b,
                                       long long total) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < total; i += (long long)gridDim.x * blockDim.x)
    x[i] = a * x[i] + (y ? b * y[i] : 0.0);
}

// P (d_in x d_out, fp64, orthonormal columns) -> A = P^T (d_out x d_in)
// and At = P (d_in x d_out), both fp32
extern "C" __global__ void k_opq_store(const double *__restrict__ P, int d_in,
                                       int d_out, float *__restrict__ A,
                                       float *__restrict__ At) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = (long long)d_in * d_out;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    int r = (int)(i / d_out), c = (int)(i % d_out);
    float v = (float)P[i];
    At[i] = v;
    A[(long long)c * d_in + r] = v;
  }
}

// first `cols` columns of a square (d x d) matrix -> (d x cols)
extern "C" __global__ void k_opq_take_cols(const double *__restrict__ Q, int d,
                                           int cols, double *__restrict__ P) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = (long long)d * cols;
  for (; i < total; i += (long long)gridDim.x * blockDim.x)
    P[i] = Q[(i / cols) * d + (i % cols)];
}

// fp32 transpose (set_transform: At from an injected A)
extern "C" __global__ void k_opq_transpose(const float *__restrict__ A,
                                           int rows, int cols,
                                           float *__restrict__ At) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = (long long)rows * cols;
  for (; i < total; i += (long long)gridDim.x * blockDim.x)
    At[(i % cols) * rows + (i / cols)] = A[i];
}
