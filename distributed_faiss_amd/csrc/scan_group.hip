// dfann — list-major ("grouped") scan of fp16 IVF lists (spec "scan_group",
// DESIGN.md §6n). Included by dfann.hip after kernels.hip.
//
// The pair-major scans run one block per (query, probe) pair, so a list
// probed by a hundred queries of the batch is streamed a hundred times. Here
// the (nq, nprobe) probes table is inverted into per-list groups of pairs,
// and one block multiplies a tile of up to GS_TQ pairs of ONE list against
// the list's rows on the matrix cores, with the per-pair top-k fused behind
// the GEMM: the list is read once per GS_TQ pairs instead of once per pair.
//
// Stages (all stream-ordered, no host read of any count):
//   k_grp_zero      clears the per-list counters (a kernel, so that the
//                   search stays capturable into a graph)
//   k_grp_count     pairs per list; a pair whose probe is outside [0, nlist)
//                   or names an empty list enters no group and gets its k pad
//                   candidates here
//   k_grp_tiles     one block: fixed-order integer exclusive scan over nlist
//                   (the k_range_offsets style), first grouped slot of every
//                   list and the tile table (list, first slot, count <= TQ)
//   k_grp_scatter   pair index q * nprobe + slot into its list's span
//   k_grp_operands  A rows in grouped order: fp16(q - c) (L2) or fp16(q)
//                   (IP), ldh = round_up(d, 8) halves, zero pad; and per
//                   slot ||fp16(q - c)||^2 of the rounded values (L2) or the
//                   bias q . c (IP)
//   k_scan_sqf_grp  the scan, below
//
// The launch bound of the scan, ceil(P / TQ) + min(nlist, P) with
// P = nq * nprobe, covers any tile count (sum over lists of ceil(c / TQ) <=
// P / TQ + the lists that have pairs); surplus blocks exit on the device
// count.

#define GS_TQ 64    // pair rows of a tile (MFMA M)
#define GS_TN 128   // list rows of a row tile (MFMA N)
#define GS_K 64     // halves of a K block
// dynamic LDS: [B buffer 0 | B buffer 1 | row norms | A region]
#define GS_B_BYTES (GS_TN * GS_K * 2)         // 16 KB, one B buffer
#define GS_XN_OFF (2 * GS_B_BYTES)            // key tile (32 KB) aliases B
#define GS_A_OFF (GS_XN_OFF + GS_TN * 4)
#define GS_A_BYTES (GS_TQ * GS_K * 2)         // 8 KB, one K block of A
#define GS_A_RES_MAX (96 * 1024)              // resident A up to here
#define GS_META_NTILES 0
#define GS_META_NGRP 1

extern "C" __global__ void k_grp_zero(int *__restrict__ p, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0;
}

extern "C" __global__ __launch_bounds__(256) void k_grp_count(
    const int *__restrict__ probes, const int64_t *__restrict__ off,
    long long P, int nlist, int k, int *__restrict__ cnt,
    float *__restrict__ cand_d, unsigned *__restrict__ cand_p) {
  long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  int L = probes[p];
  if ((unsigned)L < (unsigned)nlist && off[L + 1] > off[L]) {
    atomicAdd(cnt + L, 1);  // integer count: order-free
    return;
  }
  for (int j = 0; j < k; ++j) {
    cand_d[p * k + j] = DFANN_FLT_MAX;
    cand_p[p * k + j] = PAD_POS;
  }
}

// One block. Thread t owns the contiguous lists [t * per, (t + 1) * per): its
// pair and tile totals go to LDS, every thread adds the totals before its
// own in thread order, then it walks its lists again.
extern "C" __global__ __launch_bounds__(256) void k_grp_tiles(
    const int *__restrict__ cnt, int nlist, int *__restrict__ start,
    int4 *__restrict__ tiles, int *__restrict__ meta) {
  __shared__ int part_p[256], part_t[256];
  int per = (nlist + 255) / 256;
  int i0 = min((int)threadIdx.x * per, nlist), i1 = min(i0 + per, nlist);
  int sp = 0, st = 0;
  for (int i = i0; i < i1; ++i) {
    sp += cnt[i];
    st += (cnt[i] + GS_TQ - 1) / GS_TQ;
  }
  part_p[threadIdx.x] = sp;
  part_t[threadIdx.x] = st;
  __syncthreads();
  int bp = 0, bt = 0, tp = 0, tt = 0;
  for (int t = 0; t < 256; ++t) {
    if (t == (int)threadIdx.x) { bp = tp; bt = tt; }
    tp += part_p[t];
    tt += part_t[t];
  }
  for (int i = i0; i < i1; ++i) {
    int c = cnt[i];
    start[i] = bp;
    for (int j = 0; j < c; j += GS_TQ)
      tiles[bt++] = make_int4(i, bp + j, min(GS_TQ, c - j), 0);
    bp += c;
  }
  if (threadIdx.x == 0) {
    meta[GS_META_NTILES] = tt;
    meta[GS_META_NGRP] = tp;
  }
}

// The order of the pairs inside a group follows the atomics and is not
// fixed; no result depends on it (see k_scan_sqf_grp).
extern "C" __global__ __launch_bounds__(256) void k_grp_scatter(
    const int *__restrict__ probes, const int64_t *__restrict__ off,
    long long P, int nlist, const int *__restrict__ start,
    int *__restrict__ cur, int *__restrict__ order) {
  long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  int L = probes[p];
  if ((unsigned)L < (unsigned)nlist && off[L + 1] > off[L])
    order[start[L] + atomicAdd(cur + L, 1)] = (int)p;
}

// One wave per grouped slot. The rounding is k_flat_f16_store's: one fp32
// subtraction, then __float2half; the norm is of the rounded values, lane l
// adding t = l, l + 64, ... then a fixed shuffle tree.
extern "C" __global__ DFANN_NO_PK_F32 __launch_bounds__(256) void
k_grp_operands(const float *__restrict__ q, const float *__restrict__ cent,
               const int *__restrict__ probes, const float *__restrict__ keys,
               const int *__restrict__ order, const int *__restrict__ meta,
               int nprobe, int d, int ldh, int ip,
               unsigned short *__restrict__ A, float *__restrict__ qn) {
  long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= meta[GS_META_NGRP]) return;
  const int lane = threadIdx.x & 63;
  const int p = order[s];
  const float *qp = q + (long long)(p / nprobe) * d;
  const float *cp = cent + (long long)probes[p] * d;
  float acc = 0.f;
  for (int t = lane; t < ldh; t += 64) {
    __half hv = __float2half(0.f);
    if (t < d) hv = __float2half(ip ? qp[t] : qp[t] - cp[t]);
    float v = __half2float(hv);
    acc += v * v;
    A[s * ldh + t] = __half_as_ushort(hv);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if (lane == 0) qn[s] = ip ? -keys[p] : acc;  // IP: the bias q . c
}

// ---------------------------------------------------------------------------
// k_scan_sqf_grp<KP, IS_IP, FILT>: 256 threads, one tile-table entry per
// block — list L, pair slots [first, first + cnt), cnt <= GS_TQ.
//
// The block walks the list in row tiles of GS_TN rows from the list's first
// row on. Per row tile, K blocks of GS_K halves of the list rows (read in
// place through slab_row, so a list may straddle slabs) go global -> LDS by
// 16-byte global_load_lds, double-buffered, with the XOR swizzle of the bf16
// and flat-f16 kernels on the source group and on the fragment read. The A
// tile (cnt x ldh) is staged the same way: when all its K blocks fit in
// GS_A_RES_MAX (ldh <= 768) it is staged once, with the first row tile, and
// stays resident; otherwise its K blocks are double-buffered next to B's and
// re-read from L2 for every row tile. Groups past ldh, pair rows past cnt
// and list rows past the list's end are staged as zeros, so d, the list
// length and the group size are unrestricted.
//
// Four waves as 2 (M) x 2 (N), wave tile 32 x 64 = acc[2][4] on
// v_mfma_f32_16x16x32_f16. L2 needs ||x||^2 of every list row, which the
// index does not store: two threads per row sum the squares of the staged B
// block (v_dot2_f32_f16) while it sits in LDS, once per row per block.
//
// After the K loop the dots go to a 64 x 128 fp32 tile over the B buffers.
// Thread t owns pair row t >> 2 and the 32-column chunk t & 3, turns a dot
// into the key — L2 (qn - 2 dot) + xn, IP -(bias + dot) — and streams it
// into a RegTopK<KP> that lives across all row tiles. A key not below
// FLT_MAX (NaN included) is not admitted, FILT tests the position's allow
// bit first. The four threads of a pair row merge by shuffle and one writes
// k (key, position) entries to the pair's own slot of cand_d / cand_p.
//
// INVARIANT — a pair's result does not depend on the rest of the batch. The
// row-tile partition starts at the list's first row and so depends on the
// list alone; xn of a row depends on the row and its place in that
// partition; an MFMA output row depends on its own A row only; (key,
// position) is a strict total order, so the push order is immaterial. Which
// other pairs share the tile, their number and their order change nothing.
// Keep it so: no reduction across pair rows, no atomics on results.
// ---------------------------------------------------------------------------

// K block kb of the list's row tile at CSR position r0 into dst[GS_TN][GS_K]
__device__ __forceinline__ void gs_stage_b(
    unsigned short *dst, const uint8_t *const *__restrict__ codes, int rlog,
    int stride, long long r0, long long l1, int ldh, int k0, int w, int lane) {
#pragma unroll
  for (int i = 0; i < GS_TN / 32; ++i) {
    int gb = (w * (GS_TN / 32) + i) * 64;  // the wave's first group
    int g = gb + lane;
    int r = g >> 3;
    int c8s = ((g & 7) * 8) ^ ((r & 7) << 3);
    if (r0 + r < l1 && k0 + c8s < ldh)
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int *)(
              slab_row(codes, rlog, r0 + r, stride) + (size_t)(k0 + c8s) * 2),
          (__attribute__((address_space(3))) unsigned int *)(dst +
                                                             (size_t)gb * 8),
          16, 0, 0);
    else
      *reinterpret_cast<uint4 *>(dst + (size_t)g * 8) = uint4{0, 0, 0, 0};
  }
}

// K block kb of the tile's A rows (grouped slots first ..) into dst[GS_TQ][GS_K]
__device__ __forceinline__ void gs_stage_a(unsigned short *dst,
                                           const unsigned short *__restrict__ A,
                                           long long first, int cnt, int ldh,
                                           int k0, int w, int lane) {
#pragma unroll
  for (int i = 0; i < GS_TQ / 32; ++i) {
    int gb = (w * (GS_TQ / 32) + i) * 64;
    int g = gb + lane;
    int r = g >> 3;
    int c8s = ((g & 7) * 8) ^ ((r & 7) << 3);
    if (r < cnt && k0 + c8s < ldh)
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int *)(
              A + (size_t)(first + r) * ldh + k0 + c8s),
          (__attribute__((address_space(3))) unsigned int *)(dst +
                                                             (size_t)gb * 8),
          16, 0, 0);
    else
      *reinterpret_cast<uint4 *>(dst + (size_t)g * 8) = uint4{0, 0, 0, 0};
  }
}

typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;

// squares of one staged B block: thread t adds half (t & 1) of row t >> 1.
// The slot rotation spreads the 16 lanes of a read group over the 16 slots
// of a 256-byte bank row; the swizzle only permutes the groups of a row.
__device__ __forceinline__ float gs_sumsq(const unsigned short *sb, int tid,
                                          float acc) {
  const int r = tid >> 1, hs = tid & 1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int slot = hs * 4 + ((j + (r >> 1)) & 3);
    uint4 v = *reinterpret_cast<const uint4 *>(sb + r * GS_K + slot * 8);
    const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      f16x2 h = __builtin_bit_cast(f16x2, u[e]);
      acc = __builtin_amdgcn_fdot2(h, h, acc, false);
    }
  }
  return acc;
}

__device__ __forceinline__ void gs_mfma(const unsigned short *sa,
                                        const unsigned short *sb,
                                        f32x4 (&acc)[2][4], int wr, int wc,
                                        int li, int ke) {
#pragma unroll
  for (int kk = 0; kk < GS_K; kk += 32) {
    f16x8 a[2];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
      int ra = wr + ti * 16 + li;
      a[ti] = *reinterpret_cast<const f16x8 *>(
          sa + ra * GS_K + ((kk + ke) ^ ((ra & 7) << 3)));
    }
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
      int rb = wc + tj * 16 + li;
      f16x8 b = *reinterpret_cast<const f16x8 *>(
          sb + rb * GS_K + ((kk + ke) ^ ((rb & 7) << 3)));
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
        acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
            a[ti], b, acc[ti][tj], 0, 0, 0);
    }
  }
}

struct GrpScanArgs {
  const int4 *tiles;
  const int *meta, *order;
  const unsigned short *A;
  const float *qn;
  const uint8_t *const *codes;
  const int64_t *off;
  const unsigned *posbits;  // FILT
  int ldh, stride, rlog, k, a_res;
  float *cand_d;
  unsigned *cand_p;
};

template <int KP, bool IS_IP, bool FILT>
__global__ DFANN_NO_PK_F32 __launch_bounds__(256) void k_scan_sqf_grp(
    GrpScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) char gsm[];
  if ((int)blockIdx.x >= a.meta[GS_META_NTILES]) return;
  const int4 te = a.tiles[blockIdx.x];
  const long long first = te.y;
  const int cnt = te.z;
  const long long l0 = a.off[te.x], l1 = a.off[te.x + 1];
  const int ldh = a.ldh, nkb = (ldh + GS_K - 1) / GS_K;
  const bool a_res = a.a_res != 0;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = (w >> 1) * 32, wc = (w & 1) * 64;
  const int li = lane & 15, ke = (lane >> 4) * 8, rrow = (lane >> 4) * 4;
  unsigned short *sb = reinterpret_cast<unsigned short *>(gsm);
  float *xn_s = reinterpret_cast<float *>(gsm + GS_XN_OFF);
  unsigned short *sa = reinterpret_cast<unsigned short *>(gsm + GS_A_OFF);
  float *tile = reinterpret_cast<float *>(gsm);  // [GS_TQ][GS_TN] over B
  // select ownership: pair row srow, 32-column chunk sch (as k_flat_f16)
  const int srow = tid >> 2, sch = tid & 3;
  const int rot = ((tid >> 2) & 3) * 2 + ((tid & 3) >> 1);
  const bool live = srow < cnt;
  const float qn = live ? a.qn[first + srow] : 0.f;
  RegTopK<KP> loc;
  loc.init();

  for (long long r0 = l0; r0 < l1; r0 += GS_TN) {
    f32x4 acc[2][4] = {};
    float xacc = 0.f;
    if (a_res) {
      if (r0 == l0)
        for (int kb = 0; kb < nkb; ++kb)
          gs_stage_a(sa + (size_t)kb * GS_TQ * GS_K, a.A, first, cnt, ldh,
                     kb * GS_K, w, lane);
    } else {
      gs_stage_a(sa, a.A, first, cnt, ldh, 0, w, lane);
    }
    gs_stage_b(sb, a.codes, a.rlog, a.stride, r0, l1, ldh, 0, w, lane);
    __syncthreads();
    int cur = 0;
    for (int kb = 1; kb < nkb; ++kb) {
      // DMA of the next K block in flight during the MFMAs
      if (!a_res)
        gs_stage_a(sa + (cur ^ 1) * GS_TQ * GS_K, a.A, first, cnt, ldh,
                   kb * GS_K, w, lane);
      gs_stage_b(sb + (cur ^ 1) * GS_TN * GS_K, a.codes, a.rlog, a.stride, r0,
                 l1, ldh, kb * GS_K, w, lane);
      const unsigned short *cb = sb + cur * GS_TN * GS_K;
      if (!IS_IP) xacc = gs_sumsq(cb, tid, xacc);
      gs_mfma(sa + (size_t)(a_res ? kb - 1 : cur) * GS_TQ * GS_K, cb, acc, wr,
              wc, li, ke);
      __syncthreads();  // drains the glds queue (vmcnt(0) inside)
      cur ^= 1;
    }
    {
      const unsigned short *cb = sb + cur * GS_TN * GS_K;
      if (!IS_IP) xacc = gs_sumsq(cb, tid, xacc);
      gs_mfma(sa + (size_t)(a_res ? nkb - 1 : cur) * GS_TQ * GS_K, cb, acc, wr,
              wc, li, ke);
    }
    __syncthreads();  // every wave is done with the B buffers
    if (!IS_IP) {
      xacc += __shfl_xor(xacc, 1, 64);
      if ((tid & 1) == 0) xn_s[tid >> 1] = xacc;
    }
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < 4; ++tj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg)
          tile[(wr + ti * 16 + rrow + rg) * GS_TN + wc + tj * 16 + li] =
              acc[ti][tj][rg];
    __syncthreads();
    if (live) {
      const float4 *rp =
          reinterpret_cast<const float4 *>(tile + srow * GS_TN + sch * 32);
      const float4 *xp = reinterpret_cast<const float4 *>(xn_s + sch * 32);
#pragma unroll 2
      for (int j = 0; j < 8; ++j) {
        int s = (j + rot) & 7;
        float4 v = rp[s];
        float4 x = IS_IP ? float4{0.f, 0.f, 0.f, 0.f} : xp[s];
        const float dv[4] = {v.x, v.y, v.z, v.w};
        const float xv[4] = {x.x, x.y, x.z, x.w};
        long long pos = r0 + sch * 32 + s * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float key = IS_IP ? -(qn + dv[e]) : (qn - 2.0f * dv[e]) + xv[e];
          if (pos + e < l1 && key < DFANN_FLT_MAX &&
              (!FILT || pos_allowed(a.posbits, pos + e)))
            loc.push(key, (unsigned)(pos + e));
        }
      }
    }
    __syncthreads();  // tile consumed before the next stage overwrites it
  }

  // merge the pair row's four chunk lists (lanes t ^ 1, then t ^ 2)
#pragma unroll
  for (int x = 1; x <= 2; x <<= 1) {
    float od[KP];
    unsigned op[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) {
      od[i] = __shfl_xor(loc.d[i], x, 64);
      op[i] = __shfl_xor(loc.p[i], x, 64);
    }
#pragma unroll
    for (int i = 0; i < KP; ++i) loc.push(od[i], op[i]);
  }
  if (sch == 0 && live) {
    size_t o = (size_t)a.order[first + srow] * a.k;
#pragma unroll
    for (int i = 0; i < KP; ++i)
      if (i < a.k) {
        a.cand_d[o + i] = loc.d[i];
        a.cand_p[o + i] = loc.p[i];
      }
  }
}
