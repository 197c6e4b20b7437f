// dfann — list-major ("grouped") scan of fp32 IVF-Flat lists (spec
// "scan_group_flat"). Included by dfann.hip after
// scan_group_pq.hip; the grouping stages, the tile table, gs_stage_a and the
// select are scan_group.hip's as they are.
//
// Operand algebra. An ivf_flat row is the raw fp32 vector x. With c the
// list's centroid, a = fp32(q - c) and r = fp32(x - c) (L2: centring keeps
// the cancellation of W - 2 a.r + V small, as the residual indexes get for
// free) or a = q and r = x (IP),
//   L2   D = (W - 2 a.r) + V,  W = sum a_t^2 per pair, V = sum r_t^2 per row;
//   IP   key = -(a.r).
// a.r is a GEMM of the pairs' rows against the list rows, but fp32 has no
// MFMA type on gfx950 and one rounding to fp16 / bf16 would leave the fp32
// tolerance tier. Both sides are therefore split, v = hi + lo + e with
// hi = bf16_rn(v), lo = bf16_rn(v - hi) (the difference is exact in fp32),
// |e| <= 2^-16 |v|, and the dot is three bf16 products accumulated in fp32,
//   a.r ~= sum (ah rh + ah rl + al rh):
// what is dropped, al rl and the two e terms, is below 2^-14 |a_t r_t| a
// product. bf16 has fp32's exponent range, so no operand is scaled. W and V
// are fp32 sums of the unsplit values in a fixed order.

#define GF_KD 32                 // dimensions of a K block (GS_K halves: hi | lo)
#define GF_LDS_MAX (160 * 1024)

typedef __attribute__((ext_vector_type(2))) float gf_f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 gf_bf16x2;

__host__ __device__ __forceinline__ int gf_ld(int d) {
  return (d + GF_KD - 1) & ~(GF_KD - 1);
}

// LDS bytes of k_scan_flat_grp: B buffers, row terms, the A region (resident
// while all K blocks fit in GS_A_RES_MAX, else two), the centroid
__host__ __device__ __forceinline__ size_t gf_lds_bytes(int d) {
  size_t nkb = (size_t)gf_ld(d) / GF_KD;
  bool res = nkb * GS_A_BYTES <= GS_A_RES_MAX;
  return GS_A_OFF + (res ? nkb : 2) * GS_A_BYTES + (size_t)gf_ld(d) * 4;
}

// (v0, v1) -> packed bf16 pairs hi and lo (v_cvt_pk_bf16_f32: nearest even,
// NaN stays NaN)
__device__ __forceinline__ void gf_split2(float v0, float v1, unsigned &hi,
                                          unsigned &lo) {
  hi = __builtin_bit_cast(
      unsigned, __builtin_convertvector(gf_f32x2{v0, v1}, gf_bf16x2));
  float h0 = __uint_as_float(hi << 16);
  float h1 = __uint_as_float(hi & 0xFFFF0000u);
  lo = __builtin_bit_cast(
      unsigned, __builtin_convertvector(gf_f32x2{v0 - h0, v1 - h1}, gf_bf16x2));
}

// One wave per grouped slot. a_t = q_t - c_t (L2, one fp32 subtraction) or
// q_t (IP), split; the row is 2 ld halves, per K block [32 hi | 32 lo], zero
// past d. W (L2) is of the unsplit a_t: lane l adds t = l, l + 64, ... then a
// fixed shuffle tree.
extern "C" __global__ DFANN_NO_PK_F32 __launch_bounds__(256) void
k_grp_operands_flat(const float *__restrict__ q, const float *__restrict__ cent,
                    const int *__restrict__ probes,
                    const int *__restrict__ order, const int *__restrict__ meta,
                    int nprobe, int d, int ld, int ip,
                    unsigned short *__restrict__ A, float *__restrict__ W) {
  long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= meta[GS_META_NGRP]) return;
  const int lane = threadIdx.x & 63;
  const int p = order[s];
  const float *qp = q + (long long)(p / nprobe) * d;
  const float *cp = cent + (long long)probes[p] * d;
  unsigned short *ar = A + (size_t)s * 2 * ld;
  float acc = 0.f;
  for (int t = lane; t < ld; t += 64) {
    float a = 0.f;
    if (t < d) a = ip ? qp[t] : qp[t] - cp[t];
    acc += a * a;
    unsigned hi, lo;
    gf_split2(a, 0.f, hi, lo);
    int o = (t >> 5) * GS_K + (t & 31);
    ar[o] = (unsigned short)hi;
    ar[o + GF_KD] = (unsigned short)lo;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if (lane == 0) W[s] = ip ? 0.f : acc;
}

// ---------------------------------------------------------------------------
// k_scan_flat_grp<KP, IS_IP, FILT>: 256 threads, one tile-table entry per
// block — list L, pair slots [first, first + cnt), cnt <= GS_TQ — GS_TQ pair
// rows x GS_TN list rows, four waves as 2 x 2, acc[2][4], RegTopK<KP> across
// all row tiles: the frame of k_scan_sqf_grp, with the A staging, residency
// rule, key tile and select unchanged.
//
// K block: GF_KD dimensions. In LDS a block is [rows][GS_K halves], the hi
// halves of the 32 dimensions in columns 0-31 and the lo halves in 32-63,
// byte for byte k_scan_sqf_grp's tile: same 16-byte XOR swizzle (group G of
// row r in slot G ^ (r & 7)), 16 KB B buffers (two), 8 KB A blocks, the key
// tile over the B buffers. A rows arrive in that layout from
// k_grp_operands_flat, so gs_stage_a moves them by global_load_lds with
// ldh = 2 ld; A is resident while its ld / 32 blocks fit in GS_A_RES_MAX
// (d <= 384), else double-buffered per row tile.
//
// B staging cannot be a DMA: the rows need arithmetic on the way. Thread t
// owns 8 consecutive dimensions (group t & 3) of rows (t >> 2) + 64 i, i < 2:
// two 16-byte loads a row through slab_row (a 16-byte load that starts below
// d ends inside the row's stride, which is round16(4 d)). It subtracts the
// centroid (L2; in LDS once per block, zero past d), squares the 8 values
// into the row's running V partial, splits them and writes the 8 hi halves
// and the 8 lo halves as two 16-byte LDS stores into slots G and G + 4.
// Dimensions at or past d and rows past the list's end are zeros whatever
// the stored pad holds. The loads of K block kb + 1 are issued before the
// MFMAs of block kb, wait in 16 VGPRs, and are converted and stored to the
// other buffer after them: one barrier a K block.
//
// gf_mfma: per K block and accumulator tile three
// v_mfma_f32_16x16x32_bf16 in the fixed order (A hi, B hi), (A hi, B lo),
// (A lo, B hi); the four fragments of a lane are read once.
//
// V: the four partials of a row (threads 4 r' .. 4 r' + 3) meet in a fixed
// xor tree after the K loop. Key: L2 (W - 2 dot) + V, IP -dot. Admission,
// FILT, the four-thread merge, the output slot: k_scan_sqf_grp's. Plain
// vector stores, no atomics. INVARIANT as there: a pair's result does not
// depend on the rest of the batch (V depends on the list row alone).
// ---------------------------------------------------------------------------

// the thread's two rows of the K block at dimension k0, raw, into registers
__device__ __forceinline__ void gf_load(
    float4 (&nb)[2][2], const uint8_t *const *__restrict__ codes, int rlog,
    int stride, long long r0, long long l1, int d, int k0, int tid) {
  const int t0 = k0 + (tid & 3) * 8;
  const float4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long long pos = r0 + (tid >> 2) + 64 * i;
    // the address is that of the list's last row past its end: never read
    // there, and the slab table is never indexed past the list
    const float *rp = reinterpret_cast<const float *>(
        slab_row(codes, rlog, min(pos, l1 - 1), stride));
    const bool row = pos < l1;
    nb[i][0] = row && t0 < d ? *reinterpret_cast<const float4 *>(rp + t0) : z;
    nb[i][1] =
        row && t0 + 4 < d ? *reinterpret_cast<const float4 *>(rp + t0 + 4) : z;
  }
}

// ... centred, squared into vacc, split, and into the B buffer at
// gs_stage_b's layout
template <bool IS_IP>
__device__ __forceinline__ void gf_put(unsigned short *dst,
                                       const float4 (&nb)[2][2],
                                       const float *cs, float (&vacc)[2],
                                       long long r0, long long l1, int d,
                                       int k0, int tid) {
  const int G = tid & 3, t0 = k0 + G * 8;
  float c[8];
  if (!IS_IP) {
    const float4 c0 = *reinterpret_cast<const float4 *>(cs + t0);
    const float4 c1 = *reinterpret_cast<const float4 *>(cs + t0 + 4);
    c[0] = c0.x; c[1] = c0.y; c[2] = c0.z; c[3] = c0.w;
    c[4] = c1.x; c[5] = c1.y; c[6] = c1.z; c[7] = c1.w;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = (tid >> 2) + 64 * i;
    const bool row = r0 + r < l1;
    float v[8] = {nb[i][0].x, nb[i][0].y, nb[i][0].z, nb[i][0].w,
                  nb[i][1].x, nb[i][1].y, nb[i][1].z, nb[i][1].w};
    float sq = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (!IS_IP) v[e] -= c[e];
      if (!row || t0 + e >= d) v[e] = 0.f;
      if (!IS_IP) sq += v[e] * v[e];
    }
    vacc[i] += sq;
    uint4 hi, lo;
    gf_split2(v[0], v[1], hi.x, lo.x);
    gf_split2(v[2], v[3], hi.y, lo.y);
    gf_split2(v[4], v[5], hi.z, lo.z);
    gf_split2(v[6], v[7], hi.w, lo.w);
    unsigned short *rp = dst + r * GS_K;
    *reinterpret_cast<uint4 *>(rp + ((G ^ (r & 7)) << 3)) = hi;
    *reinterpret_cast<uint4 *>(rp + (((G + 4) ^ (r & 7)) << 3)) = lo;
  }
}

__device__ __forceinline__ void gf_mfma(const unsigned short *sa,
                                        const unsigned short *sb,
                                        f32x4 (&acc)[2][4], int wr, int wc,
                                        int li, int ke) {
  bf16x8 ah[2], al[2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti) {
    int ra = wr + ti * 16 + li, sw = (ra & 7) << 3;
    ah[ti] = *reinterpret_cast<const bf16x8 *>(sa + ra * GS_K + (ke ^ sw));
    al[ti] =
        *reinterpret_cast<const bf16x8 *>(sa + ra * GS_K + ((GF_KD + ke) ^ sw));
  }
#pragma unroll
  for (int tj = 0; tj < 4; ++tj) {
    int rb = wc + tj * 16 + li, sw = (rb & 7) << 3;
    bf16x8 bh = *reinterpret_cast<const bf16x8 *>(sb + rb * GS_K + (ke ^ sw));
    bf16x8 bl =
        *reinterpret_cast<const bf16x8 *>(sb + rb * GS_K + ((GF_KD + ke) ^ sw));
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
      acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[ti], bh,
                                                            acc[ti][tj], 0, 0, 0);
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
      acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[ti], bl,
                                                            acc[ti][tj], 0, 0, 0);
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
      acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[ti], bh,
                                                            acc[ti][tj], 0, 0, 0);
  }
}

struct GrpFlatScanArgs {
  GrpScanArgs g;      // A: split rows; qn: W; ldh: 2 ld
  const float *cent;  // L2
  int d;
};

template <int KP, bool IS_IP, bool FILT>
__global__ DFANN_NO_PK_F32 __launch_bounds__(256) void k_scan_flat_grp(
    GrpFlatScanArgs af) {
  const GrpScanArgs &a = af.g;
  extern __shared__ __attribute__((aligned(16))) char gsm[];
  if ((int)blockIdx.x >= a.meta[GS_META_NTILES]) return;
  const int4 te = a.tiles[blockIdx.x];
  const long long first = te.y;
  const int cnt = te.z;
  const long long l0 = a.off[te.x], l1 = a.off[te.x + 1];
  const int d = af.d, ldh = a.ldh, nkb = ldh / GS_K;
  const bool a_res = a.a_res != 0;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = (w >> 1) * 32, wc = (w & 1) * 64;
  const int li = lane & 15, ke = (lane >> 4) * 8, rrow = (lane >> 4) * 4;
  unsigned short *sb = reinterpret_cast<unsigned short *>(gsm);
  float *xn_s = reinterpret_cast<float *>(gsm + GS_XN_OFF);
  unsigned short *sa = reinterpret_cast<unsigned short *>(gsm + GS_A_OFF);
  float *cs = reinterpret_cast<float *>(
      gsm + GS_A_OFF + (size_t)(a_res ? nkb : 2) * GS_A_BYTES);
  float *tile = reinterpret_cast<float *>(gsm);  // [GS_TQ][GS_TN] over B
  const int srow = tid >> 2, sch = tid & 3;
  const int rot = ((tid >> 2) & 3) * 2 + ((tid & 3) >> 1);
  const bool live = srow < cnt;
  const float qn = live ? a.qn[first + srow] : 0.f;
  RegTopK<KP> loc;
  loc.init();
  if (!IS_IP) {
    const float *cp = af.cent + (long long)te.x * d;
    for (int t = tid; t < ldh / 2; t += 256) cs[t] = t < d ? cp[t] : 0.f;
    __syncthreads();
  }

  for (long long r0 = l0; r0 < l1; r0 += GS_TN) {
    f32x4 acc[2][4] = {};
    float vacc[2] = {0.f, 0.f};
    float4 nb[2][2];  // the next K block's rows, in flight
    if (a_res) {
      if (r0 == l0)
        for (int kb = 0; kb < nkb; ++kb)
          gs_stage_a(sa + (size_t)kb * GS_TQ * GS_K, a.A, first, cnt, ldh,
                     kb * GS_K, w, lane);
    } else {
      gs_stage_a(sa, a.A, first, cnt, ldh, 0, w, lane);
    }
    gf_load(nb, a.codes, a.rlog, a.stride, r0, l1, d, 0, tid);
    gf_put<IS_IP>(sb, nb, cs, vacc, r0, l1, d, 0, tid);
    __syncthreads();  // drains the glds queue (vmcnt(0) inside)
    int cur = 0;
    for (int kb = 1; kb < nkb; ++kb) {
      // A's DMA and the loads of the next K block in flight during the MFMAs
      if (!a_res)
        gs_stage_a(sa + (cur ^ 1) * GS_TQ * GS_K, a.A, first, cnt, ldh,
                   kb * GS_K, w, lane);
      gf_load(nb, a.codes, a.rlog, a.stride, r0, l1, d, kb * GF_KD, tid);
      gf_mfma(sa + (size_t)(a_res ? kb - 1 : cur) * GS_TQ * GS_K,
              sb + cur * GS_TN * GS_K, acc, wr, wc, li, ke);
      gf_put<IS_IP>(sb + (cur ^ 1) * GS_TN * GS_K, nb, cs, vacc, r0, l1, d,
                    kb * GF_KD, tid);
      __syncthreads();
      cur ^= 1;
    }
    gf_mfma(sa + (size_t)(a_res ? nkb - 1 : cur) * GS_TQ * GS_K,
            sb + cur * GS_TN * GS_K, acc, wr, wc, li, ke);
    __syncthreads();  // every wave is done with the B buffers
    if (!IS_IP) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        vacc[i] += __shfl_xor(vacc[i], 1, 64);
        vacc[i] += __shfl_xor(vacc[i], 2, 64);
        if ((tid & 3) == 0) xn_s[(tid >> 2) + 64 * i] = vacc[i];
      }
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
          float key = IS_IP ? -dv[e] : (qn - 2.0f * dv[e]) + xv[e];
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
