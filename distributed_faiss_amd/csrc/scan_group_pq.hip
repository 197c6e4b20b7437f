// dfann — list-major ("grouped") scan of IVFPQ lists with 8-bit codes (spec
// "scan_group_pq"). Included by dfann.hip after
// scan_group_sq8.hip; the grouping stages, the tile table, gs_stage_a,
// gs_mfma, gs_sumsq and the select are scan_group.hip's as they are.
//
// Operand algebra. A stored row decodes to x^ = its m codewords side by side,
// and the row is cent + x^, so with a = q - cent (L2) or q (IP)
//   L2   D = ||a - x^||^2 = W - 2 a.x^ + ||x^||^2,  W = sum a_t^2 per pair;
//   IP   dot = q.c + q.x^.
// a.x^ is a GEMM of the pairs' rows against the DECODED list rows. The B side
// of that GEMM does not exist in memory: it is gathered from an fp16 image of
// the codebooks on its way to LDS, one K block at a time (below). No table of
// m x 256 partial distances is built per pair, which is what the pair-major
// scan spends its LUT stage and its LDS on.
//
// Scaling. Codebook entries of normalised embeddings are far below the fp16
// normal range, so the image carries ONE power of two for the index, 2^ec with
// max |cb| 2^ec in [2^12, 2^13), and every A row carries its own 2^ea with max
// |a_t| 2^ea in [2^14, 2^15): products stay below 2^28 and the roundings are
// relative (2^-11 each). 2^-(ea+ec) multiplies the dot back in fp32, 2^-2ec
// the row's sum of squares. Both exponents are clamped to |e| <= GSP_EMAX so
// that those two factors (and twice the first) stay normal; entries the clamp
// leaves subnormal in fp16 have squares that are zero in fp32 already.

#define GSP_EMAX 62
#define GSP_LDS_MAX (160 * 1024)
#define GSP_CODE_OFF GS_A_OFF  // the row tile's code bytes, then the A region

// bytes of cb16: the halves, then the int ec on a 16-byte boundary
__host__ __device__ __forceinline__ size_t gsp_cb16_ec_off(int d) {
  return ((size_t)d * 256 * 2 + 15) & ~(size_t)15;
}

// LDS bytes of k_scan_pq_grp: B buffers, row terms, GS_TN code rows, A region
// (resident while all K blocks fit in GS_A_RES_MAX, else two)
__host__ __device__ __forceinline__ size_t gsp_lds_bytes(int d, int stride) {
  size_t nkb = ((size_t)d + GS_K - 1) / GS_K;
  bool res = nkb * GS_A_BYTES <= GS_A_RES_MAX;
  return GSP_CODE_OFF + (size_t)GS_TN * stride + (res ? nkb : 2) * GS_A_BYTES;
}

// ec of a largest magnitude, shared by the image and the operand kernel:
// amax 2^e in [2^(top-1), 2^top), 0 for amax == 0
__device__ __forceinline__ int gsp_exp(float amax, int top) {
  if (!(amax > 0.f)) return 0;
  int x;
  frexpf(amax, &x);  // amax in [2^(x-1), 2^x)
  return min(max(top - x, -GSP_EMAX), GSP_EMAX);
}

// One block (the codebooks are a few hundred KB and change with training
// only): largest magnitude and a non-finite flag over all n entries (max and
// or: order-free), ec, then cb16[i] = fp16(cb[i] 2^ec), one rounding each. A
// codebook with a non-finite entry is left unscaled so that NaN propagates.
extern "C" __global__ __launch_bounds__(1024) void k_pq_cb16(
    const float *__restrict__ cb, long long n, unsigned short *__restrict__ cb16,
    int *__restrict__ ec_out) {
  __shared__ float smax[16];
  __shared__ int sbad[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float amax = 0.f;
  bool bad = false;
  for (long long i = tid; i < n; i += 1024) {
    float v = fabsf(cb[i]);
    bad |= !(v <= DFANN_FLT_MAX);  // NaN or inf
    amax = fmaxf(amax, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  const bool wbad = __builtin_amdgcn_ballot_w64(bad) != 0;
  if (lane == 0) {
    smax[w] = amax;
    sbad[w] = wbad;
  }
  __syncthreads();
  bool anybad = false;
  amax = 0.f;
  for (int i = 0; i < 16; ++i) {
    amax = fmaxf(amax, smax[i]);
    anybad |= sbad[i] != 0;
  }
  const int ec = anybad ? 0 : gsp_exp(amax, 13);
  const float up = ldexpf(1.0f, ec);
  for (long long i = tid; i < n; i += 1024)
    cb16[i] = __half_as_ushort(__float2half(cb[i] * up));
  if (tid == 0) *ec_out = ec;
}

// One wave per grouped slot. a_t = q_t - c_t (L2, one fp32 subtraction) or
// q_t (IP), times the row's own 2^ea, one rounding to fp16; ld = round_up(d,
// 8) halves, zero pad. ea = 0 for an all-zero row; a row with a non-finite
// entry is left unscaled so that NaN propagates. inv = 2^-(ea+ec); cst = W of
// the unrounded a_t (L2) or q.c (IP: the coarse key is -(q.c)). Lane l adds
// t = l, l + 64, ... then a fixed shuffle tree.
extern "C" __global__ __launch_bounds__(256) void k_grp_operands_pq(
    const float *__restrict__ q, const float *__restrict__ cent,
    const int *__restrict__ probes, const float *__restrict__ keys,
    const int *__restrict__ order, const int *__restrict__ meta,
    const int *__restrict__ ec_p, int nprobe, int d, int ld, int ip,
    unsigned short *__restrict__ A, float *__restrict__ cst,
    float *__restrict__ inv) {
  long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= meta[GS_META_NGRP]) return;
  const int lane = threadIdx.x & 63;
  const int p = order[s];
  const float *qp = q + (long long)(p / nprobe) * d;
  const float *cp = cent + (long long)probes[p] * d;
  float acc = 0.f, amax = 0.f;
  bool bad = false;
  for (int t = lane; t < d; t += 64) {
    float a = ip ? qp[t] : qp[t] - cp[t];
    acc += a * a;
    bad |= !(fabsf(a) <= DFANN_FLT_MAX);  // NaN or inf
    amax = fmaxf(amax, fabsf(a));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc += __shfl_down(acc, o, 64);
    amax = fmaxf(amax, __shfl_xor(amax, o, 64));  // max: order-free
  }
  const int ea =
      __builtin_amdgcn_ballot_w64(bad) == 0 ? gsp_exp(amax, 15) : 0;
  const float up = ldexpf(1.0f, ea);
  for (int t = lane; t < ld; t += 64) {
    float a = 0.f;
    if (t < d) a = ip ? qp[t] : qp[t] - cp[t];
    A[s * ld + t] = __half_as_ushort(__float2half(a * up));
  }
  if (lane == 0) {
    cst[s] = ip ? -keys[p] : acc;
    inv[s] = ldexpf(1.0f, -(ea + *ec_p));
  }
}

// ---------------------------------------------------------------------------
// k_scan_pq_grp<KP, IS_IP, FILT, V>: 256 threads, one tile-table entry per
// block — list L, pair slots [first, first + cnt), cnt <= GS_TQ — GS_TQ pair
// rows x GS_TN list rows, four waves as 2 x 2, acc[2][4] on
// v_mfma_f32_16x16x32_f16, RegTopK<KP> across all row tiles: the frame of
// k_scan_sqf_grp, with the A staging, residency rule, fragment reads, row
// term and select unchanged. What is new is where a B block comes from.
//
// Row-tile codes. The tile's GS_TN code rows (stride bytes each, read in
// place through slab_row, zero rows past the list's end) go to an LDS region
// of their own once per row tile: stride / 16 groups a row by 16-byte
// global_load_lds, group g of the tile at byte 16 g, i.e. rows back to back.
// Every K block of the tile reads its code bytes from there, so the list is
// still read from memory once per GS_TQ pairs.
//
// B-block decode. A B block is [GS_TN][GS_K halves] = 1024 groups of 8
// halves. Thread t owns group G = t & 7 of rows (t >> 3) + 32 i, i < 4, that
// is columns col0 = k0 + 8 G .. col0 + 7 of four rows: the column arithmetic
// (sub-quantizer j = col / dsub and the offset col % dsub inside it) is done
// once per K block and serves the four rows. V is the largest of 8, 4, 2
// that divides dsub, so a run of V columns that starts at a multiple of V
// lies inside ONE sub-quantizer whatever dsub is, also where a K block or a
// group begins or ends inside one (dsub = 12: j changes at column 12, in the
// middle of group 1). Per run: the row's code byte c of sub-quantizer j from
// LDS, then one 2 V-byte load of cb16[(j 256 + c) dsub + col % dsub ..]; runs
// at or past d are zeros (d is a multiple of V). The 8 / V runs of a group
// are assembled in registers and stored as one 16-byte LDS write at the
// fragment layout of gs_stage_b (group G of row r in slot G ^ (r & 7)), so
// gs_mfma and gs_sumsq read a decoded block as they read a staged one. A
// wave's write covers 1 KB of consecutive LDS.
//
// Pipeline. The gathers of K block kb + 1 are issued before the row term and
// the MFMAs of block kb, sit in 16 VGPRs meanwhile, and are written to the
// other B buffer after them: the codebook round trip (L2 / L1 hits: the image
// is 2 d 256 bytes) lies under the matrix work as the DMA does in
// k_scan_sqf_grp. Block 0 of a row tile is decoded in the open, behind the
// barrier that publishes the tile's codes. Not built: a codebook slice staged
// in LDS per K block (32 KB at GS_K columns) with the gather served from LDS.
//
// Key: L2 (W - 2 2^-(ea+ec) dot) + 2^-2ec xn with xn = sum (2^ec x^_t)^2 of
// the rounded halves (gs_sumsq over the decoded block), IP -(q.c +
// 2^-(ea+ec) dot). Admission, FILT, the four-thread merge, the output slot:
// k_scan_sqf_grp's. Plain vector stores, no atomics. INVARIANT as there: a
// pair's result does not depend on the rest of the batch (2^ea depends on
// the pair's own row, 2^ec on the index, xn on the list row and its place in
// the row-tile partition).
// ---------------------------------------------------------------------------

struct GrpPqScanArgs {
  GrpScanArgs g;  // qn: W or q.c; ldh: round_up(d, 8)
  const float *inv;
  const unsigned short *cb16;
  const int *ec;
  int d, dsub;
};

// the row tile's code rows into sc[GS_TN][stride]
__device__ __forceinline__ void gsp_stage_codes(
    uint8_t *sc, const uint8_t *const *__restrict__ codes, int rlog,
    int stride, long long r0, long long l1, int w, int lane) {
  const int gpr = stride >> 4;  // 16-byte groups of a row
  for (int c = w; c < 2 * gpr; c += 4) {  // GS_TN * gpr / 64 wave chunks
    int g = c * 64 + lane;
    int r = g / gpr, o = (g - r * gpr) << 4;
    if (r0 + r < l1)
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int *)(
              slab_row(codes, rlog, r0 + r, stride) + o),
          (__attribute__((address_space(3))) unsigned int *)(sc +
                                                             (size_t)c * 1024),
          16, 0, 0);
    else
      *reinterpret_cast<uint4 *>(sc + (size_t)g * 16) = uint4{0, 0, 0, 0};
  }
}

// the thread's four groups of the K block at column k0, from the codebook
// image into registers
template <int V>
__device__ __forceinline__ void gsp_gather(
    uint4 (&g)[4], const uint8_t *sc, int stride,
    const unsigned short *__restrict__ cb16, int d, int dsub, int k0,
    int tid) {
  constexpr int NR = 8 / V;  // runs of a group
  const int col0 = k0 + (tid & 7) * 8, rr = tid >> 3;
  int sub[NR], base[NR];  // sub-quantizer; element of its codeword 0
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    int col = col0 + u * V;
    int j = col / dsub;
    sub[u] = col < d ? j : -1;
    base[u] = j * 256 * dsub + (col - j * dsub);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint8_t *cr = sc + (rr + 32 * i) * stride;
    unsigned u32[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int u = 0; u < NR; ++u) {
      if (sub[u] < 0) continue;
      const unsigned short *src = cb16 + base[u] + (int)cr[sub[u]] * dsub;
      if constexpr (V == 8) {
        uint4 v = *reinterpret_cast<const uint4 *>(src);
        u32[0] = v.x; u32[1] = v.y; u32[2] = v.z; u32[3] = v.w;
      } else if constexpr (V == 4) {
        uint2 v = *reinterpret_cast<const uint2 *>(src);
        u32[2 * u] = v.x; u32[2 * u + 1] = v.y;
      } else {
        u32[u] = *reinterpret_cast<const unsigned *>(src);
      }
    }
    g[i] = uint4{u32[0], u32[1], u32[2], u32[3]};
  }
}

// ... and from registers into the B buffer, at gs_stage_b's layout
__device__ __forceinline__ void gsp_put(unsigned short *dst,
                                        const uint4 (&g)[4], int tid) {
  const int G = tid & 7, rr = tid >> 3;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int r = rr + 32 * i;
    *reinterpret_cast<uint4 *>(dst + r * GS_K + ((G ^ (r & 7)) << 3)) = g[i];
  }
}

template <int KP, bool IS_IP, bool FILT, int V>
__global__ __launch_bounds__(256) void k_scan_pq_grp(GrpPqScanArgs ap) {
  const GrpScanArgs &a = ap.g;
  extern __shared__ __attribute__((aligned(16))) char gsm[];
  if ((int)blockIdx.x >= a.meta[GS_META_NTILES]) return;
  const int4 te = a.tiles[blockIdx.x];
  const long long first = te.y;
  const int cnt = te.z;
  const long long l0 = a.off[te.x], l1 = a.off[te.x + 1];
  const int ldh = a.ldh, nkb = (ldh + GS_K - 1) / GS_K;
  const int d = ap.d, dsub = ap.dsub, stride = a.stride;
  const bool a_res = a.a_res != 0;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = (w >> 1) * 32, wc = (w & 1) * 64;
  const int li = lane & 15, ke = (lane >> 4) * 8, rrow = (lane >> 4) * 4;
  unsigned short *sb = reinterpret_cast<unsigned short *>(gsm);
  float *xn_s = reinterpret_cast<float *>(gsm + GS_XN_OFF);
  uint8_t *sc = reinterpret_cast<uint8_t *>(gsm + GSP_CODE_OFF);
  unsigned short *sa = reinterpret_cast<unsigned short *>(
      gsm + GSP_CODE_OFF + (size_t)GS_TN * stride);
  float *tile = reinterpret_cast<float *>(gsm);  // [GS_TQ][GS_TN] over B
  const int srow = tid >> 2, sch = tid & 3;
  const int rot = ((tid >> 2) & 3) * 2 + ((tid & 3) >> 1);
  const bool live = srow < cnt;
  const float cst = live ? a.qn[first + srow] : 0.f;
  // L2 takes 2 * 2^-(ea+ec) (exact), IP 2^-(ea+ec)
  const float inv = live ? (IS_IP ? 1.0f : 2.0f) * ap.inv[first + srow] : 0.f;
  const float xs = ldexpf(1.0f, -2 * *ap.ec);  // 2^-2ec
  RegTopK<KP> loc;
  loc.init();

  for (long long r0 = l0; r0 < l1; r0 += GS_TN) {
    f32x4 acc[2][4] = {};
    float xacc = 0.f;
    uint4 nb[4];  // the next K block's groups, in flight
    if (a_res) {
      if (r0 == l0)
        for (int kb = 0; kb < nkb; ++kb)
          gs_stage_a(sa + (size_t)kb * GS_TQ * GS_K, a.A, first, cnt, ldh,
                     kb * GS_K, w, lane);
    } else {
      gs_stage_a(sa, a.A, first, cnt, ldh, 0, w, lane);
    }
    gsp_stage_codes(sc, a.codes, a.rlog, stride, r0, l1, w, lane);
    __syncthreads();  // the tile's codes are in LDS (vmcnt(0) inside)
    gsp_gather<V>(nb, sc, stride, ap.cb16, d, dsub, 0, tid);
    gsp_put(sb, nb, tid);
    __syncthreads();
    int cur = 0;
    for (int kb = 1; kb < nkb; ++kb) {
      // A's DMA and the gathers of the next K block in flight during the MFMAs
      if (!a_res)
        gs_stage_a(sa + (cur ^ 1) * GS_TQ * GS_K, a.A, first, cnt, ldh,
                   kb * GS_K, w, lane);
      gsp_gather<V>(nb, sc, stride, ap.cb16, d, dsub, kb * GS_K, tid);
      const unsigned short *cb = sb + cur * GS_TN * GS_K;
      if (!IS_IP) xacc = gs_sumsq(cb, tid, xacc);
      gs_mfma(sa + (size_t)(a_res ? kb - 1 : cur) * GS_TQ * GS_K, cb, acc, wr,
              wc, li, ke);
      gsp_put(sb + (cur ^ 1) * GS_TN * GS_K, nb, tid);
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
      if ((tid & 1) == 0) xn_s[tid >> 1] = xs * xacc;
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
          float key = IS_IP ? -(cst + inv * dv[e]) : (cst - inv * dv[e]) + xv[e];
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
