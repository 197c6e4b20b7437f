// dfann — list-major ("grouped") scan of 8-bit IVFSQ lists (spec
// "scan_group_sq8"). Included by dfann.hip after
// scan_group.hip, whose grouping stages (k_grp_zero / count / tiles /
// scatter), tile table and A staging it reuses as they are.
//
// Operand algebra. The faiss 8-bit codec decodes x_t = vmin_t + (c_t + 0.5)
// s_t with s_t = vdiff_t / 255 (the engine's sq_scale). Centred on the middle
// of the range, b_t = c_t - 128 in [-128, 127] (exact in fp16) and mid_t =
// vmin_t + 128.5 s_t give x_t = mid_t + s_t b_t, so
//   L2  with w_t = (q_t - cent_t) - mid_t:
//         D = sum (w_t - s_t b_t)^2 = W - 2 sum (w_t s_t) b_t + V,
//         W = sum w_t^2 per pair, V = sum (s_t b_t)^2 per row;
//   IP    dot = q.c + sum q_t mid_t + sum (q_t s_t) b_t, no per-row term.
// Uncentred (c_t in [0, 255], offset vmin) the three L2 terms are about four
// times larger for the same distance and cancel that much harder.
//
// The MFMA multiplies A rows a_t = w_t s_t (L2) or q_t s_t (IP) against the
// stored bytes widened EXACTLY to the halves b_t: only the query side is
// rounded, once per a_t. a_t of normalised embeddings sits near or below the
// fp16 normal range, so every A row carries a power of two 2^e that puts its
// largest magnitude into [2^14, 2^15); 2^-e multiplies the dot back in fp32.

#define GS8_KB 128                      // codes of a K block (two GS_K halves of A)
#define GS8_A_BYTES (2 * GS_A_BYTES)    // 16 KB, one K block of A
#define GS8_LDS_MAX (160 * 1024)

// LDS bytes of k_scan_sq8_grp at dimension d: B buffers, row terms, A region
// (resident while all K blocks fit in GS_A_RES_MAX, else two), per-dimension
// scales of every K block
__host__ __device__ __forceinline__ size_t gs8_lds_bytes(int d) {
  size_t nkb = ((size_t)d + GS8_KB - 1) / GS8_KB;
  bool res = nkb * GS8_A_BYTES <= GS_A_RES_MAX;
  return GS_A_OFF + (res ? nkb : 2) * GS8_A_BYTES + nkb * GS8_KB * 4;
}

// One wave per grouped slot. a_t in fp32, then the row's 2^e, then one
// rounding to fp16; ld = round_up(d, 16) halves, zero pad. e puts max |a_t|
// 2^e into [2^14, 2^15) (clamped to |e| <= 126, so that 2^e and 2^-e stay
// normal); 0 for an all-zero row; a row with a non-finite entry is left
// unscaled so that NaN propagates. cst = W (L2) or q.c + sum q_t mid_t (IP),
// lane l adding t = l, l + 64, ... then a fixed shuffle tree.
extern "C" __global__ __launch_bounds__(256) void k_grp_operands_sq8(
    const float *__restrict__ q, const float *__restrict__ cent,
    const int *__restrict__ probes, const float *__restrict__ keys,
    const int *__restrict__ order, const int *__restrict__ meta,
    const float *__restrict__ vmin, const float *__restrict__ scale,
    int nprobe, int d, int ld, int ip, unsigned short *__restrict__ A,
    float *__restrict__ cst, float *__restrict__ inv) {
  long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= meta[GS_META_NGRP]) return;
  const int lane = threadIdx.x & 63;
  const int p = order[s];
  const float *qp = q + (long long)(p / nprobe) * d;
  const float *cp = cent + (long long)probes[p] * d;
  float acc = 0.f, amax = 0.f;
  bool bad = false;
  for (int t = lane; t < d; t += 64) {
    float sc = scale[t], mid = vmin[t] + 128.5f * sc;
    float a;
    if (ip) {
      acc += qp[t] * mid;
      a = qp[t] * sc;
    } else {
      float w = (qp[t] - cp[t]) - mid;
      acc += w * w;
      a = w * sc;
    }
    bad |= !(fabsf(a) <= DFANN_FLT_MAX);  // NaN or inf
    amax = fmaxf(amax, fabsf(a));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc += __shfl_down(acc, o, 64);
    amax = fmaxf(amax, __shfl_xor(amax, o, 64));  // max: order-free
  }
  int e = 0;
  if (__builtin_amdgcn_ballot_w64(bad) == 0 && amax > 0.f) {
    int x;
    frexpf(amax, &x);  // amax in [2^(x-1), 2^x)
    e = min(max(15 - x, -126), 126);
  }
  const float up = ldexpf(1.0f, e);
  for (int t = lane; t < ld; t += 64) {
    float a = 0.f;
    if (t < d) {
      float sc = scale[t];
      a = ip ? qp[t] * sc : ((qp[t] - cp[t]) - (vmin[t] + 128.5f * sc)) * sc;
    }
    A[s * ld + t] = __half_as_ushort(__float2half(a * up));
  }
  if (lane == 0) {
    cst[s] = ip ? acc - keys[p] : acc;  // IP: the coarse key is -(q . c)
    inv[s] = ldexpf(1.0f, -e);
  }
}

// ---------------------------------------------------------------------------
// k_scan_sq8_grp<KP, IS_IP, FILT>: 256 threads, one tile-table entry per
// block — list L, pair slots [first, first + cnt), cnt <= GS_TQ — GS_TQ pair
// rows x GS_TN list rows, four waves as 2 x 2, acc[2][4] on
// v_mfma_f32_16x16x32_f16, RegTopK<KP> across all row tiles: the frame of
// k_scan_sqf_grp. What differs, and the decisions taken:
//
// B staging and conversion. A K block is GS8_KB = 128 codes, so the B buffer
// is [128 rows][128 bytes], byte for byte the fp16 kernel's tile: gs_stage_b
// stages it (16-byte global_load_lds, XOR group swizzle, 2 x 16 KB), and the
// bytes stay bytes in LDS. A lane's MFMA fragment is one 8-byte LDS read,
// widened in registers: v_perm_b32 against 0x64 makes the halves 0x6400 | c
// = 1024 + c, and one packed half add of -1152 a pair gives c - 128, exactly.
// B fragment traffic from LDS is half the fp16 kernel's per code. The
// alternative (convert at staging, fp16 in LDS) was not built: it doubles
// the LDS bytes that BASELINE.md names as the fp16 kernel's bound and gives
// up the DMA staging.
//
// A tile. A K block of A is two GS_K-half sub-blocks in the fp16 kernel's
// layout (gs_stage_a, 2 x 8 KB). Resident across the list's row tiles while
// nkb x 16 KB fits GS_A_RES_MAX (d <= 768), else double-buffered and re-read
// per row tile. Every sub-block of every K block is staged, the ones past ld
// as zeros: B bytes past the stride are staged as zero BYTES, which widen to
// -128, and only a zero in A silences them. The same holds for the stored
// zero pad in [d, stride).
//
// V per row (L2). Thread t owns the 16-byte group G = t & 7 of rows (t >> 3)
// + 32 i, i < 4: the scales of its 16 dimensions sit in registers for the K
// block (from the LDS copy of sq_scale, zero at t >= d, which is how V skips
// the tail), a row's eight group sums meet by a fixed xor tree after the K
// loop. A wave's read of a block is 1 KB of consecutive LDS. V therefore
// depends on the row and on its place in the row-tile partition only.
//
// Key: L2 (W - 2 2^-e dot) + V, IP -(cst + 2^-e dot). Admission, FILT, the
// four-thread merge, the output slot: k_scan_sqf_grp's. Plain vector stores,
// no atomics. INVARIANT as there: a pair's result does not depend on the rest
// of the batch (2^e depends on the pair's own row alone).
// ---------------------------------------------------------------------------

typedef __attribute__((ext_vector_type(2))) float gs8_f32x2;

// 8 stored bytes -> the 8 halves c - 128
__device__ __forceinline__ f16x8 gs8_widen(uint2 v) {
  const f16x2 off = {(_Float16)-1152.0f, (_Float16)-1152.0f};
  // selector bytes 0..3 pick from the second operand, 4 the 0x64 of the first
  f16x2 h0 = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(0x64646464u, v.x, 0x04010400u)) + off;
  f16x2 h1 = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(0x64646464u, v.x, 0x04030402u)) + off;
  f16x2 h2 = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(0x64646464u, v.y, 0x04010400u)) + off;
  f16x2 h3 = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(0x64646464u, v.y, 0x04030402u)) + off;
  return f16x8{h0[0], h0[1], h1[0], h1[1], h2[0], h2[1], h3[0], h3[1]};
}

// sa: the K block's two A sub-blocks; sb: the staged bytes [GS_TN][GS8_KB]
__device__ __forceinline__ void gs8_mfma(const unsigned short *sa,
                                         const uint8_t *sb, f32x4 (&acc)[2][4],
                                         int wr, int wc, int li, int ke) {
#pragma unroll
  for (int kk = 0; kk < GS8_KB; kk += 32) {
    const unsigned short *sk = sa + (kk >> 6) * (GS_TQ * GS_K);
    f16x8 a[2];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
      int ra = wr + ti * 16 + li;
      a[ti] = *reinterpret_cast<const f16x8 *>(
          sk + ra * GS_K + (((kk & 63) + ke) ^ ((ra & 7) << 3)));
    }
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
      int rb = wc + tj * 16 + li;
      int o = kk + ke;  // first of the lane's 8 codes
      f16x8 b = gs8_widen(*reinterpret_cast<const uint2 *>(
          sb + rb * GS8_KB + ((((o >> 4) ^ (rb & 7)) << 4) | (o & 8))));
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
        acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
            a[ti], b, acc[ti][tj], 0, 0, 0);
    }
  }
}

// (s_t b_t)^2 of one staged block; sk: the block's 128 scales
__device__ __forceinline__ void gs8_rowterm(const uint8_t *sb, const float *sk,
                                            int tid, gs8_f32x2 (&xacc)[4]) {
  const int G = tid & 7, rr = tid >> 3;
  gs8_f32x2 sv[8], ov[8];  // s_t and -128 s_t of the thread's 16 dimensions
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float4 v = *reinterpret_cast<const float4 *>(sk + G * 16 + j * 4);
    sv[2 * j] = gs8_f32x2{v.x, v.y};
    sv[2 * j + 1] = gs8_f32x2{v.z, v.w};
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) ov[j] = sv[j] * -128.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int r = rr + 32 * i;
    uint4 v = *reinterpret_cast<const uint4 *>(sb + r * GS8_KB +
                                               ((G ^ (r & 7)) << 4));
    const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      gs8_f32x2 c0 = {(float)(u[j] & 0xffu), (float)((u[j] >> 8) & 0xffu)};
      gs8_f32x2 c1 = {(float)((u[j] >> 16) & 0xffu), (float)(u[j] >> 24)};
      gs8_f32x2 x0 = c0 * sv[2 * j] + ov[2 * j];
      gs8_f32x2 x1 = c1 * sv[2 * j + 1] + ov[2 * j + 1];
      xacc[i] = x0 * x0 + xacc[i];
      xacc[i] = x1 * x1 + xacc[i];
    }
  }
}

// the fp16 kernel's arguments (qn: W or the IP constant, ldh: ld) and the
// 8-bit extras
struct Grp8ScanArgs {
  GrpScanArgs g;
  const float *inv, *scale;
  int d;
};

template <int KP, bool IS_IP, bool FILT>
__global__ __launch_bounds__(256) void k_scan_sq8_grp(Grp8ScanArgs a8) {
  const GrpScanArgs &a = a8.g;
  extern __shared__ __attribute__((aligned(16))) char gsm[];
  if ((int)blockIdx.x >= a.meta[GS_META_NTILES]) return;
  const int4 te = a.tiles[blockIdx.x];
  const long long first = te.y;
  const int cnt = te.z;
  const long long l0 = a.off[te.x], l1 = a.off[te.x + 1];
  const int ld = a.ldh, nkb = (a8.d + GS8_KB - 1) / GS8_KB;
  const int sth = a.stride / 2;  // gs_stage_b counts the row in halves
  const bool a_res = a.a_res != 0;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = (w >> 1) * 32, wc = (w & 1) * 64;
  const int li = lane & 15, ke = (lane >> 4) * 8, rrow = (lane >> 4) * 4;
  unsigned short *sb = reinterpret_cast<unsigned short *>(gsm);
  float *xn_s = reinterpret_cast<float *>(gsm + GS_XN_OFF);
  unsigned short *sa = reinterpret_cast<unsigned short *>(gsm + GS_A_OFF);
  float *sc_s = reinterpret_cast<float *>(
      gsm + GS_A_OFF + (size_t)(a_res ? nkb : 2) * GS8_A_BYTES);
  float *tile = reinterpret_cast<float *>(gsm);  // [GS_TQ][GS_TN] over B
  constexpr int AK = 2 * GS_TQ * GS_K;  // halves of a K block of A
  const int srow = tid >> 2, sch = tid & 3;
  const int rot = ((tid >> 2) & 3) * 2 + ((tid & 3) >> 1);
  const bool live = srow < cnt;
  const float cst = live ? a.qn[first + srow] : 0.f;
  // L2 takes 2 * 2^-e (exact), IP 2^-e
  const float inv = live ? (IS_IP ? 1.0f : 2.0f) * a8.inv[first + srow] : 0.f;
  RegTopK<KP> loc;
  loc.init();
  if (!IS_IP)
    for (int t = tid; t < nkb * GS8_KB; t += 256)
      sc_s[t] = t < a8.d ? a8.scale[t] : 0.f;  // visible after the first barrier

  // both sub-blocks of K block kb of A
  auto stage_a = [&](unsigned short *dst, int kb) {
    gs_stage_a(dst, a.A, first, cnt, ld, kb * GS8_KB, w, lane);
    gs_stage_a(dst + GS_TQ * GS_K, a.A, first, cnt, ld, kb * GS8_KB + GS_K, w,
               lane);
  };

  for (long long r0 = l0; r0 < l1; r0 += GS_TN) {
    f32x4 acc[2][4] = {};
    gs8_f32x2 xacc[4] = {};
    if (a_res) {
      if (r0 == l0)
        for (int kb = 0; kb < nkb; ++kb) stage_a(sa + (size_t)kb * AK, kb);
    } else {
      stage_a(sa, 0);
    }
    gs_stage_b(sb, a.codes, a.rlog, a.stride, r0, l1, sth, 0, w, lane);
    __syncthreads();
    int cur = 0;
    for (int kb = 1; kb < nkb; ++kb) {
      // DMA of the next K block in flight during the MFMAs
      if (!a_res) stage_a(sa + (cur ^ 1) * AK, kb);
      gs_stage_b(sb + (cur ^ 1) * GS_TN * GS_K, a.codes, a.rlog, a.stride, r0,
                 l1, sth, kb * GS_K, w, lane);
      const uint8_t *cb =
          reinterpret_cast<const uint8_t *>(sb + cur * GS_TN * GS_K);
      if (!IS_IP) gs8_rowterm(cb, sc_s + (kb - 1) * GS8_KB, tid, xacc);
      gs8_mfma(sa + (size_t)(a_res ? kb - 1 : cur) * AK, cb, acc, wr, wc, li,
               ke);
      __syncthreads();  // drains the glds queue (vmcnt(0) inside)
      cur ^= 1;
    }
    {
      const uint8_t *cb =
          reinterpret_cast<const uint8_t *>(sb + cur * GS_TN * GS_K);
      if (!IS_IP) gs8_rowterm(cb, sc_s + (nkb - 1) * GS8_KB, tid, xacc);
      gs8_mfma(sa + (size_t)(a_res ? nkb - 1 : cur) * AK, cb, acc, wr, wc, li,
               ke);
    }
    __syncthreads();  // every wave is done with the B buffers
    if (!IS_IP) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float x = xacc[i][0] + xacc[i][1];
        x += __shfl_xor(x, 1, 64);
        x += __shfl_xor(x, 2, 64);
        x += __shfl_xor(x, 4, 64);
        if ((tid & 7) == 0) xn_s[(tid >> 3) + 32 * i] = x;
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
