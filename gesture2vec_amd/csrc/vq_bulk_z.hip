// vq_bulk_z.hip -- bulk code assignment from RAW latents at the checkpoints' width (E = 400): idx = argmin_k |W_pre z + b - w_k|^2
// without writing the projected rows (pipeline.chunks_to_codes, VQ_Payam_EMA.assign; lmdb_data_loader.py:1274-1281).
//
// The contract is bitwise: idx equals g2v_linear_fwd on the route g2v_linear_route names TILED with float4 operands (the forward
// product M = N rows, 400 -> 400, bias, no mask: what the rows this kernel serves, N > smallm_rows, select -- held to the query by
// tests/test_dense_route_host.py) followed by g2v_vq_assign_packed_fwd (vq_assign_p_kernel, 2048 rows and up) on every row -- ties,
// near-ties and non-finite rows included.
//
//   vq_bulkz_pack_kernel     once per call: U = W W_pre (K x E, fp64 sums rounded once to fp32) as bf16 hi / lo images zero-padded
//                            to [Kp][416], per-code constants {c'_k, P_k, Q_k, R0_k} (below), |W_pre|_F, |b| and a non-finite flag.
//                            Nothing is trusted across calls: every workspace byte the sweep reads is written here first.
//   vq_bulkz_sweep_kernel    screens in z-space on the bf16 MFMA (16x16x32), 3-term split (Ul.zh + Uh.zl + Uh.zh), k zero-padded
//                            400 -> 416: the 128 rows of a workgroup sit in registers (32 per wave as bf16 hi / lo fragments), the
//                            codebook streams through LDS in chunks of 32 codes (LDS-DMA, double-buffered, 16-byte pieces
//                            XOR-swizzled by (code >> 1) & 7 inside rows padded to 56 pieces: conflict-free ds_read_b128).
//                            A row is decided when its winner clears every other code by the radius; the rest go to a list.
//   vq_bulkz_recheck_kernel  the listed rows, 16 per workgroup: the projection with gemm_nt_kernel's own chain (same operands,
//                            same k order incl. its zero-padded last k-step, bias added after), then vq_assign_p_kernel's |x|^2,
//                            distance chain, expression and argmin -- the same bits.
//
// ---- the radius (E = 400; u = 2^-24) --------------------------------------------------------------------------------------------
// In reals flat.w_k = z.u_k + b.w_k with u_k = W_pre^T w_k, so  T_k := |w_k|^2 - 2 flat.w_k = c_k - 2 z.u_k,  c_k = |w_k|^2 - 2 b.w_k.
// Screen:  S_k = c_k - 2 A_k,  A_k = the bf16 MFMA chain.  |S_k - T_k| <= 2 |z||u_k| (
//     2^-12.7 x 1.01        fp32 accumulation: 39 MFMAs x 32 products = 1248 sequential fp32 adds, each budgeted 2u (truncating),
//                           partial sums <= sum |products| <= 1.01 |z||u_k| (the accumulator starts at 0: no constants folded in)
//   + 3.01 x 2^-18          bf16 hi / lo of z and of U (|z - zh - zl| <= 2^-18 |z|, likewise U) and the dropped zl.Ul
//   + 2^-24)                fp32 rounding of U (the fp64 sum rounded once)
//   + 3 u (|c_k| + 2.02 |z||u_k|)   the three fp32 roundings of the lower bound's own evaluation (c'_k - |z| P_k - F Q_k - 2 A_k)
//   <= 2^-11.6 |z||u_k| + 2^-22 |c_k|.
// The fp32 route:  x = fl(W_pre z + b) (401-term chains: |x - flat| <= gamma_401 F, F = |W_pre|_F |z| + |b| >= |flat|), then
// d_k = fl(fl(|x|^2) + sq_k) - 2 fl(x.w_k) (400-term chains).  Against the row constant fl(|x|^2) (one value for all k):
//   |(d_k - fl|x|^2) - T_k| <= gamma_400 |w_k|^2 (sq_k)  + 2 gamma_400 F |w_k| (x.w_k)  + 2 gamma_401 F |w_k| (x - flat)
//                              + 2u (F^2 + |w_k|^2 + 2 F |w_k|) (the two roundings of the combination)
//                           <= 2^-15.3 |w_k|^2 + 2^-13.3 F |w_k| + 2^-23 F^2.
// Underflow: products below 2^-126 (flushed or subnormal) in either chain and subnormal split residuals add at most
// 2^-118 |u_k| + 2^-110 |w_k| + 2^-118 |z| + 1e-30.
// Budgeted per code (1.3x to 2x the sums above):  R_k = |z| P_k + F Q_k + R0_k + ROW,
//   P_k = 2^-11 |u_k|,  Q_k = 2^-13 |w_k|,  R0_k = 2^-14 |w_k|^2 + 2^-20 |c_k| + 2^-118 |u_k| + 2^-110 |w_k|,
//   ROW = 2^-22 F^2 + 2^-118 |z| + 1e-30 (the same for every code of the row: only in the margin).
// The sweep ranks the LOWER bounds L_k = c'_k - |z| P_k - F Q_k - 2 A_k (c'_k = c_k - R0_k, from fp64) and decides the row iff
//   L_2 - L_1 > 2 R_a + 2^-22 (|L_1| + |L_2|)          (a = argmin L; the last term: the fp32 subtraction itself)
// with L_1, L_2 and the margin finite and 2^-60 <= |z| <= 2^60: then every other code's fp32 distance lies strictly above the
// winner's, and the fp32 argmin is a whatever its tie rule.  Exact ties (a duplicated code), non-finite rows or codes, overflow:
// the list.  A codebook, W_pre or b with a non-finite value (or a constant that overflows fp32) sends every row to the list.
#include "common.hpp"

namespace g2v {
namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bz_bf16x8;

constexpr int BZ_E = VQ_BULK_Z_E;           // the shipped width: hidden_size 200 x n_layers 2
constexpr int BZ_EP = 416;                  // k zero-padded to 13 k-blocks of 32
constexpr int BZ_KB = BZ_EP / 32;
constexpr int BZ_PIECES = BZ_EP / 8;        // 16-byte pieces per code row: 52
constexpr int BZ_PPAD = 56;                 // LDS row: 52 pieces + 4 unused, swizzle groups of 8
constexpr int BZ_CH = 32;                   // codes per LDS chunk (two 16-code tiles)
constexpr int BZ_RT = 2;                    // row tiles per wave: 32 rows
constexpr int BZ_ROWS = 4 * 16 * BZ_RT;     // rows per workgroup
constexpr int BZ_IMG = BZ_CH * BZ_PPAD * 8; // bf16 elements per chunk image (28 KiB)

__device__ __forceinline__ bool bz_finite(double v) { return fabs(v) <= 3.0e38; }

// one workgroup per padded code row k < Kp; workgroup Kp: |W_pre|_F and |b|
__global__ __launch_bounds__(256) void vq_bulkz_pack_kernel(const float* __restrict__ W, const float* __restrict__ Wp,
                                                           const float* __restrict__ bp, __bf16* __restrict__ Uh,
                                                           __bf16* __restrict__ Ul, float4* __restrict__ cst,
                                                           float* __restrict__ scal, int* __restrict__ flags, int K, int Kp) {
  __shared__ double red[3][256];
  const int k = blockIdx.x, tid = threadIdx.x;
  constexpr int E = BZ_E;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  if (k == Kp) {
    for (int e = tid; e < E * E; e += 256) s0 += (double)Wp[e] * (double)Wp[e];
    for (int e = tid; e < E; e += 256) s1 += (double)bp[e] * (double)bp[e];
  } else {
    for (int j = tid; j < BZ_EP; j += 256) {
      float u = 0.f;
      if (k < K && j < E) {
        double a = 0.0;
        for (int n = 0; n < E; ++n) a += (double)W[(int64_t)k * E + n] * (double)Wp[(int64_t)n * E + j];
        u = (float)a;
      }
      const __bf16 h = (__bf16)u;
      Uh[(int64_t)k * BZ_EP + j] = h;
      Ul[(int64_t)k * BZ_EP + j] = (__bf16)(u - (float)h);
      s0 += (double)u * (double)u;
    }
    if (k < K)
      for (int n = tid; n < E; n += 256) {
        const double w = W[(int64_t)k * E + n];
        s1 += w * w;
        s2 += (double)bp[n] * w;
      }
  }
  red[0][tid] = s0;
  red[1][tid] = s1;
  red[2][tid] = s2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o)
      for (int a = 0; a < 3; ++a) red[a][tid] += red[a][tid + o];
    __syncthreads();
  }
  if (tid) return;
  const double up = 1.0 + 0x1p-20;
  bool bad = false;
  if (k == Kp) {
    const double wpf = sqrt(red[0][0]) * up, bn = sqrt(red[1][0]) * up;
    scal[0] = (float)wpf;
    scal[1] = (float)bn;
    bad = !(bz_finite(wpf) && bz_finite(bn));
  } else if (k >= K) {
    cst[k] = make_float4(INFINITY, 0.f, 0.f, 0.f);     // padding codes: lower bound +inf, never ranked first or second
  } else {
    const double un = sqrt(red[0][0]), ww = red[1][0], wn = sqrt(ww), c = ww - 2.0 * red[2][0];
    const double r0 = (0x1p-14 * ww + 0x1p-20 * fabs(c) + 0x1p-118 * un + 0x1p-110 * wn) * up;
    const double cp = c - r0, P = 0x1p-11 * un * up, Q = 0x1p-13 * wn * up;
    cst[k] = make_float4((float)cp, (float)P, (float)Q, (float)r0);
    bad = !(bz_finite(cp) && bz_finite(P) && bz_finite(Q) && bz_finite(r0) && bz_finite(ww * up));
  }
  if (bad) atomicOr(&flags[1], 1);
}

__global__ __launch_bounds__(256, 1) void vq_bulkz_sweep_kernel(const float* __restrict__ z, const __bf16* __restrict__ Uh,
                                                               const __bf16* __restrict__ Ul, const float4* __restrict__ cst,
                                                               const float* __restrict__ scal, int64_t* __restrict__ idx_out,
                                                               int* __restrict__ und_list, int* __restrict__ und_count, int N,
                                                               int Kp) {
  constexpr int E = BZ_E;
  __shared__ __attribute__((aligned(16))) __bf16 Ls[2][2][BZ_IMG];     // [buffer][hi / lo][code][slot][8]
  __shared__ __attribute__((aligned(16))) float4 Cs[2][BZ_CH];         // [buffer][code]{c', P, Q, R0}
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r0 = blockIdx.x * BZ_ROWS + 16 * BZ_RT * wave;
  // ---- chunk fill: 56 wave-instructions of 1 KiB (both images), 14 per wave; lane -> slot 64 jj + lane of its image, which
  // holds logical piece slot ^ ((code >> 1) & 7) (>= 52: padding, fetched from piece 0 and never read) ----
  auto fill = [&](int c, int buf) {
#pragma unroll
    for (int j = 0; j < 14; ++j) {
      const int g = 14 * wave + j, img = g / 28, ii = g - 28 * img;
      const int slot = 64 * ii + lane, cc = slot / BZ_PPAD, sp = slot - BZ_PPAD * cc;
      int p = sp ^ ((cc >> 1) & 7);
      if (p >= BZ_PIECES) p = 0;
      const __bf16* src = (img ? Ul : Uh) + (int64_t)(c * BZ_CH + cc) * BZ_EP + 8 * p;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)&Ls[buf][img][ii * 512], 16, 0, 0);
    }
    if (wave == 0 && lane < BZ_CH)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(cst + c * BZ_CH + lane),
                                       (__attribute__((address_space(3))) void*)&Cs[buf][0], 16, 0, 0);
  };
  fill(0, 0);
  // ---- this wave's rows as B-operand fragments: lane (i, q) of row tile t holds z[row][32 s + 8 q .. + 7] ----
  bz_bf16x8 xh[BZ_RT][BZ_KB], xl[BZ_RT][BZ_KB];
  float zn[BZ_RT], fr[BZ_RT];
  const float wpf = scal[0], bn = scal[1];
#pragma unroll
  for (int t = 0; t < BZ_RT; ++t) {
    const int row = r0 + 16 * t + i;
    const float* xp = z + (int64_t)(row < N ? row : N - 1) * E + 8 * q;
    float ss = 0.f;
#pragma unroll
    for (int s = 0; s < BZ_KB; ++s) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
      if (32 * s + 8 * q < E) {                          // (E % 8 == 0: a piece is wholly inside or wholly padding)
        a = *reinterpret_cast<const float4*>(xp + 32 * s);
        b = *reinterpret_cast<const float4*>(xp + 32 * s + 4);
      }
      const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const __bf16 h = (__bf16)v[j];
        xh[t][s][j] = h;
        xl[t][s][j] = (__bf16)(v[j] - (float)h);
        ss += v[j] * v[j];
      }
    }
    ss += __shfl_xor(ss, 16);
    ss += __shfl_xor(ss, 32);
    zn[t] = sqrtf(ss) * (1.0f + 0x1p-20f);
    fr[t] = fmaf(wpf, zn[t], bn) * (1.0f + 0x1p-20f);
  }
  float d1[BZ_RT], d2[BZ_RT];
  int k1[BZ_RT];
#pragma unroll
  for (int t = 0; t < BZ_RT; ++t) { d1[t] = INFINITY; d2[t] = INFINITY; k1[t] = 0; }
  const int nch = Kp / BZ_CH;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  const int sw = (i >> 1) & 7;                           // swizzle of code rows 16 tl + i
  for (int c = 0; c < nch; ++c) {
    const int buf = c & 1;
    if (c + 1 < nch) fill(c + 1, buf ^ 1);             // (buffer buf ^ 1 was last read in iteration c - 1, before the barrier)
    f32x4 acc[2][BZ_RT];
#pragma unroll
    for (int tl = 0; tl < 2; ++tl)
#pragma unroll
      for (int t = 0; t < BZ_RT; ++t) acc[tl][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < BZ_KB; ++s) {
      bz_bf16x8 fh[2], fl[2];
#pragma unroll
      for (int tl = 0; tl < 2; ++tl) {
        const int off = ((16 * tl + i) * BZ_PPAD + ((4 * s + q) ^ sw)) * 8;
        fh[tl] = *reinterpret_cast<const bz_bf16x8*>(&Ls[buf][0][off]);
        fl[tl] = *reinterpret_cast<const bz_bf16x8*>(&Ls[buf][1][off]);
      }
#pragma unroll
      for (int tl = 0; tl < 2; ++tl)
#pragma unroll
        for (int t = 0; t < BZ_RT; ++t) acc[tl][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fl[tl], xh[t][s], acc[tl][t], 0, 0, 0);
#pragma unroll
      for (int tl = 0; tl < 2; ++tl)
#pragma unroll
        for (int t = 0; t < BZ_RT; ++t) acc[tl][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fh[tl], xl[t][s], acc[tl][t], 0, 0, 0);
#pragma unroll
      for (int tl = 0; tl < 2; ++tl)
#pragma unroll
        for (int t = 0; t < BZ_RT; ++t) acc[tl][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fh[tl], xh[t][s], acc[tl][t], 0, 0, 0);
    }
    // lower bounds and ranking: lane (i, q) holds codes 16 tl + 4 q + e of row 16 t + i, ascending per lane
#pragma unroll
    for (int tl = 0; tl < 2; ++tl)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float4 k4 = Cs[buf][16 * tl + 4 * q + e];
        const int code = c * BZ_CH + 16 * tl + 4 * q + e;
#pragma unroll
        for (int t = 0; t < BZ_RT; ++t) {
          const float base = fmaf(-fr[t], k4.z, fmaf(-zn[t], k4.y, k4.x));
          const float v = fmaf(-2.0f, acc[tl][t][e], base);
          if (v < d1[t]) {
            d2[t] = d1[t];
            d1[t] = v;
            k1[t] = code;
          } else {
            d2[t] = fminf(d2[t], v);                       // (a NaN leaves both untouched)
          }
        }
      }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of the next chunk has landed ...
    __builtin_amdgcn_s_barrier();                      // ... and everybody's; everybody is done with this chunk's buffer
  }
  const bool all_undecided = und_count[1] != 0;
#pragma unroll
  for (int t = 0; t < BZ_RT; ++t) {
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {               // the four lanes of a row: (smallest, its code, second smallest)
      const float e1 = __shfl_xor(d1[t], o), e2 = __shfl_xor(d2[t], o);
      const int ek = __shfl_xor(k1[t], o);
      const float nd2 = fminf(fminf(d2[t], e2), fmaxf(d1[t], e1));
      if (e1 < d1[t] || (e1 == d1[t] && ek < k1[t])) {
        d1[t] = e1;
        k1[t] = ek;
      }
      d2[t] = nd2;
    }
    const int row = r0 + 16 * t + i;
    if (q == 0 && row < N) {
      const int a = k1[t];
      idx_out[row] = (int64_t)a;
      const float4 ca = cst[a];
      const float f = fr[t], x = zn[t];
      const float ra = fmaf(x, ca.y, fmaf(f, ca.z, ca.w)) + (0x1p-22f * f * f + 0x1p-118f * x + 1e-30f);
      const float margin = 2.0f * ra + 0x1p-22f * (fabsf(d1[t]) + fabsf(d2[t]));
      const bool decided = !all_undecided && x >= 0x1p-60f && x <= 0x1p60f && fabsf(d1[t]) <= 3.0e38f &&
                           fabsf(d2[t]) <= 3.0e38f && margin <= 3.0e38f && d2[t] - d1[t] > margin;
      if (!decided) und_list[atomicAdd(und_count, 1)] = row;
    }
  }
}

// The listed rows, 16 per iteration of a persistent workgroup (8 waves).  Operands, k order and expressions are those of
// gemm_nt_kernel<false, true> (projection: 26 k-steps of 16, the last all zeros, bias added to the finished chain) and of
// vq_assign_p_kernel (|x|^2 by 16 threads per row + reduce16, 25 k-steps, d = (|x|^2 + sq) - 2 acc, argmin_better / merge).
__global__ __launch_bounds__(512) void vq_bulkz_recheck_kernel(const float* __restrict__ z, const float* __restrict__ Wp,
                                                              const float* __restrict__ bp, const float* __restrict__ W,
                                                              const float* __restrict__ wsq, int64_t* __restrict__ idx_out,
                                                              const int* __restrict__ und_list, const int* __restrict__ und_count,
                                                              int K) {
  constexpr int E = BZ_E, LDZ = BZ_EP + 4, LDX = E + 4, NW = 8;
  __shared__ __attribute__((aligned(16))) float Zs[16 * LDZ];
  __shared__ __attribute__((aligned(16))) float Xs[16 * LDX];
  __shared__ float xx[16], wbest_d[NW * 16];
  __shared__ int wbest_k[NW * 16], rows[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
  const int cnt = *und_count;
  for (int base = blockIdx.x * 16; base < cnt; base += gridDim.x * 16) {
    const int nrows = min(16, cnt - base);
    if (tid < 16) rows[tid] = tid < nrows ? und_list[base + tid] : -1;
    __syncthreads();
    for (int e = tid; e < 16 * (BZ_EP / 4); e += 512) {
      const int r = e / (BZ_EP / 4), c = 4 * (e - r * (BZ_EP / 4));
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (rows[r] >= 0 && c < E) v = *reinterpret_cast<const float4*>(z + (int64_t)rows[r] * E + c);
      *reinterpret_cast<float4*>(Zs + r * LDZ + c) = v;
    }
    __syncthreads();
    for (int t = wave; t < E / 16; t += NW) {          // projection: output features 16 t + 4 q + r of row i
      f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
      const float* wrow = Wp + (int64_t)(16 * t + i) * E + 4 * q;
      for (int s = 0; s < BZ_EP / 16; ++s) {
        const float4 wa = 16 * s < E ? *reinterpret_cast<const float4*>(wrow + 16 * s) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 xb = *reinterpret_cast<const float4*>(Zs + i * LDZ + 16 * s + 4 * q);
        acc = mfma16(wa.x, xb.x, acc);
        acc = mfma16(wa.y, xb.y, acc);
        acc = mfma16(wa.z, xb.z, acc);
        acc = mfma16(wa.w, xb.w, acc);
      }
      float v[4] = {acc[0], acc[1], acc[2], acc[3]};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[r] += bp[16 * t + 4 * q + r];
        Xs[i * LDX + 16 * t + 4 * q + r] = v[r];
      }
    }
    __syncthreads();
    {                                                  // ||x||^2 per row: vq_assign_p_kernel's loop
      const int row = tid >> 4, part = tid & 15;
      float sacc = 0.f;
      if (row < 16)
        for (int k = part; k < E; k += 16) sacc += Xs[row * LDX + k] * Xs[row * LDX + k];
      sacc = reduce16(sacc);
      if (part == 0 && row < 16) xx[row] = sacc;
    }
    __syncthreads();
    const float xr = xx[i];
    float bd = INFINITY;
    int bk = 0;
    for (int tl = wave; tl < K / 16; tl += NW) {
      const float4 wq = *reinterpret_cast<const float4*>(wsq + 16 * tl + 4 * q);
      f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
      const float* crow = W + (int64_t)(16 * tl + i) * E + 4 * q;
      for (int s = 0; s < E / 16; ++s) {
        const float4 wa = *reinterpret_cast<const float4*>(crow + 16 * s);
        const float4 xb = *reinterpret_cast<const float4*>(Xs + i * LDX + 16 * s + 4 * q);
        acc = mfma16(wa.x, xb.x, acc);
        acc = mfma16(wa.y, xb.y, acc);
        acc = mfma16(wa.z, xb.z, acc);
        acc = mfma16(wa.w, xb.w, acc);
      }
      const float sq[4] = {wq.x, wq.y, wq.z, wq.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = (xr + sq[e]) - 2.0f * acc[e];
        if (argmin_better(d, bd)) {
          bd = d;
          bk = 16 * tl + 4 * q + e;
        }
      }
    }
    float d2 = __shfl_xor(bd, 16);
    int k2 = __shfl_xor(bk, 16);
    argmin_merge(bd, bk, d2, k2);
    d2 = __shfl_xor(bd, 32);
    k2 = __shfl_xor(bk, 32);
    argmin_merge(bd, bk, d2, k2);
    if (lane < 16) {
      wbest_d[wave * 16 + lane] = bd;
      wbest_k[wave * 16 + lane] = bk;
    }
    __syncthreads();
    if (tid < 16) {
      float d = wbest_d[tid];
      int k = wbest_k[tid];
#pragma unroll
      for (int w = 1; w < NW; ++w) argmin_merge(d, k, wbest_d[w * 16 + tid], wbest_k[w * 16 + tid]);
      if (rows[tid] >= 0) idx_out[rows[tid]] = (int64_t)k;
    }
    __syncthreads();
  }
}

inline size_t bz_pad(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace
}  // namespace g2v

using namespace g2v;

extern "C" size_t g2v_vq_assign_bulk_z_workspace(int N, int E, int K) {
  if (N <= 0 || E <= 0 || K <= 0) return 0;
  const size_t Kp = (size_t)round_up(K, BZ_CH);
  // [counters][scalars][per-code constants][U hi image][U lo image][list of undecided rows]
  return 256 + 256 + bz_pad(Kp * 16) + 2 * bz_pad(Kp * BZ_EP * 2) + bz_pad((size_t)N * 4);
}

extern "C" int g2v_vq_assign_bulk_z(const float* z, const float* w_pre, const float* b_pre, const float* codebook,
                                    const float* code_sqnorm, int64_t* idx, int N, int E, int K, void* workspace,
                                    size_t workspace_bytes, int* undecided, g2v_stream_t stream) {
  G2V_REQUIRE(z && w_pre && b_pre && codebook && code_sqnorm && idx && workspace, "null pointer");
  G2V_REQUIRE(N > 0 && E > 0 && K > 0, "non-positive size");
  const uintptr_t mis = reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(w_pre) | reinterpret_cast<uintptr_t>(codebook) |
                        reinterpret_cast<uintptr_t>(code_sqnorm) | reinterpret_cast<uintptr_t>(workspace);
  const char* why = nullptr;
  if (const int rc = g2v_internal_vq_bulk_z_admits(N, E, K, (mis & 15) == 0, &why)) {      // the plan's BULK_Z row (vq.hip)
    set_error("g2v_vq_assign_bulk_z: %s", why);
    return rc;
  }
  if (workspace_bytes < g2v_vq_assign_bulk_z_workspace(N, E, K)) {
    set_error("g2v_vq_assign_bulk_z: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int Kp = round_up(K, BZ_CH);
  char* w = (char*)workspace;
  int* count = (int*)w;
  float* scal = (float*)(w + 256);
  float4* cst = (float4*)(w + 512);
  __bf16* Uh = (__bf16*)(w + 512 + bz_pad((size_t)Kp * 16));
  __bf16* Ul = (__bf16*)((char*)Uh + bz_pad((size_t)Kp * BZ_EP * 2));
  int* list = (int*)((char*)Ul + bz_pad((size_t)Kp * BZ_EP * 2));
  if (hipMemsetAsync(count, 0, 2 * sizeof(int), st) != hipSuccess) {   // [0] undecided rows, [1] non-finite operand flag
    set_error("g2v_vq_assign_bulk_z: memset failed");
    return G2V_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(vq_bulkz_pack_kernel, dim3(Kp + 1), dim3(256), 0, st, codebook, w_pre, b_pre, Uh, Ul, cst, scal, count, K, Kp);
  hipLaunchKernelGGL(vq_bulkz_sweep_kernel, dim3(cdiv(N, BZ_ROWS)), dim3(256), 0, st, z, (const __bf16*)Uh, (const __bf16*)Ul,
                     (const float4*)cst, (const float*)scal, idx, list, count, N, Kp);
  hipLaunchKernelGGL(vq_bulkz_recheck_kernel, dim3(min(cdiv(N, 16), 1024)), dim3(512), 0, st, z, w_pre, b_pre, codebook,
                     code_sqnorm, idx, (const int*)list, (const int*)count, K);
  if (undecided) (void)hipMemcpyAsync(undecided, count, sizeof(int), hipMemcpyDeviceToDevice, st);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
