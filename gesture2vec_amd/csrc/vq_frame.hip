// vq_frame.hip -- the frame-level quantised autoencoder of Part a (reference scripts/model/DAE_model.py:118-275 VQ_Frame, :351-482
// its own VQ_Payam_EMA; train_eval/train_seq2seq.py:161-241):
//     x (B,D) -> Dropout -> Linear(D,L) -> BatchNorm1d(L) = z -> nearest of K codes = q -> Linear(L,D) = out
//     loss = mse(out, t) + 0.25 mse(q.detach(), z);  the codebook moves by an EMA of the batch's code statistics, not by a gradient.
//
// g2v_vqframe_step: the whole training forward AND backward of one batch as ONE workgroup of sixteen waves.  At the shipped shape
// (128 x 135 x 40 x 80) the iteration is 69 KB of input and ~7 MFLOP; one CU's LDS holds every operand that is used twice.
// Nothing is exchanged with another workgroup: no flag, no spin, no atomic.
//   LDS (floats; ld(n) = n rounded up to 4 mod 8, so that 16 rows x 4 consecutive k of an MFMA operand hit 64 different banks):
//     A   max(B ld(L), L ld(D))   the encoder weight for the first product; then z, then dz, then dy in place
//     XH  B ld(L)                 the linear output y, then the normalised y (BatchNorm's backward reads it)
//     WD  D ld(L)                 the decoder weight (out = q Wd^T and dq = g Wd)
//     EC  K ld(L)                 the OLD codebook: distances, q = EC[id], the loss and dz read it; the new one goes to global only
//     IST L | CS K | HS K | RED 48 | IDX B (16-bit)
//   x, the target and the keep mask are read from global memory (L2 resident: 69 KB) where a product needs them; g = d loss / d out
//   (B,D) goes through a global workspace between the product that makes it and the two that contract it (one workgroup: a
//   __syncthreads orders the stores before the loads).
//   Every matrix product is a chain of v_mfma_f32_16x16x4_f32 per 16x16 output tile, one wave per tile, k ascending; every other sum
//   (batch statistics, code counts, bias gradients, the three scalars) has a fixed tree.  The same input gives the same bits.
//   Steps: S1 y = xm We^T + be | S2 batch statistics, running statistics, xh, z | S3 argmin | S4 counts, EMA state, dw, loss_vq,
//   perplexity | S5 out, g, mse | S6 dz = g Wd + 0.5 (z - q) / (B L); dWd = g^T q, dbd | S7 BatchNorm backward | S8 dWe = dy^T xm, dbe.
//   No dx is formed.
//
// g2v_vqframe_infer: the eval-mode forward over independent tiles of 16 rows (one workgroup of four waves each): encoder, BatchNorm
// on the running statistics, the exact fp32 argmin (lowest index on ties), optionally the decoder.  The weights stream from L2 as
// MFMA operands; a row's result depends on that row alone, so its bits do not depend on what else is in the call.
//
// g2v_vqframe_plan: host arithmetic only -- which route serves a shape and what `auto` takes.
#include "common.hpp"
// shared with vae_frame.hip: frame_ld (the ld(n) above), tile_mma, q_sum, quad_sum, the tile guard (tile_guarded, tile_each), the two
// stage shapes (rows_tile, wgrad_tile), dropped_at, recon_epilogue, argmin_merge16
#include "frame_tile.hpp"

namespace g2v {
namespace {

constexpr int VQF_NW = 16;                      // waves of the training workgroup
constexpr int VQF_THREADS = 64 * VQF_NW;
constexpr int VQF_MAX_L = 256, VQF_MAX_K = 256; // four threads per column / per code in the fixed-order sums
constexpr size_t VQF_LDS_BYTES = 160 * 1024;
constexpr int VQF_INFER_MAX_D = 256, VQF_INFER_MAX_L = 256, VQF_INFER_MAX_K = 4096;
constexpr int VQF_INFER_ROWS = 16, VQF_INFER_NW = 4;

// What `auto` takes (g2v_vqframe_plan): the fused kernel exactly inside the box whose corners were measured faster than the staged
// route (scripts/time_vq_frame.py); the staged route everywhere else, admitted or not.
constexpr int VQF_AUTO_STEP_MAX_B = 256, VQF_AUTO_STEP_MAX_D = 135, VQF_AUTO_STEP_MAX_L = 45, VQF_AUTO_STEP_MAX_K = 128;
constexpr int64_t VQF_AUTO_INFER_MIN_ROWS = 1 << 20;
constexpr int VQF_AUTO_INFER_MAX_D = 135, VQF_AUTO_INFER_MAX_L = 200, VQF_AUTO_INFER_MAX_K = 100;

struct VqfLayout {
  int ldl, ldd;
  size_t a, xh, wd, ec, ist, cs, hs, red, idx, total;      // offsets in floats, total in floats
};
__host__ __device__ inline VqfLayout vqf_layout(int B, int D, int L, int K) {
  VqfLayout o;
  o.ldl = frame_ld(L);
  o.ldd = frame_ld(D);
  const size_t za = (size_t)B * o.ldl, wa = (size_t)L * o.ldd;
  o.a = 0;
  o.xh = o.a + (za > wa ? za : wa);
  o.wd = o.xh + za;
  o.ec = o.wd + (size_t)D * o.ldl;
  o.ist = o.ec + (size_t)K * o.ldl;
  o.cs = o.ist + L;
  o.hs = o.cs + K;
  o.red = o.hs + K;
  o.idx = o.red + 48;
  o.total = o.idx + (B + 1) / 2;
  return o;
}

struct VqfStepArgs {
  const float *x, *t;
  const uint8_t* keep;
  float scale;
  const float *we, *be, *gamma, *beta, *wd, *bd;
  float *rmean, *rvar;
  float *code, *ema_w, *ema_cs;
  float *g_we, *g_be, *g_gamma, *g_beta, *g_wd, *g_bd;
  float* scalars;
  int64_t* ids;
  float *latent, *out;
  float* g;
  int B, D, L, K;
  float momentum, bn_eps, decay, one_minus_decay, vq_eps, k_eps, commitment;
};

__global__ __launch_bounds__(VQF_THREADS) void vqframe_step_kernel(VqfStepArgs p) {
  extern __shared__ __align__(16) float smem[];
  const int B = p.B, D = p.D, L = p.L, K = p.K;
  const VqfLayout o = vqf_layout(B, D, L, K);
  const int ldl = o.ldl, ldd = o.ldd;
  float* A = smem + o.a;
  float* XH = smem + o.xh;
  float* WD = smem + o.wd;
  float* EC = smem + o.ec;
  float* IST = smem + o.ist;
  float* CS = smem + o.cs;
  float* HS = smem + o.hs;
  float* RED = smem + o.red;
  unsigned short* IDX = reinterpret_cast<unsigned short*>(smem + o.idx);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int nrt = (B + 15) >> 4, nlt = (L + 15) >> 4, ndt = (D + 15) >> 4, nkt = (K + 15) >> 4;
  const float invB = 1.0f / (float)B;

  auto xm_at = [&](int b, int d) { return dropped_at(p.x, p.keep, p.scale, D, b, d); };

  // ---- S0: the weights and the old codebook into LDS
  for (int e = tid; e < L * D; e += VQF_THREADS) A[(e / D) * ldd + (e % D)] = p.we[e];
  for (int e = tid; e < D * L; e += VQF_THREADS) WD[(e / L) * ldl + (e % L)] = p.wd[e];
  for (int e = tid; e < K * L; e += VQF_THREADS) EC[(e / L) * ldl + (e % L)] = p.code[e];
  __syncthreads();

  // ---- S1: y = xm We^T + be -> XH
  for (int tt = w; tt < nrt * nlt; tt += VQF_NW)
    rows_tile(D, lane, (tt / nlt) * 16, B, (tt % nlt) * 16, L, xm_at, [&](int k, int l) { return A[l * ldd + k]; },
              [&](int b, int l, float v) { XH[b * ldl + l] = v + p.be[l]; });
  __syncthreads();

  // ---- S2: batch statistics of column c (four threads per column, rows b = rr mod 4), the running statistics, xh and z
  {
    const int c = tid >> 2, rr = tid & 3;
    const bool on = c < L;
    float s = 0.f;
    if (on)
      for (int b = rr; b < B; b += 4) s += XH[b * ldl + c];
    const float mean = quad_sum(s) * invB;
    float ss = 0.f;
    if (on)
      for (int b = rr; b < B; b += 4) {
        const float d = XH[b * ldl + c] - mean;
        ss = fmaf(d, d, ss);
      }
    ss = quad_sum(ss);
    const float istd = 1.0f / sqrtf(ss * invB + p.bn_eps);
    if (on) {
      const float ga = p.gamma[c], be = p.beta[c];
      if (rr == 0) {
        IST[c] = istd;
        p.rmean[c] = (1.0f - p.momentum) * p.rmean[c] + p.momentum * mean;
        p.rvar[c] = (1.0f - p.momentum) * p.rvar[c] + p.momentum * (ss / (float)(B - 1));
      }
      for (int b = rr; b < B; b += 4) {
        const float xh = (XH[b * ldl + c] - mean) * istd;
        const float z = xh * ga + be;
        XH[b * ldl + c] = xh;
        A[b * ldl + c] = z;           // (the encoder weight is dead: every wave has passed the barrier after S1)
        if (p.latent) p.latent[(int64_t)b * L + c] = z;
      }
    }
  }
  __syncthreads();

  // ---- S3: id[b] = argmin_k (|z_b|^2 + |e_k|^2) - 2 z_b . e_k, lowest k on ties; one wave per row tile, the code tiles in turn
  //      (not rows_tile: the tile's own |z|^2 and |e|^2 enter, every lane of a column merges, and one result is kept across tiles)
  for (int rt = w; rt < nrt; rt += VQF_NW) {
    const int r0 = rt * 16;
    float bd_[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
    int bk_[4] = {0, 0, 0, 0};
    for (int kt = 0; kt < nkt; ++kt) {
      const int c0 = kt * 16;
      Side s;
      const f32x4 acc = tile_guarded(
          L, lane, r0, B, c0, K, [&](int b, int k) { return A[b * ldl + k]; }, [&](int k, int c) { return EC[c * ldl + k]; }, s);
      const float zz = q_sum(s.saa);      // |z|^2 of row r0 + (lane & 15)
      const float ee = q_sum(s.sbb);      // |e|^2 of code c0 + (lane & 15)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float zzr = __shfl(zz, 4 * q + r);
        const float d = (zzr + ee) - 2.0f * acc[r];
        if (c0 + j < K) argmin_merge(bd_[r], bk_[r], d, c0 + j);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      argmin_merge16(bd_[r], bk_[r]);
      const int b = r0 + 4 * q + r;
      if (j == 0 && b < B) {
        IDX[b] = (unsigned short)bk_[r];
        p.ids[b] = bk_[r];
      }
    }
  }
  __syncthreads();

  // ---- S4a: code counts (four threads per code), the decayed cluster sizes and the entropy terms; the loss_vq partial sums
  {
    const int c = tid >> 2, rr = tid & 3;
    float cnt = 0.f;
    if (c < K)
      for (int b = rr; b < B; b += 4) cnt += (IDX[b] == c) ? 1.0f : 0.f;
    cnt = quad_sum(cnt);
    if (c < K && rr == 0) {
      CS[c] = p.ema_cs[c] * p.decay + p.one_minus_decay * cnt;
      const float pr = cnt * invB;
      HS[c] = pr * logf(pr + 1e-10f);
    }
    float sq = 0.f;
    for (int e = tid; e < B * L; e += VQF_THREADS) {
      const int b = e / L, l = e - b * L;
      const float d = EC[IDX[b] * ldl + l] - A[b * ldl + l];
      sq = fmaf(d, d, sq);
    }
    sq = wave_sum(sq);
    if (lane == 0) RED[16 + w] = sq;
  }
  __syncthreads();
  if (w == 0) {
    float n = 0.f, h = 0.f;
    for (int c = lane; c < K; c += 64) {
      n += CS[c];
      h += HS[c];
    }
    n = wave_sum(n);
    h = wave_sum(h);
    if (lane == 0) {
      RED[0] = n;
      RED[1] = h;
    }
  }
  __syncthreads();
  if (tid < K) {
    const float n = RED[0];
    const float cs = (CS[tid] + p.vq_eps) / (n + p.k_eps) * n;      // Laplace smoothing
    CS[tid] = cs;
    p.ema_cs[tid] = cs;
  }
  __syncthreads();

  // ---- S4b: dw = onehot^T z, _ema_w and the new codebook (global only) | S5: out = q Wd^T + bd, g = 2 (out - t) / (B D), the mse
  float rec = 0.f;
  {
    const int n4b = nkt * nlt, n5 = nrt * ndt;
    const float gsc = 2.0f / ((float)B * (float)D);
    for (int tt = w; tt < n4b + n5; tt += VQF_NW) {
      if (tt < n4b) {
        rows_tile(B, lane, (tt / nlt) * 16, K, (tt % nlt) * 16, L, [&](int c, int b) { return IDX[b] == c ? 1.0f : 0.f; },
                  [&](int b, int l) { return A[b * ldl + l]; }, [&](int c, int l, float v) {
                    const int64_t e = (int64_t)c * L + l;
                    const float ew = p.ema_w[e] * p.decay + p.one_minus_decay * v;
                    p.ema_w[e] = ew;
                    p.code[e] = ew / CS[c];
                  });
      } else {
        const int t5 = tt - n4b;
        rows_tile(L, lane, (t5 / ndt) * 16, B, (t5 % ndt) * 16, D, [&](int b, int k) { return EC[IDX[b] * ldl + k]; },
                  [&](int k, int d) { return WD[d * ldl + k]; },
                  [&](int b, int d, float v) { recon_epilogue(v, p.bd[d], (int64_t)b * D + d, p.t, gsc, p.out, p.g, rec); });
      }
    }
    rec = wave_sum(rec);
    if (lane == 0) RED[32 + w] = rec;
  }
  __syncthreads();      // (also orders the stores of g before the loads below: one workgroup)
  if (tid == 0) {
    float r = 0.f, v = 0.f;
    for (int k = 0; k < VQF_NW; ++k) {
      r += RED[32 + k];
      v += RED[16 + k];
    }
    p.scalars[0] = r / ((float)B * (float)D);
    p.scalars[1] = p.commitment * (v / ((float)B * (float)L));
    p.scalars[2] = expf(-RED[1]);
  }

  // ---- S6: dz = g Wd + 2 commitment (z - q) / (B L) in place of z | dWd = g^T q, dbd = sum_b g
  {
    const int n6a = nrt * nlt, n6b = ndt * nlt;
    const float cc = 2.0f * p.commitment / ((float)B * (float)L);
    auto g_at = [&](int b, int d) { return p.g[(int64_t)b * D + d]; };
    for (int tt = w; tt < n6a + n6b; tt += VQF_NW) {
      if (tt < n6a) {
        rows_tile(D, lane, (tt / nlt) * 16, B, (tt % nlt) * 16, L, g_at, [&](int k, int l) { return WD[k * ldl + l]; },
                  [&](int b, int l, float v) {
                    const float z = A[b * ldl + l];
                    A[b * ldl + l] = v + cc * (z - EC[IDX[b] * ldl + l]);
                  });
      } else {
        const int t6 = tt - n6a;
        wgrad_tile(B, lane, (t6 / nlt) * 16, D, (t6 % nlt) * 16, L, g_at, [&](int b, int l) { return EC[IDX[b] * ldl + l]; }, p.g_wd,
                   p.g_bd);
      }
    }
  }
  __syncthreads();

  // ---- S7: BatchNorm backward from the batch sums of dz and dz xh; dy in place of dz
  {
    const int c = tid >> 2, rr = tid & 3;
    const bool on = c < L;
    float s1 = 0.f, s2 = 0.f;
    if (on)
      for (int b = rr; b < B; b += 4) {
        const float dz = A[b * ldl + c];
        s1 += dz;
        s2 = fmaf(dz, XH[b * ldl + c], s2);
      }
    s1 = quad_sum(s1);
    s2 = quad_sum(s2);
    if (on) {
      if (rr == 0) {
        p.g_beta[c] = s1;
        p.g_gamma[c] = s2;
      }
      const float m1 = s1 * invB, m2 = s2 * invB, gi = p.gamma[c] * IST[c];
      for (int b = rr; b < B; b += 4) A[b * ldl + c] = (A[b * ldl + c] - m1 - XH[b * ldl + c] * m2) * gi;
    }
  }
  __syncthreads();

  // ---- S8: dWe = dy^T xm, dbe = sum_b dy
  for (int tt = w; tt < nlt * ndt; tt += VQF_NW)
    wgrad_tile(B, lane, (tt / ndt) * 16, L, (tt % ndt) * 16, D, [&](int b, int l) { return A[b * ldl + l]; }, xm_at, p.g_we, p.g_be);
}

// |e_k|^2 of the codebook, one thread per code, l ascending
__global__ __launch_bounds__(256) void vqframe_sqnorm_kernel(const float* __restrict__ code, int K, int L, float* __restrict__ esq) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  float s = 0.f;
  for (int l = 0; l < L; ++l) {
    const float v = code[(int64_t)k * L + l];
    s = fmaf(v, v, s);
  }
  esq[k] = s;
}

struct VqfInferArgs {
  const float* x;
  const float *we, *be, *gamma, *beta, *rmean, *rvar, *code, *esq, *wd, *bd;
  int64_t* ids;
  float *latent, *out;
  int64_t N;
  int D, L, K;
  float bn_eps;
};

// LDS: Z[16][ld(L)] | zz[16] | best distance [4][16] | best code [4][16] | id[16]
__global__ __launch_bounds__(64 * VQF_INFER_NW) void vqframe_infer_kernel(VqfInferArgs p) {
  extern __shared__ __align__(16) float smem[];
  const int D = p.D, L = p.L, K = p.K;
  const int ldl = frame_ld(L);
  float* Z = smem;
  float* ZZ = Z + 16 * ldl;
  float* BD = ZZ + 16;
  int* BK = reinterpret_cast<int*>(BD + 16 * VQF_INFER_NW);
  int* ID = BK + 16 * VQF_INFER_NW;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * VQF_INFER_ROWS;
  const int rows = p.N - r0 < VQF_INFER_ROWS ? (int)(p.N - r0) : VQF_INFER_ROWS;      // of this tile; i below is a row of the tile
  const int nlt = (L + 15) >> 4, ndt = (D + 15) >> 4, nkt = (K + 15) >> 4;
  Side s;

  for (int lt = w; lt < nlt; lt += VQF_INFER_NW) {
    const int l0 = lt * 16;
    const f32x4 acc = tile_guarded(
        D, lane, 0, rows, l0, L, [&](int i, int k) { return p.x[(r0 + i) * D + k]; },
        [&](int k, int l) { return p.we[(int64_t)l * D + k]; }, s);
    // (not rows_tile: Z takes all sixteen rows, the ones past N too, and five column constants are formed once for the four rows)
    const int l = l0 + j;
    if (l < L) {
      const float bias = p.be[l], mu = p.rmean[l], istd = 1.0f / sqrtf(p.rvar[l] + p.bn_eps), ga = p.gamma[l], be = p.beta[l];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 4 * q + r;
        const float z = ((acc[r] + bias) - mu) * istd * ga + be;
        Z[i * ldl + l] = z;
        if (p.latent && i < rows) p.latent[(r0 + i) * L + l] = z;
      }
    }
  }
  __syncthreads();
  if (tid < 16) {
    float zz = 0.f;
    for (int l = 0; l < L; ++l) zz = fmaf(Z[tid * ldl + l], Z[tid * ldl + l], zz);
    ZZ[tid] = zz;
  }
  __syncthreads();
  {
    float bd_[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
    int bk_[4] = {0, 0, 0, 0};
    for (int kt = w; kt < nkt; kt += VQF_INFER_NW) {
      const int c0 = kt * 16;
      // (not rows_tile: the merge needs the accumulator's index r; all sixteen rows of Z are defined)
      const f32x4 acc = tile_guarded(
          L, lane, 0, 16, c0, K, [&](int i, int k) { return Z[i * ldl + k]; }, [&](int k, int c) { return p.code[(int64_t)c * L + k]; },
          s);
      tile_each(lane, 0, 16, c0, K, [&](int r, int i, int c) { argmin_merge(bd_[r], bk_[r], (ZZ[i] + p.esq[c]) - 2.0f * acc[r], c); });
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      argmin_merge16(bd_[r], bk_[r]);
      if (j == 0) {
        BD[w * 16 + 4 * q + r] = bd_[r];
        BK[w * 16 + 4 * q + r] = bk_[r];
      }
    }
  }
  __syncthreads();
  if (tid < 16) {
    float d = BD[tid];
    int k = BK[tid];
    for (int ww = 1; ww < VQF_INFER_NW; ++ww) argmin_merge(d, k, BD[ww * 16 + tid], BK[ww * 16 + tid]);
    ID[tid] = k;
    if (tid < rows) p.ids[r0 + tid] = k;
  }
  if (p.out == nullptr) return;
  __syncthreads();
  for (int dt = w; dt < ndt; dt += VQF_INFER_NW)
    rows_tile(L, lane, 0, rows, dt * 16, D, [&](int i, int k) { return p.code[(int64_t)ID[i] * L + k]; },
              [&](int k, int d) { return p.wd[(int64_t)d * L + k]; },
              [&](int i, int d, float v) { p.out[(r0 + i) * D + d] = v + p.bd[d]; });
}

const char* step_refusal(int B, int D, int L, int K) {
  if (B < 2) return "a training batch needs B >= 2 (BatchNorm1d on batch statistics)";
  if (D < 1 || L < 1 || K < 1) return "bad size";
  if (L > VQF_MAX_L) return "the fused step serves L <= 256";
  if (K > VQF_MAX_K) return "the fused step serves K <= 256";
  if ((int64_t)B * D > INT32_MAX) return "B * D exceeds 2^31";
  const VqfLayout o = vqf_layout(B, D, L, K);
  if (o.total * sizeof(float) > VQF_LDS_BYTES) return "the batch does not fit one CU's 160 KB of LDS";
  return nullptr;
}
const char* infer_refusal(int64_t N, int D, int L, int K) {
  if (N < 1 || D < 1 || L < 1 || K < 1) return "bad size";
  if (D > VQF_INFER_MAX_D) return "the grid kernel serves D <= 256";
  if (L > VQF_INFER_MAX_L) return "the grid kernel serves L <= 256";
  if (K > VQF_INFER_MAX_K) return "the grid kernel serves K <= 4096";
  if (cdiv(N, VQF_INFER_ROWS) > INT32_MAX / 2) return "too many rows for one grid";
  return nullptr;
}

}  // namespace
}  // namespace g2v

using namespace g2v;

static bool vqf_auto_takes_fused(int B, int D, int L, int K, int training) {
  if (training) return B <= VQF_AUTO_STEP_MAX_B && D <= VQF_AUTO_STEP_MAX_D && L <= VQF_AUTO_STEP_MAX_L && K <= VQF_AUTO_STEP_MAX_K;
  return B >= VQF_AUTO_INFER_MIN_ROWS && D <= VQF_AUTO_INFER_MAX_D && L <= VQF_AUTO_INFER_MAX_L && K <= VQF_AUTO_INFER_MAX_K;
}

extern "C" int g2v_vqframe_plan(int B, int D, int L, int K, int training) {
  if (D < 1 || L < 1 || K < 1 || B < (training ? 2 : 1)) return G2V_VQFRAME_REFUSED;
  const bool ok = training ? step_refusal(B, D, L, K) == nullptr : infer_refusal(B, D, L, K) == nullptr;
  const bool take = ok && vqf_auto_takes_fused(B, D, L, K, training);
  return (take ? G2V_VQFRAME_FUSED : G2V_VQFRAME_STAGED) | (ok ? G2V_VQFRAME_FUSED_OK : 0);
}

extern "C" const char* g2v_vqframe_plan_reason(int B, int D, int L, int K, int training) {
  if (D < 1 || L < 1 || K < 1 || B < 1) return "refused: bad size";
  if (training && B < 2) return "refused: a training batch needs B >= 2 (BatchNorm1d on batch statistics)";
  const char* why = training ? step_refusal(B, D, L, K) : infer_refusal(B, D, L, K);
  if (why) return why;
  if (vqf_auto_takes_fused(B, D, L, K, training)) return "fused: inside the shapes measured faster than the staged route";
  return training ? "staged: the fused step is admitted but not measured faster at this shape"
                  : "staged: the grid kernel is admitted but not measured faster at this shape";
}

extern "C" size_t g2v_vqframe_workspace(int B, int D, int L, int K, int training) {
  if (training) return step_refusal(B, D, L, K) ? 0 : (size_t)round_up(B * D, 4) * sizeof(float);
  return infer_refusal(B, D, L, K) ? 0 : (size_t)round_up(K, 4) * sizeof(float);
}

extern "C" size_t g2v_vqframe_step_lds(int B, int D, int L, int K) {
  return step_refusal(B, D, L, K) ? 0 : vqf_layout(B, D, L, K).total * sizeof(float);
}

extern "C" int g2v_vqframe_step(const float* x, const float* target, const uint8_t* keep, float scale, const float* w_enc,
                                const float* b_enc, const float* bn_weight, const float* bn_bias, float* running_mean,
                                float* running_var, float momentum, const float* w_dec, const float* b_dec, float* codebook,
                                float* ema_w, float* ema_cluster_size, float commitment, double decay, double epsilon,
                                float* g_w_enc, float* g_b_enc, float* g_bn_weight, float* g_bn_bias, float* g_w_dec, float* g_b_dec,
                                float* scalars, int64_t* ids, float* latent, float* out, void* workspace, size_t workspace_bytes,
                                int B, int D, int L, int K, g2v_stream_t stream) {
  G2V_REQUIRE(x && target && w_enc && b_enc && bn_weight && bn_bias && running_mean && running_var && w_dec && b_dec, "null pointer");
  G2V_REQUIRE(codebook && ema_w && ema_cluster_size, "null quantiser state");
  G2V_REQUIRE(g_w_enc && g_b_enc && g_bn_weight && g_bn_bias && g_w_dec && g_b_dec && scalars && ids && workspace, "null output pointer");
  if (const char* why = step_refusal(B, D, L, K)) {
    set_error("g2v_vqframe_step: shape not served: %s (see g2v_vqframe_plan)", why);
    return B < 2 || D < 1 || L < 1 || K < 1 ? G2V_ERR_ARG : G2V_ERR_UNSUPPORTED;
  }
  G2V_REQUIRE(workspace_bytes >= g2v_vqframe_workspace(B, D, L, K, 1), "workspace too small");
  VqfStepArgs a;
  a.x = x; a.t = target; a.keep = keep; a.scale = scale;
  a.we = w_enc; a.be = b_enc; a.gamma = bn_weight; a.beta = bn_bias; a.wd = w_dec; a.bd = b_dec;
  a.rmean = running_mean; a.rvar = running_var;
  a.code = codebook; a.ema_w = ema_w; a.ema_cs = ema_cluster_size;
  a.g_we = g_w_enc; a.g_be = g_b_enc; a.g_gamma = g_bn_weight; a.g_beta = g_bn_bias; a.g_wd = g_w_dec; a.g_bd = g_b_dec;
  a.scalars = scalars; a.ids = ids; a.latent = latent; a.out = out; a.g = static_cast<float*>(workspace);
  a.B = B; a.D = D; a.L = L; a.K = K;
  a.momentum = momentum; a.bn_eps = 1e-5f;
  a.decay = (float)decay; a.one_minus_decay = (float)(1.0 - decay); a.vq_eps = (float)epsilon; a.k_eps = (float)(K * epsilon);
  a.commitment = commitment;
  const size_t lds = vqf_layout(B, D, L, K).total * sizeof(float);
  if (!g2v_internal_lds_reserve((const void*)vqframe_step_kernel, lds)) return G2V_ERR_LAUNCH;
  hipLaunchKernelGGL(vqframe_step_kernel, dim3(1), dim3(VQF_THREADS), lds, (hipStream_t)stream, a);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int g2v_vqframe_infer(const float* x, int64_t N, const float* w_enc, const float* b_enc, const float* bn_weight,
                                 const float* bn_bias, const float* running_mean, const float* running_var, const float* codebook,
                                 const float* w_dec, const float* b_dec, int64_t* ids, float* latent, float* out, void* workspace,
                                 size_t workspace_bytes, int D, int L, int K, g2v_stream_t stream) {
  G2V_REQUIRE(x && w_enc && b_enc && bn_weight && bn_bias && running_mean && running_var && codebook && ids && workspace, "null pointer");
  G2V_REQUIRE(out == nullptr || (w_dec && b_dec), "the output needs the decoder's weight and bias");
  if (const char* why = infer_refusal(N, D, L, K)) {
    set_error("g2v_vqframe_infer: shape not served: %s", why);
    return N < 1 || D < 1 || L < 1 || K < 1 ? G2V_ERR_ARG : G2V_ERR_UNSUPPORTED;
  }
  G2V_REQUIRE(workspace_bytes >= (size_t)round_up(K, 4) * sizeof(float), "workspace too small");
  VqfInferArgs a;
  a.x = x; a.we = w_enc; a.be = b_enc; a.gamma = bn_weight; a.beta = bn_bias; a.rmean = running_mean; a.rvar = running_var;
  a.code = codebook; a.esq = static_cast<float*>(workspace); a.wd = w_dec; a.bd = b_dec;
  a.ids = ids; a.latent = latent; a.out = out; a.N = N; a.D = D; a.L = L; a.K = K; a.bn_eps = 1e-5f;
  hipLaunchKernelGGL(vqframe_sqnorm_kernel, dim3(cdiv(K, 256)), dim3(256), 0, (hipStream_t)stream, codebook, K, L,
                     static_cast<float*>(workspace));
  G2V_CHECK_LAUNCH();
  const size_t lds = (size_t)(16 * frame_ld(L) + 16 + 32 * VQF_INFER_NW + 16) * sizeof(float);
  hipLaunchKernelGGL(vqframe_infer_kernel, dim3(cdiv(N, VQF_INFER_ROWS)), dim3(64 * VQF_INFER_NW), lds, (hipStream_t)stream, a);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
