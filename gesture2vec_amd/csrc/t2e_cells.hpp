// t2e_cells.hpp -- what the per-step kernels of the text -> gesture decoders share: the tiling constants, the LDS carves, the
// argument blocks, the pieces of a forward launch (BatchNorm finish, cells, out layer with feedback, attention head, pre_linear with
// its partial sums), Part A of a backward launch (BatchNorm backward finish, attention backward) and the GRU cells' BPTT step of one
// 16-row workgroup.  t2e_rollout.hip (discrete codes, greedy feedback without a gradient), t2e_latent.hip (continuous latents, the
// output fed back WITH its gradient) and pose_attn.hip (poses, attention AND such feedback) all build on it.
#pragma once
#include "gru_cells.hpp"

namespace g2v {

constexpr int CT_NTHR = 512, CT_NW = CT_NTHR / 64;
constexpr int CT_MAX_TW = 64;

struct CodePackF {      // packed forward weights (fragment-major, common.hpp)
  const float* pre;     // rows H, K = Hin
  const float* ih0; const float* hh0; const float* ih1; const float* hh1;   // 3 gate groups x H rows, K = H
  const float* out;     // rows K (tiles padded to a multiple of 4 * CT_NW), K = H
  const float* attn_h;  // rows H, K = H  (W_attn[:, :H])
};
struct CodePackB {      // packed transposed weights for the backward
  const float* out_t;   // rows H, K = Kdim   (W_out^T)
  const float* ih0_t; const float* hh0_t; const float* ih1_t; const float* hh1_t;   // rows H, K = 3H
  const float* pre_ctx_t;   // rows H (context features), K = H: W_pre[:, H:2H]^T          (attention)
  const float* attn_h_t;    // rows H (state features), K = H: W_attn[:, :H]^T              (attention)
};
struct CodeDims {
  int S1, B, H, K, Hin, Tw;
  float p_drop;
  int n_pre, training, nblk, att, scratch;
};

static inline int ct_ktiles_alloc(int K) { return round_up((K + 15) >> 4, 4 * CT_NW); }

// LDS carve of the forward kernel (floats)
struct CtFwdLds {
  int xa, xh0, xh1, xx1, xh1n, xe, st, red, scratch, amv, amk, ids, sc, total;
};
static __host__ __device__ inline CtFwdLds ct_fwd_lds(int H, int Hin, int Tw, int scratch) {
  const int Hp = (H + 15) & ~15, ldh = Hp + 4, ldx = ((Hin + 15) & ~15) + 4;
  CtFwdLds l;
  int o = 0;
  l.xa = o; o += 16 * ldh;
  l.xh0 = o; o += 16 * ldh;
  l.xh1 = o; o += 16 * ldh;
  l.xx1 = o; o += 16 * ldh;
  l.xh1n = o; o += 16 * ldh;
  l.xe = o; o += 16 * ldx;
  l.st = o; o += 2 * Hp;
  l.red = o; o += 2 * Hp;
  l.scratch = o; o += scratch;
  l.amv = o; o += CT_NW * 16;
  l.amk = o; o += CT_NW * 16;
  l.ids = o; o += 16;
  l.sc = o; o += 16 * (Tw > 0 ? Tw : 1);
  l.total = o;
  return l;
}

// =====================================================================================================================
// forward pieces of one launch, single-sourced for the three step kernels (t2e_rollout.hip, t2e_latent.hip, pose_attn.hip)
// =====================================================================================================================
// Biased batch variance from the sums over the batch of c = u - b_pre: s2 = sum c^2, mv = sum c / B.  One row has no spread: its
// variance is 0, not what the difference leaves -- the compiler contracts it to fma(-mv, mv, s2), which at B = 1 is the rounding
// residue of mv^2, up to 2^-24 c^2, and against eps = 1e-5 that moved 1 / sqrt(var + eps) by 2e-3 at |c| of a few.
__device__ __forceinline__ float bn_batch_var(float s2, float mv, int B) {
  return B > 1 ? fmaxf(s2 / (float)B - mv * mv, 0.f) : 0.f;
}

// this block's rows of u_t, h0_t, h1_t (written by the previous launch on some other CU), one float4 group per thread and slot
constexpr int CT_NPF = 2;                                  // 16 x H / 4 <= 1024 float4 (H <= 256)
struct CtRowPf {
  float4 u[CT_NPF], h0[CT_NPF], h1[CT_NPF];
  int r[CT_NPF], c[CT_NPF];
  bool v[CT_NPF];
};
__device__ __forceinline__ void ct_fwd_prefetch(CtRowPf& p, const g2v_code_dec_saved& sv, const float* __restrict__ h_init, int t,
                                                bool has_tail, int B, int H, int b0, int nrows, int tid) {
  const int H4 = H >> 2;
#pragma unroll
  for (int k = 0; k < CT_NPF; ++k) {
    const int e = tid + k * CT_NTHR;
    p.r[k] = e / H4;
    p.c[k] = (e - p.r[k] * H4) * 4;
    p.v[k] = e < 16 * H4 && p.r[k] < nrows;
    p.u[k] = p.h0[k] = p.h1[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.v[k]) {
      if (has_tail) {
        const int64_t row = ((int64_t)t * B + b0 + p.r[k]) * H + p.c[k];
        p.u[k] = *reinterpret_cast<const float4*>(sv.u + row);
        p.h0[k] = *reinterpret_cast<const float4*>(sv.h0 + row);
        p.h1[k] = *reinterpret_cast<const float4*>(sv.h1 + row);
      } else {
        p.h0[k] = *reinterpret_cast<const float4*>(h_init + (int64_t)(b0 + p.r[k]) * H + p.c[k]);
        p.h1[k] = *reinterpret_cast<const float4*>(h_init + ((int64_t)B + b0 + p.r[k]) * H + p.c[k]);
      }
    }
  }
}
// launch 0: the state in front of step 0 = encoder_hidden[:2]; xh1n != NULL: also the tile the attention of step 0 scores
__device__ __forceinline__ void ct_fwd_init_state(const CtRowPf& p, const g2v_code_dec_saved& sv, int B, int H, int b0, float* xh1n,
                                                  int ldh) {
#pragma unroll
  for (int k = 0; k < CT_NPF; ++k)
    if (p.v[k]) {
      *reinterpret_cast<float4*>(sv.h0 + (int64_t)(b0 + p.r[k]) * H + p.c[k]) = p.h0[k];
      *reinterpret_cast<float4*>(sv.h1 + (int64_t)(b0 + p.r[k]) * H + p.c[k]) = p.h1[k];
      if (xh1n) *reinterpret_cast<float4*>(xh1n + p.r[k] * ldh + p.c[k]) = p.h1[k];
    }
}
// BatchNorm statistics of u_t from the per-workgroup partials of the previous launch (batch statistics) -> st = mean[Hp], invstd[Hp];
// workgroup 0 leaves them in bn_stats and, where the caller gave them, updates the running statistics (momentum 0.1, unbiased
// variance; one update per decode step, in step order = stream order; bn_running_mean == NULL: the caller commits them behind the
// backward, g2v_bn_running_update_invstd).  GUARD_B1: one row has variance 0 exactly (bn_batch_var).  CENTER1 (with
// ct_pre_linear_partials<true>): where ONE row tile holds the whole batch its second sum is taken about the tile's own mean.
template <bool GUARD_B1, bool CENTER1 = false>
__device__ __forceinline__ void ct_bn_finish_fwd(const g2v_code_dec_weights& w, const g2v_code_dec_saved& sv, const CodeDims& dm, int t,
                                                 float* st, float* red, float* red_scratch, int tid) {
  const int B = dm.B, H = dm.H, Hp = (H + 15) & ~15;
  const float* part = sv.bn_partial + (int64_t)(t & 1) * dm.nblk * 2 * H;
  reduce_partials<CT_NTHR>(part, dm.nblk, 2 * H, red, red_scratch, tid, dm.scratch);
  for (int f = tid; f < H; f += CT_NTHR) {
    const float s1 = red[f], s2 = red[H + f];
    const float mv = s1 / (float)B;
    const float var = (CENTER1 && dm.nblk == 1) ? s2 / (float)B                                   // biased batch variance
                      : GUARD_B1 ? bn_batch_var(s2, mv, B) : fmaxf(s2 / (float)B - mv * mv, 0.f);
    const float mean = mv + w.b_pre[f];
    const float invstd = bn_invstd_(var);
    st[f] = mean;
    st[Hp + f] = invstd;
    if (blockIdx.x == 0) {
      sv.bn_stats[(int64_t)t * 2 * H + f] = mean;
      sv.bn_stats[(int64_t)t * 2 * H + H + f] = invstd;
      if (w.bn_running_mean) {
        const float unb = (B > 1) ? var * (float)B / (float)(B - 1) : var;
        w.bn_running_mean[f] = 0.9f * w.bn_running_mean[f] + 0.1f * mean;
        w.bn_running_var[f] = 0.9f * w.bn_running_var[f] + 0.1f * unb;
      }
    }
  }
}
// a_t = ReLU(BN(u_t)); stage the previous hidden states
__device__ __forceinline__ void ct_bn_relu_stage(const CtRowPf& p, const g2v_code_dec_weights& w, const g2v_code_dec_saved& sv,
                                                 const float* st, float* Xa, float* Xh0, float* Xh1, int ldh, int t, int B, int H,
                                                 int b0) {
  const int Hp = (H + 15) & ~15;
#pragma unroll
  for (int k = 0; k < CT_NPF; ++k)
    if (p.v[k]) {
      const int c = p.c[k];
      const float4 g4 = *reinterpret_cast<const float4*>(w.bn_w + c), b4 = *reinterpret_cast<const float4*>(w.bn_b + c);
      const float4 m4 = *reinterpret_cast<const float4*>(st + c), i4 = *reinterpret_cast<const float4*>(st + Hp + c);
      float4 a4;
      a4.x = fmaxf((p.u[k].x - m4.x) * i4.x * g4.x + b4.x, 0.f);
      a4.y = fmaxf((p.u[k].y - m4.y) * i4.y * g4.y + b4.y, 0.f);
      a4.z = fmaxf((p.u[k].z - m4.z) * i4.z * g4.z + b4.z, 0.f);
      a4.w = fmaxf((p.u[k].w - m4.w) * i4.w * g4.w + b4.w, 0.f);
      *reinterpret_cast<float4*>(Xa + p.r[k] * ldh + c) = a4;
      *reinterpret_cast<float4*>(Xh0 + p.r[k] * ldh + c) = p.h0[k];
      *reinterpret_cast<float4*>(Xh1 + p.r[k] * ldh + c) = p.h1[k];
      if (sv.a) *reinterpret_cast<float4*>(sv.a + ((int64_t)t * B + b0 + p.r[k]) * H + c) = a4;
    }
}
// GRU layer 0 (inter-layer dropout on its output), barrier, GRU layer 1, barrier: h1_{t+1} is left in Xh1n
__device__ __forceinline__ void ct_cells_fwd(const CodePackF& pk, const g2v_code_dec_weights& w, const g2v_code_dec_saved& sv,
                                             const uint8_t* __restrict__ keep_l0, bool drop, const CodeDims& dm, int t, int b0, int nrows,
                                             float* Xa, float* Xh0, float* Xh1, float* Xx1, float* Xh1n, int lane, int wave) {
  const int B = dm.B, H = dm.H, Hp = (H + 15) & ~15, ldh = Hp + 4;
  gru_cell_fwd<0>(pk.ih0, pk.hh0, w.b_ih0, w.b_hh0, Xa, Xh0, ldh, H, Hp, Xx1, sv.h0 + ((int64_t)(t + 1) * B + b0) * H,
                  sv.gates0 ? sv.gates0 + ((int64_t)t * B + b0) * 4 * H : nullptr,
                  drop ? keep_l0 + ((int64_t)t * B + b0) * H : nullptr, 1.0f / (1.0f - dm.p_drop),
                  (drop && sv.x1) ? sv.x1 + ((int64_t)t * B + b0) * H : nullptr, nrows, lane, wave, CT_NW);
  lds_barrier();
  gru_cell_fwd<0>(pk.ih1, pk.hh1, w.b_ih1, w.b_hh1, Xx1, Xh1, ldh, H, Hp, Xh1n, sv.h1 + ((int64_t)(t + 1) * B + b0) * H,
                  sv.gates1 ? sv.gates1 + ((int64_t)t * B + b0) * 4 * H : nullptr, nullptr, 1.0f, nullptr, nrows, lane, wave,
                  CT_NW);
  lds_barrier();
}
// y_t = out(h1_{t+1}) of a continuous decoder (width E) -> y_row0 (this tile's row 0 of outputs[t + 1], row stride E); fed back:
// also the x tile of the next step (Xe, zero rows past nrows) and its saved row (ec_row0, row stride ldec).  E % 4 == 0: a lane's
// group of four outputs is whole or padding and moves as one float4; else the rows are not 16-byte aligned and move element-wise.
__device__ __forceinline__ void ct_out_feed_fwd(const float* __restrict__ pk_out, const float* __restrict__ b_out, const float* Xh1n,
                                                int ldh, int Hp, int E, float* __restrict__ y_row0, bool feed, float* Xe, int ldx,
                                                float* __restrict__ ec_row0, int64_t ldec, int nrows, int lane, int wave) {
  const int i = lane & 15, q = lane >> 4;
  const int ntile = (E + 15) >> 4;
  const bool vec = (E & 3) == 0 && (ldec & 3) == 0;
  for (int base = 0; base < ntile; base += 4 * CT_NW) {
    f32x4 acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
    wave_gemm_p<4, 0>(acc, pk_out, Hp >> 4, base + wave, CT_NW, Xh1n, ldh, lane);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k0 = 16 * (base + wave + CT_NW * u) + 4 * q;
      if (vec) {
        if (k0 + 3 < E) {
          const float4 bo = *reinterpret_cast<const float4*>(b_out + k0);
          const float4 v = make_float4(acc[u][0] + bo.x, acc[u][1] + bo.y, acc[u][2] + bo.z, acc[u][3] + bo.w);
          if (i < nrows) *reinterpret_cast<float4*>(y_row0 + (int64_t)i * E + k0) = v;
          if (feed) {
            *reinterpret_cast<float4*>(Xe + i * ldx + k0) = (i < nrows) ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < nrows) *reinterpret_cast<float4*>(ec_row0 + (int64_t)i * ldec + k0) = v;
          }
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = k0 + r;
          if (k >= E) continue;
          const float v = acc[u][r] + b_out[k];
          if (i < nrows) y_row0[(int64_t)i * E + k] = v;
          if (feed) {
            Xe[i * ldx + k] = (i < nrows) ? v : 0.f;
            if (i < nrows) ec_row0[(int64_t)i * ldec + k] = v;
          }
        }
      }
    }
  }
}
// Bahdanau attention on h1_j (in Xh1n): hp = h1_j W_attn[:, :H]^T + b_attn -> Xhp (saved in sv.hp), energies and softmax over ALL Tw
// positions (the reference does not mask padded positions) -> sc (saved in sv.attw), context -> xc (LDS, row stride ldx) and
// ec_ctx (this tile's row 0, row stride ldec; ec_vec: the rows are 16-byte aligned).  enc / ep (Tw,B,H) are streamed from global
// memory.  Begins and ends without a barrier of its own on the caller's tiles: the caller's barrier follows.
__device__ __forceinline__ void ct_attn_head_fwd(const float* __restrict__ pk_attn_h, const g2v_code_dec_weights& w,
                                                 const g2v_code_dec_saved& sv, const float* __restrict__ enc, const float* __restrict__ ep,
                                                 const float* Xh1n, float* Xhp, float* sc, float* xc, int ldx, float* __restrict__ ec_ctx,
                                                 int64_t ldec, bool ec_vec, const CtRowPf& p, const CodeDims& dm, int j, int b0, int nrows,
                                                 int tid) {
  const int B = dm.B, H = dm.H, Tw = dm.Tw, Hp = (H + 15) & ~15, ldh = Hp + 4;
  const int lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
  const int ntile = Hp >> 4;
  lds_barrier();                     // (the readers of Xhp's former contents are long past; the caller's writes above)
  for (int ft = wave; ft < ntile; ft += CT_NW) {
    const int f0 = 16 * ft + 4 * q;
    f32x4 acc[1] = {(f32x4){0.f, 0.f, 0.f, 0.f}};
    wave_gemm_p<1, 0>(acc, pk_attn_h, Hp >> 4, ft, 0, Xh1n, ldh, lane);
    if (f0 + 3 < H) {
      const float4 ba = *reinterpret_cast<const float4*>(w.b_attn + f0);
      const float4 h4 = make_float4(acc[0][0] + ba.x, acc[0][1] + ba.y, acc[0][2] + ba.z, acc[0][3] + ba.w);
      *reinterpret_cast<float4*>(Xhp + i * ldh + f0) = h4;
      if (i < nrows && sv.hp) *reinterpret_cast<float4*>(sv.hp + ((int64_t)j * B + b0 + i) * H + f0) = h4;
    }
  }
  lds_barrier();
  // scores: one thread per (row, position); 16 x Tw <= 1024 pairs
  for (int pp = tid; pp < 16 * Tw; pp += CT_NTHR) {
    const int r = pp / Tw, tw = pp - r * Tw;
    float e = 0.f;
    if (r < nrows) {
      const float* epr = ep + ((int64_t)tw * B + b0 + r) * H;
      const float* hpr = Xhp + r * ldh;
      float e0 = 0.f, e1 = 0.f, e2 = 0.f, e3 = 0.f;
      for (int c = 0; c < H; c += 4) {
        const float4 p4 = *reinterpret_cast<const float4*>(epr + c), h4 = *reinterpret_cast<const float4*>(hpr + c);
        const float4 v4 = *reinterpret_cast<const float4*>(w.v_attn + c);
        e0 += v4.x * tanhf_(h4.x + p4.x);
        e1 += v4.y * tanhf_(h4.y + p4.y);
        e2 += v4.z * tanhf_(h4.z + p4.z);
        e3 += v4.w * tanhf_(h4.w + p4.w);
      }
      e = (e0 + e1) + (e2 + e3);
    }
    sc[r * Tw + tw] = e;
  }
  lds_barrier();
  if (tid < 16 && tid < nrows) {
    float mx = -INFINITY;
    for (int tw = 0; tw < Tw; ++tw) mx = fmaxf(mx, sc[tid * Tw + tw]);
    float sum = 0.f;
    for (int tw = 0; tw < Tw; ++tw) sum += expf(sc[tid * Tw + tw] - mx);
    const float inv = 1.0f / sum;
    for (int tw = 0; tw < Tw; ++tw) {
      const float ww = expf(sc[tid * Tw + tw] - mx) * inv;
      sc[tid * Tw + tw] = ww;
      if (sv.attw) sv.attw[((int64_t)j * B + b0 + tid) * Tw + tw] = ww;
    }
  }
  lds_barrier();
#pragma unroll
  for (int k = 0; k < CT_NPF; ++k)
    if (p.v[k]) {
      const int r = p.r[k], c = p.c[k];
      float4 c4 = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int tw = 0; tw < Tw; ++tw) {
        const float ww = sc[r * Tw + tw];
        const float4 n4 = *reinterpret_cast<const float4*>(enc + ((int64_t)tw * B + b0 + r) * H + c);
        c4.x += ww * n4.x; c4.y += ww * n4.y; c4.z += ww * n4.z; c4.w += ww * n4.w;
      }
      *reinterpret_cast<float4*>(xc + r * ldx + c) = c4;
      float* o = ec_ctx + (int64_t)r * ldec + c;
      if (ec_vec) {
        *reinterpret_cast<float4*>(o) = c4;
      } else {
        o[0] = c4.x; o[1] = c4.y; o[2] = c4.z; o[3] = c4.w;
      }
    }
}
// u_j = pre_linear.0(x_j) and the per-workgroup BatchNorm partial sums of (u - b).  The input tile is X1 (KS1 k-steps of `pre`)
// and, with pre2 != NULL, a second column block X2 (KS2 k-steps of `pre2`) accumulated into the same product.
// CENTER1: where one row tile holds the whole batch (nblk == 1) the second sum is sum (c - mean)^2 about the tile's own mean instead
// of sum c^2: two passes over values that sit in registers anyway.  A small batch needs it -- at B = 2 a feature on which the two
// rows nearly agree has var << mean^2, and sum c^2 / B - mean^2 lost 1e-4 of 1 / sqrt(var + eps) there.
template <bool CENTER1 = false>
__device__ __forceinline__ void ct_pre_linear_partials(const float* __restrict__ pre, int KS1, const float* X1,
                                                       const float* __restrict__ pre2, int KS2, const float* X2, int ldx,
                                                       const g2v_code_dec_weights& w, const g2v_code_dec_saved& sv, const CodeDims& dm,
                                                       int j, int b0, int nrows, int lane, int wave) {
  const int B = dm.B, H = dm.H, Hp = (H + 15) & ~15;
  const int i = lane & 15, q = lane >> 4;
  const int ntile = Hp >> 4;
  float* part = sv.bn_partial + ((int64_t)(j & 1) * dm.nblk + blockIdx.x) * 2 * H;
  for (int ft = wave; ft < ntile; ft += CT_NW) {
    const int f0 = 16 * ft + 4 * q;
    const bool vec = f0 + 3 < H;       // (H % 4 == 0: a lane's group of four features is whole or padding)
    float4 bp = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vec) bp = *reinterpret_cast<const float4*>(w.b_pre + f0);
    f32x4 acc[1] = {(f32x4){0.f, 0.f, 0.f, 0.f}};
    wave_gemm_p<1, 0>(acc, pre, KS1, ft, 0, X1, ldx, lane);      // (every lane of the wave: an MFMA is not predicated)
    if (pre2) wave_gemm_p<1, 0>(acc, pre2, KS2, ft, 0, X2, ldx, lane);
    if (!vec) continue;               // (uniform per DPP row of 16 lanes: the reductions below stay whole)
    float s1[4], s2[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = (i < nrows) ? acc[0][r] : 0.f;
      s1[r] = reduce16(v);
      if (CENTER1 && dm.nblk == 1) {
        const float d = (i < nrows) ? v - s1[r] / (float)nrows : 0.f;
        s2[r] = reduce16(d * d);
      } else {
        s2[r] = reduce16(v * v);
      }
    }
    if (i < nrows)
      *reinterpret_cast<float4*>(sv.u + ((int64_t)j * B + b0 + i) * H + f0) =
          make_float4(acc[0][0] + bp.x, acc[0][1] + bp.y, acc[0][2] + bp.z, acc[0][3] + bp.w);
    if (i == 0) {
      *reinterpret_cast<float4*>(part + f0) = make_float4(s1[0], s1[1], s1[2], s1[3]);
      *reinterpret_cast<float4*>(part + H + f0) = make_float4(s2[0], s2[1], s2[2], s2[3]);
    }
  }
}

// =====================================================================================================================
// backward
// =====================================================================================================================
struct CodeBwdArgs {
  const float* d_logits;     // (S1,B,K)
  const float* enc; const float* ep;
  g2v_code_dec_weights w;
  CodePackB tw;
  g2v_code_dec_saved sv;
  const uint8_t* keep_l0;
  float* dgi0; float* dgh0; float* dgi1; float* dgh1;     // (S1,B,3H)
  float* dbn;                // (S1,B,H)   d loss / d BN output (behind the ReLU mask)
  float* du;                 // (S1,B,H)
  float* dec;                // (S1,B,H)   d loss / d e_t (the embedding half of d x_t)
  float* dhp;                // (S1,B,H)   attention: d loss / d hp_t
  float* d_ep; float* d_enc; // (Tw,B,H)   attention: accumulated over the steps by the owning workgroup
  float* dv_partial;         // (nblk,H)   attention: per-workgroup sums of d v, accumulated over the steps
  float* bn_part;            // (S1,nblk,2,H) per-workgroup sums of BN backward, one slot per step
  float* bn_sums;            // (S1,2,H)
  float* d_hidden0;          // (2,B,H)
};

// LDS carve of the backward kernels (floats).  H = 200, K = 512: 152 KB of the CU's 160 -- the d logits tile [16][K] doubles as
// the layer-0 incoming gradient tile (written after the out-layer product has consumed it), and the attention phase (Part A of
// code_step_bwd_att_kernel, in front of the cells) borrows the gate tiles: nothing of its own.
struct CtBwdLds {
  int xdl, gi, gh, dd, c0, c1, total;
};
static __host__ __device__ inline CtBwdLds ct_bwd_lds(int H, int K) {
  const int Hp = (H + 15) & ~15, ldh = Hp + 4, Gp = (3 * H + 15) & ~15, ldg = Gp + 4, Kp = (K + 15) & ~15, ldk = Kp + 4;
  CtBwdLds l;
  int o = 0;
  l.xdl = o; o += 16 * (ldk > 2 * ldh ? ldk : 2 * ldh);   // d logits tile; then Xdx [16][ldh]; attention: du | d ctx tiles
  l.gi = o; o += 16 * ldg;                                // attention: d hp tile
  l.gh = o; o += 16 * ldg;                                // attention: BatchNorm sums + reduction scratch, then the d v rows
  l.dd = o; o += 16 * ldh;                                // attention: d_w / ds and the attention weights [2][16][Tw]
  l.c0 = o; o += 16 * ldh;
  l.c1 = o; o += 16 * ldh;
  l.total = o;
  return l;
}

// One step of the BPTT for this workgroup's 16 rows.  dh1 arrives as dlogits_t W_out (+ the carry in C1), the carries C0 / C1
// (LDS, [16][ldh]) hold d loss / d h0_t, d h1_t on exit.  Leaves dbn_t in global memory and this workgroup's BN-backward sums.
// FB (t2e_latent.hip: the decoder that feeds its OUTPUT back with the gradient attached): with `fb_add` the tile already holds the
// feedback term du_{t+1} W_pre of these rows and the loss's own gradient is added to it; the sum, d loss / d y_t, is also left in
// `dy_out` (S1,B,K) for the out layer's weight gradient.
template <bool FB = false>
__device__ __forceinline__ void code_bwd_cells(const CodeBwdArgs& a, const CodeDims& dm, const CtBwdLds& L, float* smem, int t,
                                               int b0, int nrows, int tid, bool first, bool fb_add = false,
                                               float* __restrict__ dy_out = nullptr) {
  constexpr int NTHR = CT_NTHR, NW = CT_NW;
  const int B = dm.B, H = dm.H, K = dm.K, G = 3 * H;
  const int Hp = (H + 15) & ~15, ldh = Hp + 4, Gp = (G + 15) & ~15, ldg = Gp + 4, Kp = (K + 15) & ~15, ldk = Kp + 4;
  float* Xdl = smem + L.xdl;
  float* Gi = smem + L.gi;
  float* Gh = smem + L.gh;
  float* Dd = smem + L.dd;
  float* Xdx = smem + L.xdl;      // (the d logits tile is dead once cell 1's products have read it: barrier in between)
  float* C0 = smem + L.c0;
  float* C1 = smem + L.c1;
  const int lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int nth = Hp >> 4;
  constexpr int MAXT = 2;                 // H <= 256: at most two feature tiles per wave
  // cell 1's saved inputs and its carry (LDS: final since the previous step's last barrier), requested before the d logits tile
  // (vector-memory results return in order)
  CellBwdIn cin1[MAXT];
#pragma unroll
  for (int m = 0; m < MAXT; ++m)
    if (wave + NW * m < nth)
      cell_bwd_prefetch(cin1[m], first ? nullptr : C1, nullptr, a.sv.gates1 + ((int64_t)t * B + b0) * 4 * H,
                        a.sv.h1 + ((int64_t)t * B + b0) * H, H, wave + NW * m, nrows, lane, ldh);
  // d logits tile of step t: 16 rows x K, 16-byte vectors
  // (padding columns and rows rewritten every step: the region doubles as the Xdx tile, below)
  if (FB && (K & 3)) {
    // (a width that is no multiple of 4: the rows of d_logits / dy_out are not 16-byte aligned and move element-wise)
    for (int e = tid; e < 16 * Kp; e += NTHR) {
      const int r = e / Kp, c = e - r * Kp;
      const bool ok = r < nrows && c < K;
      float v = ok ? a.d_logits[((int64_t)t * B + b0 + r) * K + c] : 0.f;
      if (fb_add) v += Xdl[r * ldk + c];
      if (ok) dy_out[((int64_t)t * B + b0 + r) * K + c] = v;
      Xdl[r * ldk + c] = v;
    }
  } else {
    const int K4 = Kp >> 2;
    for (int e = tid; e < 16 * K4; e += NTHR) {
      const int r = e / K4, c = (e - r * K4) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < nrows && c < K) v = *reinterpret_cast<const float4*>(a.d_logits + ((int64_t)t * B + b0 + r) * K + c);
      if constexpr (FB) {
        if (fb_add) {
          const float4 f = *reinterpret_cast<const float4*>(Xdl + r * ldk + c);
          v.x += f.x; v.y += f.y; v.z += f.z; v.w += f.w;
        }
        if (r < nrows && c < K) *reinterpret_cast<float4*>(dy_out + ((int64_t)t * B + b0 + r) * K + c) = v;
      }
      *reinterpret_cast<float4*>(Xdl + r * ldk + c) = v;
    }
  }
  CellBwdIn cin0[MAXT];
  const bool drop = a.keep_l0 && dm.p_drop > 0.f;
#pragma unroll
  for (int m = 0; m < MAXT; ++m)
    if (wave + NW * m < nth)
      cell_bwd_prefetch(cin0[m], first ? nullptr : C0, drop ? a.keep_l0 + ((int64_t)t * B + b0) * H : nullptr,
                        a.sv.gates0 + ((int64_t)t * B + b0) * 4 * H, a.sv.h0 + ((int64_t)t * B + b0) * H, H, wave + NW * m,
                        nrows, lane, ldh);
  lds_barrier();
  // ---- dh1 = carry1 + dlogits W_out ; GRU cell 1 backward ---------------------------------------------------------------
#pragma unroll
  for (int m = 0; m < MAXT; ++m) {
    const int ft = wave + NW * m;
    if (ft < nth) {
      f32x4 acc[1] = {(f32x4){0.f, 0.f, 0.f, 0.f}};
      wave_gemm_p<1, 0>(acc, a.tw.out_t, Kp >> 4, ft, 0, Xdl, ldk, lane);
      gru_cell_bwd_tile(acc[0], first ? nullptr : C1, 1.0f, nullptr, a.sv.gates1 + ((int64_t)t * B + b0) * 4 * H,
                        a.sv.h1 + ((int64_t)t * B + b0) * H, a.dgi1 + ((int64_t)t * B + b0) * G, a.dgh1 + ((int64_t)t * B + b0) * G,
                        Gi, Gh, ldg, Dd, ldh, H, ft, nrows, lane, false, true, cin1[m], ldh);
    }
  }
  lds_barrier();
  // ---- carry1' = dh1 * z + dgh1 W_hh1 ;  dx1 = dgi1 W_ih1 -> dh0 ---------------------------------------------------------
  for (int ft = wave; ft < nth; ft += NW) {
    f32x4 a1[1] = {(f32x4){0.f, 0.f, 0.f, 0.f}}, a2[1] = {(f32x4){0.f, 0.f, 0.f, 0.f}};
    wave_gemm_p_dual<1, 8>(a1, a.tw.hh1_t, Gh, a2, a.tw.ih1_t, Gi, Gp >> 4, ft, 0, ldg, lane);
    const int f0 = 16 * ft + 4 * q;
    if (f0 + 3 < H) {
      const float4 d4 = *reinterpret_cast<const float4*>(Dd + i * ldh + f0);
      *reinterpret_cast<float4*>(C1 + i * ldh + f0) = make_float4(d4.x + a1[0][0], d4.y + a1[0][1], d4.z + a1[0][2], d4.w + a1[0][3]);
      *reinterpret_cast<float4*>(Xdx + i * ldh + f0) = make_float4(a2[0][0], a2[0][1], a2[0][2], a2[0][3]);
    }
  }
  lds_barrier();
  // ---- GRU cell 0 backward (Gi / Gh / Dd are reused) ----------------------------------------------------------------------
#pragma unroll
  for (int m = 0; m < MAXT; ++m) {
    const int ft = wave + NW * m;
    if (ft < nth) {
      const int f0 = 16 * ft + 4 * q;
      f32x4 acc;
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = (f0 + r < H) ? Xdx[i * ldh + f0 + r] : 0.f;
      gru_cell_bwd_tile(acc, first ? nullptr : C0, 1.0f / (1.0f - dm.p_drop), drop ? a.keep_l0 + ((int64_t)t * B + b0) * H : nullptr,
                        a.sv.gates0 + ((int64_t)t * B + b0) * 4 * H, a.sv.h0 + ((int64_t)t * B + b0) * H,
                        a.dgi0 + ((int64_t)t * B + b0) * G, a.dgh0 + ((int64_t)t * B + b0) * G, Gi, Gh, ldg, Dd, ldh, H, ft, nrows,
                        lane, false, true, cin0[m], ldh);
    }
  }
  lds_barrier();
  // ---- carry0' = dh0 * z + dgh0 W_hh0 ;  da = dgi0 W_ih0 -> ReLU backward -> dbn_t + BN-backward partial sums --------------
  {
    const float* stats = a.sv.bn_stats + (int64_t)t * 2 * H;
    float* part = a.bn_part + ((int64_t)t * dm.nblk + blockIdx.x) * 2 * H;
    for (int ft = wave; ft < nth; ft += NW) {
      const int f0 = 16 * ft + 4 * q;
      const bool vec = f0 + 3 < H;
      float av[4] = {0.f, 0.f, 0.f, 0.f}, uv[4] = {0.f, 0.f, 0.f, 0.f}, mv[4] = {0.f, 0.f, 0.f, 0.f}, iv[4] = {0.f, 0.f, 0.f, 0.f};
      if (vec) {
        const float4 m4 = *reinterpret_cast<const float4*>(stats + f0), i4 = *reinterpret_cast<const float4*>(stats + H + f0);
        mv[0] = m4.x; mv[1] = m4.y; mv[2] = m4.z; mv[3] = m4.w;
        iv[0] = i4.x; iv[1] = i4.y; iv[2] = i4.z; iv[3] = i4.w;
        if (i < nrows) {
          const int64_t row = ((int64_t)t * B + b0 + i) * H + f0;
          const float4 a4 = *reinterpret_cast<const float4*>(a.sv.a + row), u4 = *reinterpret_cast<const float4*>(a.sv.u + row);
          av[0] = a4.x; av[1] = a4.y; av[2] = a4.z; av[3] = a4.w;
          uv[0] = u4.x; uv[1] = u4.y; uv[2] = u4.z; uv[3] = u4.w;
        }
      }
      f32x4 a1[1] = {(f32x4){0.f, 0.f, 0.f, 0.f}}, a2[1] = {(f32x4){0.f, 0.f, 0.f, 0.f}};
      wave_gemm_p_dual<1, 8>(a1, a.tw.hh0_t, Gh, a2, a.tw.ih0_t, Gi, Gp >> 4, ft, 0, ldg, lane);
      if (!vec) continue;
      float dbn[4], s1[4], s2[4], cw[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = i < nrows;
        cw[r] = Dd[i * ldh + f0 + r] + a1[0][r];
        dbn[r] = (ok && av[r] > 0.f) ? a2[0][r] : 0.f;
        const float dbx = ok ? dbn[r] * ((uv[r] - mv[r]) * iv[r]) : 0.f;
        s1[r] = reduce16(dbn[r]);
        s2[r] = reduce16(dbx);
      }
      *reinterpret_cast<float4*>(C0 + i * ldh + f0) = make_float4(cw[0], cw[1], cw[2], cw[3]);
      if (i < nrows)
        *reinterpret_cast<float4*>(a.dbn + ((int64_t)t * B + b0 + i) * H + f0) = make_float4(dbn[0], dbn[1], dbn[2], dbn[3]);
      if (i == 0) {
        *reinterpret_cast<float4*>(part + f0) = make_float4(s1[0], s1[1], s1[2], s1[3]);
        *reinterpret_cast<float4*>(part + H + f0) = make_float4(s2[0], s2[1], s2[2], s2[3]);
      }
    }
  }
  lds_barrier();
}

__device__ __forceinline__ void code_bwd_write_hidden0(const CodeBwdArgs& a, const CodeDims& dm, const CtBwdLds& L, float* smem,
                                                       int b0, int nrows, int tid) {
  const int B = dm.B, H = dm.H, Hp = (H + 15) & ~15, ldh = Hp + 4, H4 = H >> 2;
  const float* C0 = smem + L.c0;
  const float* C1 = smem + L.c1;
  for (int e = tid; e < 16 * H4; e += CT_NTHR) {
    const int r = e / H4, c = (e - r * H4) * 4;
    if (r >= nrows) continue;
    *reinterpret_cast<float4*>(a.d_hidden0 + (int64_t)(b0 + r) * H + c) = *reinterpret_cast<const float4*>(C0 + r * ldh + c);
    *reinterpret_cast<float4*>(a.d_hidden0 + ((int64_t)B + b0 + r) * H + c) = *reinterpret_cast<const float4*>(C1 + r * ldh + c);
  }
}

// ---- Part A of the per-step backward launches (t2e_rollout.hip with attention, t2e_latent.hip, pose_attn.hip) -----------------
// carries of the step behind this one (written by the previous launch)
__device__ __forceinline__ void ct_bwd_load_carries(const CodeBwdArgs& a, const CodeDims& dm, float* C0, float* C1, int b0, int nrows,
                                                    int tid) {
  const int B = dm.B, H = dm.H, Hp = (H + 15) & ~15, ldh = Hp + 4, H4 = H >> 2;
  for (int e = tid; e < 16 * H4; e += CT_NTHR) {
    const int r = e / H4, c = (e - r * H4) * 4;
    if (r >= nrows) continue;
    *reinterpret_cast<float4*>(C0 + r * ldh + c) = *reinterpret_cast<const float4*>(a.d_hidden0 + (int64_t)(b0 + r) * H + c);
    *reinterpret_cast<float4*>(C1 + r * ldh + c) = *reinterpret_cast<const float4*>(a.d_hidden0 + ((int64_t)B + b0 + r) * H + c);
  }
}
// BatchNorm backward of step s, finished from the per-workgroup partials of the launch before: the sums -> red[2H] (workgroup 0
// leaves them in bn_sums for d bn_w / d bn_b), du_s of this tile's rows -> a.du and the LDS tile Xdu [16][ldh].
// CENTER1: where one row tile holds the whole batch (nblk == 1) du is re-centred about its own column mean, as the forward's second
// sum is (ct_pre_linear_partials<true>).  The columns of du sum to zero exactly; in float32 the fused formula leaves a residue of
// g invstd^2 m2 sum(u - mean), and at a small batch, where a feature's variance can be tiny against its mean^2, invstd^2 reaches
// 1e5: at B = 2 the residue stood at 1e-6 of the weight gradient's largest entry in d b_pre, which is that column sum.
template <bool CENTER1 = false>
__device__ __forceinline__ void ct_bn_bwd_finish(const CodeBwdArgs& a, const CodeDims& dm, int s, float* red, float* red_scratch,
                                                 float* Xdu, int b0, int nrows, int tid) {
  const int B = dm.B, H = dm.H, Hp = (H + 15) & ~15, ldh = Hp + 4, H4 = H >> 2;
  reduce_partials<CT_NTHR>(a.bn_part + (int64_t)s * dm.nblk * 2 * H, dm.nblk, 2 * H, red, red_scratch, tid, dm.scratch);
  if (blockIdx.x == 0)
    for (int f = tid; f < 2 * H; f += CT_NTHR) a.bn_sums[(int64_t)s * 2 * H + f] = red[f];
  const float invB = 1.0f / (float)B;
  const float* stats = a.sv.bn_stats + (int64_t)s * 2 * H;
  for (int e = tid; e < 16 * H4; e += CT_NTHR) {
    const int r = e / H4, c = (e - r * H4) * 4;
    if (r >= nrows) continue;
    const int64_t row = ((int64_t)s * B + b0 + r) * H + c;
    const float4 u4 = *reinterpret_cast<const float4*>(a.sv.u + row), d4 = *reinterpret_cast<const float4*>(a.dbn + row);
    const float4 m4 = *reinterpret_cast<const float4*>(stats + c), i4 = *reinterpret_cast<const float4*>(stats + H + c);
    const float4 g4 = *reinterpret_cast<const float4*>(a.w.bn_w + c);
    const float uu[4] = {u4.x, u4.y, u4.z, u4.w}, db[4] = {d4.x, d4.y, d4.z, d4.w}, mm[4] = {m4.x, m4.y, m4.z, m4.w},
                ii[4] = {i4.x, i4.y, i4.z, i4.w}, gg[4] = {g4.x, g4.y, g4.z, g4.w};
    float du[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float xhat = (uu[k] - mm[k]) * ii[k];
      du[k] = gg[k] * ii[k] * (db[k] - red[c + k] * invB - xhat * red[H + c + k] * invB);
    }
    const float4 du4 = make_float4(du[0], du[1], du[2], du[3]);
    if (!(CENTER1 && dm.nblk == 1)) *reinterpret_cast<float4*>(a.du + row) = du4;
    *reinterpret_cast<float4*>(Xdu + r * ldh + c) = du4;
  }
  if (CENTER1 && dm.nblk == 1) {      // (uniform over the workgroup: every thread meets the barriers)
    lds_barrier();                    // the sums in `red` are consumed: its first H floats take the column means
    for (int f = tid; f < H; f += CT_NTHR) {
      float sum = 0.f;
      for (int r = 0; r < nrows; ++r) sum += Xdu[r * ldh + f];
      red[f] = sum / (float)nrows;
    }
    lds_barrier();
    for (int e = tid; e < 16 * H4; e += CT_NTHR) {
      const int r = e / H4, c = (e - r * H4) * 4;
      if (r >= nrows) continue;
      float4 d4 = *reinterpret_cast<const float4*>(Xdu + r * ldh + c);
      const float4 m4 = *reinterpret_cast<const float4*>(red + c);
      d4.x -= m4.x; d4.y -= m4.y; d4.z -= m4.z; d4.w -= m4.w;
      *reinterpret_cast<float4*>(Xdu + r * ldh + c) = d4;
      *reinterpret_cast<float4*>(a.du + ((int64_t)s * B + b0 + r) * H + c) = d4;
    }
  }
}
// Attention backward of step s for this tile's rows, from d ctx_s in Xdc [16][ldh] (final since the caller's last barrier):
// d_w = <d ctx, enc>, softmax backward, then per (row, feature group) d hp_s (-> a.dhp and the LDS tile Xdhp), the d v rows (-> dvp
// [16][ldh], summed into this workgroup's a.dv_partial) and the d_ep / d_enc rows, accumulated over the steps in place by this
// workgroup alone (the first step written, s == S1-1, overwrites); finally carry1 += d hp W_attn[:, :H] (the state the attention of
// step s scored is the output of step s-1).  dsc / wsc: [16][Tw] each.  Ends with a barrier.
__device__ __forceinline__ void ct_attn_bwd_step(const CodeBwdArgs& a, const CodeDims& dm, int s, const float* Xdc, float* Xdhp,
                                                 float* dsc, float* wsc, float* dvp, float* C1, int b0, int nrows, int tid) {
  const int S1 = dm.S1, B = dm.B, H = dm.H, Tw = dm.Tw, Hp = (H + 15) & ~15, ldh = Hp + 4, H4 = H >> 2;
  const int lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
  // attention weights of step s;  d_w[r][tw] = <d ctx[r], enc[tw, r]>
  for (int p = tid; p < 16 * Tw; p += CT_NTHR) {
    const int r = p / Tw, tw = p - r * Tw;
    wsc[p] = (r < nrows) ? a.sv.attw[((int64_t)s * B + b0 + r) * Tw + tw] : 0.f;
    float e = 0.f;
    if (r < nrows) {
      const float* er = a.enc + ((int64_t)tw * B + b0 + r) * H;
      const float* dc = Xdc + r * ldh;
      float e0 = 0.f, e1 = 0.f, e2 = 0.f, e3 = 0.f;
      for (int c = 0; c < H; c += 4) {
        const float4 n4 = *reinterpret_cast<const float4*>(er + c), d4 = *reinterpret_cast<const float4*>(dc + c);
        e0 += d4.x * n4.x; e1 += d4.y * n4.y; e2 += d4.z * n4.z; e3 += d4.w * n4.w;
      }
      e = (e0 + e1) + (e2 + e3);
    }
    dsc[p] = e;
  }
  lds_barrier();
  if (tid < 16) {     // softmax backward: ds = w (d_w - <w, d_w>)
    float dot = 0.f;
    for (int tw = 0; tw < Tw; ++tw) dot += wsc[tid * Tw + tw] * dsc[tid * Tw + tw];
    for (int tw = 0; tw < Tw; ++tw) dsc[tid * Tw + tw] = wsc[tid * Tw + tw] * (dsc[tid * Tw + tw] - dot);
  }
  lds_barrier();
  // per (row, feature group): d hp, d v partial, d_ep / d_enc rows (accumulated over the steps by this workgroup alone)
  const bool acc_steps = (s != S1 - 1);
  for (int e = tid; e < 16 * H4; e += CT_NTHR) {
    const int r = e / H4, c = (e - r * H4) * 4;
    float dh[4] = {0.f, 0.f, 0.f, 0.f}, dv[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < nrows) {
      const float4 hp4 = *reinterpret_cast<const float4*>(a.sv.hp + ((int64_t)s * B + b0 + r) * H + c);
      const float4 v4 = *reinterpret_cast<const float4*>(a.w.v_attn + c);
      const float4 dc4 = *reinterpret_cast<const float4*>(Xdc + r * ldh + c);
      const float hp[4] = {hp4.x, hp4.y, hp4.z, hp4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w}, dc[4] = {dc4.x, dc4.y, dc4.z, dc4.w};
      for (int tw = 0; tw < Tw; ++tw) {
        const int64_t row = ((int64_t)tw * B + b0 + r) * H + c;
        const float4 p4 = *reinterpret_cast<const float4*>(a.ep + row);
        const float pp[4] = {p4.x, p4.y, p4.z, p4.w};
        const float ds = dsc[r * Tw + tw], ww = wsc[r * Tw + tw];
        float de[4], dn[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float en = tanhf_(hp[k] + pp[k]);
          de[k] = ds * vv[k] * (1.0f - en * en);
          dh[k] += de[k];
          dv[k] += ds * en;
          dn[k] = ww * dc[k];
        }
        float4 o1 = make_float4(de[0], de[1], de[2], de[3]), o2 = make_float4(dn[0], dn[1], dn[2], dn[3]);
        if (acc_steps) {
          const float4 q1 = *reinterpret_cast<const float4*>(a.d_ep + row), q2 = *reinterpret_cast<const float4*>(a.d_enc + row);
          o1.x += q1.x; o1.y += q1.y; o1.z += q1.z; o1.w += q1.w;
          o2.x += q2.x; o2.y += q2.y; o2.z += q2.z; o2.w += q2.w;
        }
        *reinterpret_cast<float4*>(a.d_ep + row) = o1;
        *reinterpret_cast<float4*>(a.d_enc + row) = o2;
      }
      *reinterpret_cast<float4*>(a.dhp + ((int64_t)s * B + b0 + r) * H + c) = make_float4(dh[0], dh[1], dh[2], dh[3]);
    }
    *reinterpret_cast<float4*>(Xdhp + r * ldh + c) = make_float4(dh[0], dh[1], dh[2], dh[3]);
    *reinterpret_cast<float4*>(dvp + r * ldh + c) = make_float4(dv[0], dv[1], dv[2], dv[3]);
  }
  lds_barrier();
  for (int f = tid; f < H; f += CT_NTHR) {
    float sdv = 0.f;
    for (int r = 0; r < 16; ++r) sdv += dvp[r * ldh + f];
    float* o = a.dv_partial + (int64_t)blockIdx.x * H + f;
    *o = acc_steps ? *o + sdv : sdv;
  }
  const int nth = Hp >> 4;
  for (int ft = wave; ft < nth; ft += CT_NW) {
    const int f0 = 16 * ft + 4 * q;
    f32x4 acc[1] = {(f32x4){0.f, 0.f, 0.f, 0.f}};
    wave_gemm_p<1, 0>(acc, a.tw.attn_h_t, Hp >> 4, ft, 0, Xdhp, ldh, lane);
    if (f0 + 3 < H) {
      float4 c4 = *reinterpret_cast<const float4*>(C1 + i * ldh + f0);
      c4.x += acc[0][0]; c4.y += acc[0][1]; c4.z += acc[0][2]; c4.w += acc[0][3];
      *reinterpret_cast<float4*>(C1 + i * ldh + f0) = c4;
    }
  }
  lds_barrier();
}

// d bn_w = sum_t S2_t, d bn_b = sum_t S1_t; [attention] d v = sum over the workgroups' partials
static __global__ __launch_bounds__(256) void code_small_sums_kernel(const float* __restrict__ bn_sums, int S1, int H,
                                                              float* __restrict__ d_bn_w, float* __restrict__ d_bn_b,
                                                              const float* __restrict__ dv_partial, int nblk,
                                                              float* __restrict__ d_v) {
  for (int f = threadIdx.x; f < H; f += 256) {
    float sw = 0.f, sb = 0.f;
    for (int t = 0; t < S1; ++t) {
      sb += bn_sums[(int64_t)t * 2 * H + f];
      sw += bn_sums[(int64_t)t * 2 * H + H + f];
    }
    d_bn_w[f] = sw;
    d_bn_b[f] = sb;
    if (d_v) {
      float s = 0.f;
      for (int k = 0; k < nblk; ++k) s += dv_partial[(int64_t)k * H + f];
      d_v[f] = s;
    }
  }
}

static inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
static inline bool ct_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline int ct_scratch(size_t base_floats) { return (base_floats + 2048) * sizeof(float) <= 160 * 1024 ? 2048 : 1024; }

}  // namespace g2v
