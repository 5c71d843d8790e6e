// t2e_cells.hpp -- what the per-step kernels of the two text -> gesture decoders share: the tiling constants, the LDS carves, the
// argument blocks and the GRU cells' BPTT step of one 16-row workgroup.  t2e_rollout.hip (discrete codes, greedy feedback without
// a gradient) and t2e_latent.hip (continuous latents, the output fed back WITH its gradient) both build on it.
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
  {
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
