// vae_frame.hip -- the frame-level variational autoencoder of Part a (reference scripts/model/DAE_model.py:600-725 VAE_Network;
// train_eval/train_seq2seq.py:161-241), autoencoder_vq "False" with autoencoder_vae "True":
//     x (B,D) -> Dropout -> h = tanh(x We^T + be) -> mean = h Wm^T + bm, logvar = h Ws^T + bs -> z = mean + exp(logvar / 2) eps
//     -> c = z Wf^T + bf -> out = c Wd^T + bd;  loss = mse(out, t) + kl_weight mean(exp(logvar) - logvar - 1 + mean^2)
//
// g2v_vaeframe_step: the whole training forward AND backward of one batch as ONE workgroup of sixteen waves, on the design of
// g2v_vqframe_step (vq_frame.hip; the tile and its two stage shapes, the tile guard, the dropped-out input, the reconstruction
// epilogue, the four-lane sums and the ld() rule are frame_tile.hpp's).  Nothing is exchanged with
// another workgroup: no flag, no spin, no atomic.
//   LDS (floats; ld = frame_ld(L)): six row arrays of B ld each, every one used at least twice, and 32 floats of partial sums:
//     H    h                                    (S1; read by S2, the dWm / dWs products and the tanh backward)
//     M    mean, then dmean in place            (S2; S7)
//     V    logvar, then dlogvar in place        (S2; S7)
//     EPS  the noise                            (S0; read by S2 and S7)
//     Z    z, then dpre in place                (S2; S8)
//     C    c, then dc in place                  (S3; S5b)
//     RED  kl partials [16] | mse partials [16]
//   The five weight matrices do not fit beside them (135 KB of rows at 128 x 40): they stream from L2 as MFMA operands, as x, the
//   target and the keep mask do.  g = d loss / d out (B,D) goes through a global workspace between the product that makes it and the
//   two that contract it (one workgroup: a __syncthreads orders the stores before the loads).
//   Every matrix product is a chain of v_mfma_f32_16x16x4_f32 per 16x16 output tile, one wave per tile, k ascending; every other sum
//   (bias gradients, the kl and mse partials) has a fixed tree.  The same input gives the same bits.
//   Steps: S0 eps | S1 h | S2 mean, logvar, z, kl | S3 c | S4 out, g, mse | S5a dWd, dbd | S5b dc = g Wd | S6 dWf, dbf |
//   S7 dz = dc Wf -> dmean, dlogvar | S8 dWm, dbm, dWs, dbs; dh = [dmean | dlogvar] [Wm ; Ws] -> dpre | S9 dWe, dbe.  No dx.
//
// The staged route's operators: g2v_tanh_bwd, g2v_reparam_fwd / g2v_reparam_bwd (elementwise over any n; the KL mean by fixed-order
// partials and the one-workgroup finish of vae_noise.hpp).  The noise is vae_noise.hpp's philox_normal4, as in vae_latent.hip.
//
// g2v_vaeframe_plan: host arithmetic only -- which route serves a shape and what `auto` takes.
#include "common.hpp"
#include "frame_tile.hpp"
#include "vae_noise.hpp"

namespace g2v {
namespace {

constexpr int VAF_NW = 16;                      // waves of the training workgroup
constexpr int VAF_THREADS = 64 * VAF_NW;
constexpr size_t VAF_LDS_BYTES = 160 * 1024;
constexpr int VAF_RED = 2 * VAF_NW;

// What `auto` takes (g2v_vaeframe_plan): the fused step exactly inside the box whose corners were measured faster than the staged
// route (scripts/time_vae_frame.py: B = 16, 128 and the largest admitted batch at L = 40 and L = 45, all at D = 135);
// the staged route everywhere else, admitted or not.
constexpr int VAF_AUTO_MAX_B = 155, VAF_AUTO_MAX_D = 135, VAF_AUTO_MAX_L = 45;

struct VafLayout {
  int ldl;
  size_t h, m, v, eps, z, c, red, total;      // offsets in floats, total in floats
};
__host__ __device__ inline VafLayout vaf_layout(int B, int L) {
  VafLayout o;
  o.ldl = frame_ld(L);
  const size_t rows = (size_t)B * o.ldl;
  o.h = 0;
  o.m = o.h + rows;
  o.v = o.m + rows;
  o.eps = o.v + rows;
  o.z = o.eps + rows;
  o.c = o.z + rows;
  o.red = o.c + rows;
  o.total = o.red + VAF_RED;
  return o;
}

struct VafStepArgs {
  const float *x, *t;
  const uint8_t* keep;
  float scale;
  const float *we, *be, *wm, *bm, *ws, *bs, *wf, *bf, *wd, *bd;
  float kl_weight;
  const float* eps_in;
  uint64_t seed;
  int64_t* counter;
  float *g_we, *g_be, *g_wm, *g_bm, *g_ws, *g_bs, *g_wf, *g_bf, *g_wd, *g_bd;
  float *scalars, *latent, *mean, *logvar, *out, *eps_out;
  float* g;
  int B, D, L;
};

__global__ __launch_bounds__(VAF_THREADS) void vaeframe_step_kernel(VafStepArgs p) {
  extern __shared__ __align__(16) float smem[];
  const int B = p.B, D = p.D, L = p.L;
  const VafLayout o = vaf_layout(B, L);
  const int ldl = o.ldl;
  float* H = smem + o.h;
  float* M = smem + o.m;
  float* V = smem + o.v;
  float* EPS = smem + o.eps;
  float* Z = smem + o.z;
  float* C = smem + o.c;
  float* RED = smem + o.red;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nrt = (B + 15) >> 4, nlt = (L + 15) >> 4, ndt = (D + 15) >> 4;
  const int n = B * L;

  auto xm_at = [&](int b, int d) { return dropped_at(p.x, p.keep, p.scale, D, b, d); };

  // ---- S0: the noise into LDS: given, or Philox block g4 <-> elements 4 g4 .. 4 g4 + 3 of the row-major (B,L) array
  const bool draw = p.eps_in == nullptr;
  const uint64_t off = draw ? (uint64_t)p.counter[0] : 0ull;
  if (draw) {
    for (int g4 = tid; g4 < (n + 3) / 4; g4 += VAF_THREADS) {
      float ep[4];
      philox_normal4(g4, off, p.seed, ep);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int e = 4 * g4 + r;
        if (e < n) {
          const int b = e / L, l = e - b * L;
          EPS[b * ldl + l] = ep[r];
          p.eps_out[e] = ep[r];
        }
      }
    }
  } else {
    for (int e = tid; e < n; e += VAF_THREADS) {
      const int b = e / L, l = e - b * L;
      const float v = p.eps_in[e];
      EPS[b * ldl + l] = v;
      if (p.eps_out) p.eps_out[e] = v;
    }
  }

  // ---- S1: h = tanh(xm We^T + be) -> H
  for (int tt = w; tt < nrt * nlt; tt += VAF_NW)
    rows_tile(D, lane, (tt / nlt) * 16, B, (tt % nlt) * 16, L, xm_at, [&](int k, int l) { return p.we[(int64_t)l * D + k]; },
              [&](int b, int l, float v) {
                const float h = tanhf(v + p.be[l]);
                H[b * ldl + l] = h;
                if (p.latent) p.latent[(int64_t)b * L + l] = h;
              });
  __syncthreads();
  if (draw && tid == 0) p.counter[0] = (int64_t)(off + 1);      // (every thread has read the counter: the barrier above)

  // ---- S2: mean = h Wm^T + bm, logvar = h Ws^T + bs (one wave forms both tiles), z, the kl partial sums
  {
    float kl = 0.f;
    for (int tt = w; tt < nrt * nlt; tt += VAF_NW) {
      const int r0 = (tt / nlt) * 16, l0 = (tt % nlt) * 16;
      Side s;
      auto h_at = [&](int b, int k) { return H[b * ldl + k]; };
      // (not rows_tile: two accumulators meet in one epilogue)
      const f32x4 am = tile_guarded(L, lane, r0, B, l0, L, h_at, [&](int k, int l) { return p.wm[l * L + k]; }, s);
      const f32x4 as = tile_guarded(L, lane, r0, B, l0, L, h_at, [&](int k, int l) { return p.ws[l * L + k]; }, s);
      tile_each(lane, r0, B, l0, L, [&](int r, int b, int l) {
        const float mu = am[r] + p.bm[l], lv = as[r] + p.bs[l];
        const float zz = fmaf(expf(0.5f * lv), EPS[b * ldl + l], mu);
        kl += ((expf(lv) - lv) - 1.0f) + mu * mu;
        M[b * ldl + l] = mu;
        V[b * ldl + l] = lv;
        Z[b * ldl + l] = zz;
        if (p.mean) p.mean[(int64_t)b * L + l] = mu;
        if (p.logvar) p.logvar[(int64_t)b * L + l] = lv;
      });
    }
    kl = wave_sum(kl);
    if (lane == 0) RED[w] = kl;
  }
  __syncthreads();

  // ---- S3: c = z Wf^T + bf -> C
  for (int tt = w; tt < nrt * nlt; tt += VAF_NW)
    rows_tile(L, lane, (tt / nlt) * 16, B, (tt % nlt) * 16, L, [&](int b, int k) { return Z[b * ldl + k]; },
              [&](int k, int l) { return p.wf[l * L + k]; }, [&](int b, int l, float v) { C[b * ldl + l] = v + p.bf[l]; });
  __syncthreads();

  // ---- S4: out = c Wd^T + bd, g = 2 (out - t) / (B D), the mse partial sums
  {
    float rec = 0.f;
    const float gsc = 2.0f / ((float)B * (float)D);
    for (int tt = w; tt < nrt * ndt; tt += VAF_NW)
      rows_tile(L, lane, (tt / ndt) * 16, B, (tt % ndt) * 16, D, [&](int b, int k) { return C[b * ldl + k]; },
                [&](int k, int d) { return p.wd[(int64_t)d * L + k]; },
                [&](int b, int d, float v) { recon_epilogue(v, p.bd[d], (int64_t)b * D + d, p.t, gsc, p.out, p.g, rec); });
    rec = wave_sum(rec);
    if (lane == 0) RED[VAF_NW + w] = rec;
  }
  __syncthreads();      // (also orders the stores of g before the loads below: one workgroup)
  if (tid == 0) {
    float k = 0.f, r = 0.f;
    for (int i = 0; i < VAF_NW; ++i) {
      k += RED[i];
      r += RED[VAF_NW + i];
    }
    const float mse = r / ((float)B * (float)D), klm = k / ((float)B * (float)L);
    p.scalars[0] = mse;
    p.scalars[1] = klm;
    p.scalars[2] = mse + p.kl_weight * klm;
  }

  auto g_at = [&](int b, int d) { return p.g[(int64_t)b * D + d]; };

  // ---- S5a: dWd = g^T c, dbd = sum_b g
  for (int tt = w; tt < ndt * nlt; tt += VAF_NW)
    wgrad_tile(B, lane, (tt / nlt) * 16, D, (tt % nlt) * 16, L, g_at, [&](int b, int l) { return C[b * ldl + l]; }, p.g_wd, p.g_bd);
  __syncthreads();

  // ---- S5b: dc = g Wd in place of c
  for (int tt = w; tt < nrt * nlt; tt += VAF_NW)
    rows_tile(D, lane, (tt / nlt) * 16, B, (tt % nlt) * 16, L, g_at, [&](int k, int l) { return p.wd[(int64_t)k * L + l]; },
              [&](int b, int l, float v) { C[b * ldl + l] = v; });
  __syncthreads();

  // ---- S6: dWf = dc^T z, dbf = sum_b dc | S7: dz = dc Wf (registers only) -> dmean in place of mean, dlogvar in place of logvar.
  //      S6 reads C and Z, S7 reads C and reads and writes its own elements of M and V: the two share the phase.
  {
    const int n6 = nlt * nlt, n7 = nrt * nlt;
    const float kap = p.kl_weight / ((float)B * (float)L);
    auto c_at = [&](int b, int l) { return C[b * ldl + l]; };
    for (int tt = w; tt < n6 + n7; tt += VAF_NW) {
      if (tt < n6) {
        wgrad_tile(B, lane, (tt / nlt) * 16, L, (tt % nlt) * 16, L, c_at, [&](int b, int l) { return Z[b * ldl + l]; }, p.g_wf,
                   p.g_bf);
      } else {
        const int t7 = tt - n6;
        rows_tile(L, lane, (t7 / nlt) * 16, B, (t7 % nlt) * 16, L, c_at, [&](int k, int l) { return p.wf[k * L + l]; },
                  [&](int b, int l, float v) {
                    const float mu = M[b * ldl + l], lv = V[b * ldl + l], ep = EPS[b * ldl + l];
                    M[b * ldl + l] = v + 2.0f * kap * mu;
                    V[b * ldl + l] = v * (0.5f * expf(0.5f * lv) * ep) + kap * (expf(lv) - 1.0f);
                  });
      }
    }
  }
  __syncthreads();

  // ---- S8: dWm = dmean^T h, dbm | dWs = dlogvar^T h, dbs | dh = dmean Wm + dlogvar Ws as ONE chain over the concatenated 2 L,
  //      dpre = dh (1 - h^2) in place of z (dead since S6)
  {
    const int n8 = nlt * nlt, n8b = nrt * nlt;
    for (int tt = w; tt < 2 * n8 + n8b; tt += VAF_NW) {
      if (tt < 2 * n8) {
        const bool second = tt >= n8;
        const int t8 = second ? tt - n8 : tt;
        const float* S = second ? V : M;
        wgrad_tile(B, lane, (t8 / nlt) * 16, L, (t8 % nlt) * 16, L, [&](int b, int o2) { return S[b * ldl + o2]; },
                   [&](int b, int l) { return H[b * ldl + l]; }, second ? p.g_ws : p.g_wm, second ? p.g_bs : p.g_bm);
      } else {
        const int t8 = tt - 2 * n8;
        rows_tile(2 * L, lane, (t8 / nlt) * 16, B, (t8 % nlt) * 16, L,
                  [&](int b, int k) { return k < L ? M[b * ldl + k] : V[b * ldl + k - L]; },
                  [&](int k, int l) { return k < L ? p.wm[k * L + l] : p.ws[(k - L) * L + l]; },
                  [&](int b, int l, float v) {
                    const float h = H[b * ldl + l];
                    Z[b * ldl + l] = v * (1.0f - h * h);
                  });
      }
    }
  }
  __syncthreads();

  // ---- S9: dWe = dpre^T xm, dbe = sum_b dpre
  for (int tt = w; tt < nlt * ndt; tt += VAF_NW)
    wgrad_tile(B, lane, (tt / ndt) * 16, L, (tt % ndt) * 16, D, [&](int b, int l) { return Z[b * ldl + l]; }, xm_at, p.g_we, p.g_be);
}

// dpre = dy (1 - y^2)
__global__ __launch_bounds__(256) void tanh_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dpre,
                                                       int64_t n) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const float v = y[e];
    dpre[e] = dy[e] * (1.0f - v * v);
  }
}

constexpr int RPM_THREADS = 256;      // one Philox block (four elements) per thread: 1024 elements per workgroup

// z, eps_out and this workgroup's partial sum of exp(logvar) - logvar - 1 + mean^2 (a fixed tree)
__global__ __launch_bounds__(RPM_THREADS) void reparam_fwd_kernel(const float* __restrict__ mean, const float* __restrict__ logvar,
                                                                  const float* __restrict__ eps_in, uint64_t seed,
                                                                  const int64_t* __restrict__ counter, int sample, float* __restrict__ z,
                                                                  float* __restrict__ eps_out, float* __restrict__ partial, int64_t n) {
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t g4 = (int64_t)blockIdx.x * RPM_THREADS + tid;
  const bool draw = sample && !eps_in;
  float kl = 0.f;
  if (4 * g4 < n) {
    float ep[4] = {0.f, 0.f, 0.f, 0.f};
    if (draw) philox_normal4(g4, (uint64_t)counter[0], seed, ep);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t e = 4 * g4 + r;
      if (e < n) {
        const float mu = mean[e], lv = logvar[e];
        if (sample && !draw) ep[r] = eps_in[e];
        z[e] = sample ? fmaf(expf(0.5f * lv), ep[r], mu) : mu;
        if (sample && eps_out) eps_out[e] = ep[r];
        kl += ((expf(lv) - lv) - 1.0f) + mu * mu;
      }
    }
  }
  kl = wave_sum(kl);
  if (lane == 0) red[wave] = kl;
  __syncthreads();
  if (tid == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void reparam_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ g_kl,
                                                          const float* __restrict__ g_mean, const float* __restrict__ g_logvar,
                                                          const float* __restrict__ mean, const float* __restrict__ logvar,
                                                          const float* __restrict__ eps, float* __restrict__ dmean,
                                                          float* __restrict__ dlogvar, float inv_n, int64_t n) {
  const float c = g_kl ? g_kl[0] * inv_n : 0.f;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const float mu = mean[e], lv = logvar[e], d = dz ? dz[e] : 0.f, ep = eps ? eps[e] : 0.f;
    dmean[e] = (d + 2.0f * c * mu) + (g_mean ? g_mean[e] : 0.f);
    dlogvar[e] = (d * (0.5f * expf(0.5f * lv) * ep) + c * (expf(lv) - 1.0f)) + (g_logvar ? g_logvar[e] : 0.f);
  }
}

const char* vaf_refusal(int B, int D, int L) {
  if (B < 2) return "a batch needs B >= 2 (the reference's squeeze drops the row axis of a single frame)";
  if (D < 1 || L < 1) return "bad size";
  if ((int64_t)B * frame_ld(L) > (int64_t)(VAF_LDS_BYTES / sizeof(float)) ||
      vaf_layout(B, L).total * sizeof(float) > VAF_LDS_BYTES)
    return "the batch does not fit one CU's 160 KB of LDS";
  return nullptr;
}

constexpr int64_t RPM_MAX_N = (int64_t)4 * RPM_THREADS * (INT32_MAX / 2);
inline int rpm_blocks(int64_t n) { return (int)((n + 4 * RPM_THREADS - 1) / (4 * RPM_THREADS)); }
inline int ew_blocks(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, 4096); }

}  // namespace
}  // namespace g2v

using namespace g2v;

static bool vaf_auto_takes_fused(int B, int D, int L) { return B <= VAF_AUTO_MAX_B && D <= VAF_AUTO_MAX_D && L <= VAF_AUTO_MAX_L; }

extern "C" int g2v_vaeframe_plan(int B, int D, int L, int training) {
  if (D < 1 || L < 1 || B < 2) return G2V_VQFRAME_REFUSED;
  const bool ok = training && vaf_refusal(B, D, L) == nullptr;
  const bool take = ok && vaf_auto_takes_fused(B, D, L);
  return (take ? G2V_VQFRAME_FUSED : G2V_VQFRAME_STAGED) | (ok ? G2V_VQFRAME_FUSED_OK : 0);
}

extern "C" const char* g2v_vaeframe_plan_reason(int B, int D, int L, int training) {
  if (D < 1 || L < 1 || B < 1) return "refused: bad size";
  if (B < 2) return "refused: a batch needs B >= 2 (the reference's squeeze drops the row axis of a single frame)";
  if (!training) return "staged: the eval-mode forward has no fused kernel";
  if (const char* why = vaf_refusal(B, D, L)) return why;
  if (vaf_auto_takes_fused(B, D, L)) return "fused: inside the shapes measured faster than the staged route";
  return "staged: the fused step is admitted but not measured faster at this shape";
}

extern "C" size_t g2v_vaeframe_workspace(int B, int D, int L) {
  return vaf_refusal(B, D, L) ? 0 : (((size_t)B * (size_t)D + 3) / 4 * 4) * sizeof(float);
}

extern "C" size_t g2v_vaeframe_step_lds(int B, int D, int L) {
  return vaf_refusal(B, D, L) ? 0 : vaf_layout(B, L).total * sizeof(float);
}

extern "C" int g2v_vaeframe_step(const float* x, const float* target, const uint8_t* keep, float scale, const float* w_enc,
                                 const float* b_enc, const float* w_mean, const float* b_mean, const float* w_std, const float* b_std,
                                 const float* w_fc, const float* b_fc, const float* w_dec, const float* b_dec, float kl_weight,
                                 const float* eps_in, uint64_t seed, int64_t* offset_counter, float* g_w_enc, float* g_b_enc,
                                 float* g_w_mean, float* g_b_mean, float* g_w_std, float* g_b_std, float* g_w_fc, float* g_b_fc,
                                 float* g_w_dec, float* g_b_dec, float* scalars, float* latent, float* mean, float* logvar, float* out,
                                 float* eps_out, void* workspace, size_t workspace_bytes, int B, int D, int L, g2v_stream_t stream) {
  G2V_REQUIRE(x && target && w_enc && b_enc && w_mean && b_mean && w_std && b_std && w_fc && b_fc && w_dec && b_dec, "null pointer");
  G2V_REQUIRE(g_w_enc && g_b_enc && g_w_mean && g_b_mean && g_w_std && g_b_std && g_w_fc && g_b_fc && g_w_dec && g_b_dec && scalars &&
                  workspace,
              "null output pointer");
  G2V_REQUIRE(eps_in || (offset_counter && eps_out), "drawing the noise needs offset_counter and eps_out");
  if (const char* why = vaf_refusal(B, D, L)) {
    set_error("g2v_vaeframe_step: shape not served: %s (see g2v_vaeframe_plan)", why);
    return B < 2 || D < 1 || L < 1 ? G2V_ERR_ARG : G2V_ERR_UNSUPPORTED;
  }
  G2V_REQUIRE(workspace_bytes >= g2v_vaeframe_workspace(B, D, L), "workspace too small");
  VafStepArgs a;
  a.x = x; a.t = target; a.keep = keep; a.scale = scale;
  a.we = w_enc; a.be = b_enc; a.wm = w_mean; a.bm = b_mean; a.ws = w_std; a.bs = b_std; a.wf = w_fc; a.bf = b_fc; a.wd = w_dec; a.bd = b_dec;
  a.kl_weight = kl_weight; a.eps_in = eps_in; a.seed = seed; a.counter = offset_counter;
  a.g_we = g_w_enc; a.g_be = g_b_enc; a.g_wm = g_w_mean; a.g_bm = g_b_mean; a.g_ws = g_w_std; a.g_bs = g_b_std;
  a.g_wf = g_w_fc; a.g_bf = g_b_fc; a.g_wd = g_w_dec; a.g_bd = g_b_dec;
  a.scalars = scalars; a.latent = latent; a.mean = mean; a.logvar = logvar; a.out = out; a.eps_out = eps_out;
  a.g = static_cast<float*>(workspace);
  a.B = B; a.D = D; a.L = L;
  const size_t lds = vaf_layout(B, L).total * sizeof(float);
  if (!g2v_internal_lds_reserve((const void*)vaeframe_step_kernel, lds)) return G2V_ERR_LAUNCH;
  hipLaunchKernelGGL(vaeframe_step_kernel, dim3(1), dim3(VAF_THREADS), lds, (hipStream_t)stream, a);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int g2v_tanh_bwd(const float* dy, const float* y, float* dpre, int64_t n, g2v_stream_t stream) {
  G2V_REQUIRE(dy && y && dpre, "null pointer");
  G2V_REQUIRE(n >= 1, "bad size");
  hipLaunchKernelGGL(tanh_bwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, dy, y, dpre, n);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" size_t g2v_reparam_workspace(int64_t n) {
  return n >= 1 && n <= RPM_MAX_N ? (size_t)round_up(rpm_blocks(n), 4) * sizeof(float) : 0;
}

extern "C" int g2v_reparam_fwd(const float* mean, const float* logvar, const float* eps_in, uint64_t seed, int64_t* offset_counter,
                               int sample, float* z, float* eps_out, float* kl, void* workspace, size_t workspace_bytes, int64_t n,
                               g2v_stream_t stream) {
  G2V_REQUIRE(mean && logvar && z && kl && workspace, "null pointer");
  G2V_REQUIRE(n >= 1 && n <= RPM_MAX_N, "bad size");
  const bool draw = sample && !eps_in;
  G2V_REQUIRE(!draw || (offset_counter && eps_out), "drawing the noise needs offset_counter and eps_out (the backward reads eps)");
  G2V_REQUIRE(workspace_bytes >= g2v_reparam_workspace(n), "workspace too small");
  const int nblk = rpm_blocks(n);
  float* partial = static_cast<float*>(workspace);
  hipLaunchKernelGGL(reparam_fwd_kernel, dim3(nblk), dim3(RPM_THREADS), 0, (hipStream_t)stream, mean, logvar, sample ? eps_in : nullptr,
                     seed, offset_counter, sample ? 1 : 0, z, sample ? eps_out : nullptr, partial, n);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(vae_kl_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, nblk, 1.0f / (float)n, kl);
  G2V_CHECK_LAUNCH();
  if (draw) return g2v_counter_add(offset_counter, 1, stream);
  return G2V_OK;
}

extern "C" int g2v_reparam_bwd(const float* dz, const float* g_kl, const float* g_mean, const float* g_logvar, const float* mean,
                               const float* logvar, const float* eps, float* dmean, float* dlogvar, int64_t n, g2v_stream_t stream) {
  G2V_REQUIRE(mean && logvar && dmean && dlogvar, "null pointer");
  G2V_REQUIRE(n >= 1, "bad size");
  hipLaunchKernelGGL(reparam_bwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, dz, g_kl, g_mean, g_logvar, mean, logvar,
                     eps, dmean, dlogvar, 1.0f / (float)n, n);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
