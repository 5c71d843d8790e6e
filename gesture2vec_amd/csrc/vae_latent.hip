// vae_latent.hip -- the variational block of the chunk autoencoder (autoencoder_vae == "True", reference
// model/Autoencoder_VQVAE_model.py:776-789, 879-899, 989-1010; train_eval/train_seq2seq.py:710-729) as ONE forward launch (+ a
// one-workgroup finish of the KL scalar) and ONE backward launch.
//
// The block sits between the encoder state h (L,B,H) -- or the quantiser's output of the same shape -- and the decoder's initial
// state d (L,B,H).  Row b of hf = h.transpose(1, 0).reshape(B, E), E = L H, is [h[0, b] ; h[1, b] ; ...]:
//     mean = hf W_mean^T + b_mean,  logvar = hf W_std^T + b_std,  z = mean + exp(logvar / 2) eps,  d = z W_dec^T + b_dec
//     KLD  = 0.5 mean(exp(logvar) - logvar - 1 + mean^2)           over all B E elements
// The block is row-local (only the KL mean meets other rows, as per-workgroup partial sums), so a workgroup (four or sixteen
// waves) owns 16 WHOLE rows: the hf tile is gathered once from the (L,B,H) layout (segment addressing, no transposed copy) and feeds both E x E
// products; the epilogue forms z, eps and the KL term in registers; z stays in LDS for the third product, whose output goes back
// to the (L,B,H) layout.  The weights stream from L2 as MFMA operands (exact fp32 v_mfma_f32_16x16x4_f32, common.hpp:
// wave_gemm for a contraction along the weight's rows, wave_gemm_t below for one across them).
//
// Noise: a caller-supplied eps (B,E), or eps drawn here from the project's Philox stream (seed, offset_counter[0]): block g of the
// stream is elements 4g .. 4g+3 of the row-major (B,E) array -- g2v_keep_mask's mapping -- turned into four normal deviates by
// two Box-Muller pairs.  The drawn eps is written out: the backward reads it.  sample == 0: z = mean (the extractors' train=False).
//
// Determinism: no atomics; every sum has a fixed order, so the same inputs give the same bits.
// Served: E % 16 == 0, E <= 512 (g2v_vae_latent_ok); any B >= 1.
#include "common.hpp"
#include "vae_noise.hpp"      // philox_normal4 (the noise), vae_kl_finish_kernel (KLD = 0.5 sum(partials) / (B E))

namespace g2v {
namespace {

constexpr int VAE_ROWS = 16;
constexpr int VAE_MAX_E = 512;

// acc[t][r] += sum_k W[k][c0 + cstride t + 4q + r] * Xs[i][k]   (k = 0 .. K-1, K % 16 == 0): the contraction runs ACROSS the rows of
// the row-major W (ld = ldw), i.e. x W rather than x W^T.  Lane (i, q) fetches dword "columns" W[kb + 4q + c][col + i], so that
// the LDS operand of the four MFMAs of a 16-deep block is one float4.  Two blocks of 16 k in flight per buffer, double-buffered.
template <int NT>
__device__ __forceinline__ void wave_gemm_t(f32x4 (&acc)[NT], const float* __restrict__ W, int64_t ldw, int c0, int cstride, int K,
                                            const float* Xs, int ldx, int lane) {
  const int i = lane & 15, q = lane >> 4;
  constexpr int CH = 2;
  const int nks = K >> 4, nch = (nks + CH - 1) / CH;
  float wa[CH][NT][4], wb[CH][NT][4];
  auto loadc = [&](int c, float (&w)[CH][NT][4]) {
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int ks = c * CH + j;
      const bool ok = ks < nks;
      const int kb = ok ? 16 * ks : 0;            // past the end: clamped address, zero fragment
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = W[(int64_t)(kb + 4 * q + e) * ldw + c0 + cstride * t + i];
          w[j][t][e] = ok ? v : 0.f;
        }
    }
  };
  auto mmac = [&](int c, const float (&w)[CH][NT][4]) {
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int ks = c * CH + j;
      if (ks < nks) {
        const float4 xb = *reinterpret_cast<const float4*>(Xs + i * ldx + 16 * ks + 4 * q);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          acc[t] = mfma16(w[j][t][0], xb.x, acc[t]);
          acc[t] = mfma16(w[j][t][1], xb.y, acc[t]);
          acc[t] = mfma16(w[j][t][2], xb.z, acc[t]);
          acc[t] = mfma16(w[j][t][3], xb.w, acc[t]);
        }
      }
    }
  };
  loadc(0, wa);
  for (int c = 0; c < nch; c += 2) {
    loadc(c + 1, wb);
    __builtin_amdgcn_sched_barrier(0);
    mmac(c, wa);
    loadc(c + 2, wa);
    __builtin_amdgcn_sched_barrier(0);
    if (c + 1 < nch) mmac(c + 1, wb);
  }
}

// element c (0 .. E-1) of row n of hf <-> (L,B,H) element: layer c / H, column c % H.  H % 4 == 0: a float4 never straddles layers.
__device__ __forceinline__ int64_t seg_off(int64_t n, int c, int B, int H) {
  const int l = c / H;
  return ((int64_t)l * B + n) * H + (c - l * H);
}

struct VaeFwdArgs {
  const float* h;                                   // (L,B,H)
  const float *w_mean, *b_mean, *w_std, *b_std;     // (E,E), (E)
  const float *w_dec, *b_dec;                       // (E,E), (E); w_dec NULL: no d
  const float* eps_in;                              // (B,E) or NULL (drawn here when sample != 0)
  const int64_t* offset_counter;
  uint64_t seed;
  float *mean, *logvar, *z, *eps_out, *hf, *d;      // (B,E) x 5 (eps_out / hf may be NULL); d (L,B,H)
  float* kl_partial;                                // [blocks]
  int B, E, H, sample;
};

// NW waves per workgroup: wave w owns the feature tiles w, w + NW, w + 2 NW, ... (two at a time).  Four waves where the batch
// alone fills the device; sixteen at small batch, where a handful of workgroups would otherwise walk E / 16 tiles four at a time.
// LDS (floats): Xs[16][E+4] | Zs[16][E+4] | red[NW]
template <int NW>
__global__ __launch_bounds__(64 * NW) void vae_latent_fwd_kernel(VaeFwdArgs a) {
  constexpr int NTH = 64 * NW, TS = 16 * NW;          // threads; row stride between a wave's two tiles
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int E = a.E, H = a.H, B = a.B, LD = E + 4, E4 = E >> 2, ntile = E >> 4;
  float* Xs = smem;
  float* Zs = Xs + VAE_ROWS * LD;
  float* red = Zs + VAE_ROWS * LD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * VAE_ROWS, nrows = min(VAE_ROWS, B - n0);
  const bool rowok = i < nrows;
  const int64_t n = n0 + (rowok ? i : nrows - 1);

  // ---- the hf tile, gathered from the (L,B,H) layout; rows past the batch are zero -------------------------------------------------
  for (int e4 = tid; e4 < VAE_ROWS * E4; e4 += NTH) {
    const int r = e4 / E4, c = (e4 - r * E4) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < nrows) {
      v = *reinterpret_cast<const float4*>(a.h + seg_off(n0 + r, c, B, H));
      if (a.hf) *reinterpret_cast<float4*>(a.hf + (int64_t)(n0 + r) * E + c) = v;
    }
    *reinterpret_cast<float4*>(Xs + r * LD + c) = v;
  }
  const uint64_t off = (a.sample && !a.eps_in) ? (uint64_t)a.offset_counter[0] : 0ull;
  lds_barrier();

  // ---- mean / logvar tiles of this wave (feature tiles wave, wave + 4, ...), two at a time; epilogue in registers -----------------
  float kl = 0.f;
  auto epilogue = [&](int tile, const f32x4& am, const f32x4& as) {
    const int f0 = 16 * tile + 4 * q;
    const float4 bm4 = *reinterpret_cast<const float4*>(a.b_mean + f0);
    const float4 bs4 = *reinterpret_cast<const float4*>(a.b_std + f0);
    const float bm[4] = {bm4.x, bm4.y, bm4.z, bm4.w}, bs[4] = {bs4.x, bs4.y, bs4.z, bs4.w};
    float ep[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.sample) {
      if (a.eps_in) {
        const float4 e4 = *reinterpret_cast<const float4*>(a.eps_in + n * E + f0);
        ep[0] = e4.x; ep[1] = e4.y; ep[2] = e4.z; ep[3] = e4.w;
      } else {
        philox_normal4((n * E + f0) >> 2, off, a.seed, ep);
      }
    }
    float mu[4], lv[4], zz[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mu[r] = am[r] + bm[r];
      lv[r] = as[r] + bs[r];
      zz[r] = a.sample ? fmaf(expf(0.5f * lv[r]), ep[r], mu[r]) : mu[r];
      kl += rowok ? ((expf(lv[r]) - lv[r]) - 1.0f) + mu[r] * mu[r] : 0.f;
    }
    *reinterpret_cast<float4*>(Zs + i * LD + f0) = rowok ? make_float4(zz[0], zz[1], zz[2], zz[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (rowok) {
      *reinterpret_cast<float4*>(a.mean + n * E + f0) = make_float4(mu[0], mu[1], mu[2], mu[3]);
      *reinterpret_cast<float4*>(a.logvar + n * E + f0) = make_float4(lv[0], lv[1], lv[2], lv[3]);
      *reinterpret_cast<float4*>(a.z + n * E + f0) = make_float4(zz[0], zz[1], zz[2], zz[3]);
      if (a.eps_out) *reinterpret_cast<float4*>(a.eps_out + n * E + f0) = make_float4(ep[0], ep[1], ep[2], ep[3]);
    }
  };
  for (int t = wave; t < ntile; t += 2 * NW) {
    if (t + NW < ntile) {
      f32x4 am[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, as[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      wave_gemm<2>(am, a.w_mean, E, true, 16 * t, TS, 16, E, Xs, LD, lane);
      wave_gemm<2>(as, a.w_std, E, true, 16 * t, TS, 16, E, Xs, LD, lane);
      epilogue(t, am[0], as[0]);
      epilogue(t + NW, am[1], as[1]);
    } else {
      f32x4 am[1] = {{0.f, 0.f, 0.f, 0.f}}, as[1] = {{0.f, 0.f, 0.f, 0.f}};
      wave_gemm<1>(am, a.w_mean, E, true, 16 * t, 64, 16, E, Xs, LD, lane);
      wave_gemm<1>(as, a.w_std, E, true, 16 * t, 64, 16, E, Xs, LD, lane);
      epilogue(t, am[0], as[0]);
    }
  }
  kl = wave_sum(kl);
  if (lane == 0) red[wave] = kl;
  lds_barrier();                       // Zs complete, the waves' KL sums visible
  if (tid == 0) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NW; w += 4) s += (red[w] + red[w + 1]) + (red[w + 2] + red[w + 3]);
    a.kl_partial[blockIdx.x] = s;
  }
  if (!a.w_dec) return;

  // ---- d = z W_dec^T + b_dec, written back into the (L,B,H) layout ------------------------------------------------------------------
  auto store_d = [&](int tile, const f32x4& acc) {
    const int f0 = 16 * tile + 4 * q;
    const float4 b4 = *reinterpret_cast<const float4*>(a.b_dec + f0);
    if (rowok)
      *reinterpret_cast<float4*>(a.d + seg_off(n, f0, B, H)) = make_float4(acc[0] + b4.x, acc[1] + b4.y, acc[2] + b4.z, acc[3] + b4.w);
  };
  for (int t = wave; t < ntile; t += 2 * NW) {
    if (t + NW < ntile) {
      f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      wave_gemm<2>(acc, a.w_dec, E, true, 16 * t, TS, 16, E, Zs, LD, lane);
      store_d(t, acc[0]);
      store_d(t + NW, acc[1]);
    } else {
      f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
      wave_gemm<1>(acc, a.w_dec, E, true, 16 * t, 64, 16, E, Zs, LD, lane);
      store_d(t, acc[0]);
    }
  }
}

struct VaeBwdArgs {
  const float* g_d;                                 // (L,B,H): d loss / d d (the decoder stage's dh_init)
  const float* g_kl;                                // device scalar d loss / d KLD, or NULL (= 0)
  const float *g_mean, *g_logvar;                   // (B,E) gradients arriving at mean / logvar directly, or NULL (= 0)
  const float *mean, *logvar, *eps;                 // (B,E); eps NULL: the forward did not sample (z = mean)
  const float *w_mean, *w_std, *w_dec;              // (E,E)
  float *dmean, *dlogvar;                           // (B,E)
  float* dh;                                        // (L,B,H)
  float inv_n;                                      // 1 / (B E)
  int B, E, H;
};

// LDS (floats): Gs[16][E+4] | DM[16][E+4] | DS[16][E+4]
template <int NW>
__global__ __launch_bounds__(64 * NW) void vae_latent_bwd_kernel(VaeBwdArgs a) {
  constexpr int NTH = 64 * NW, TS = 16 * NW;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int E = a.E, H = a.H, B = a.B, LD = E + 4, E4 = E >> 2, ntile = E >> 4;
  float* Gs = smem;
  float* DM = Gs + VAE_ROWS * LD;
  float* DS = DM + VAE_ROWS * LD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * VAE_ROWS, nrows = min(VAE_ROWS, B - n0);
  const bool rowok = i < nrows;
  const int64_t n = n0 + (rowok ? i : nrows - 1);

  for (int e4 = tid; e4 < VAE_ROWS * E4; e4 += NTH) {
    const int r = e4 / E4, c = (e4 - r * E4) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < nrows) v = *reinterpret_cast<const float4*>(a.g_d + seg_off(n0 + r, c, B, H));
    *reinterpret_cast<float4*>(Gs + r * LD + c) = v;
  }
  const float ckl = a.g_kl ? a.g_kl[0] * a.inv_n : 0.f;
  lds_barrier();

  // ---- dz = g_d W_dec; dmean, dlogvar in registers -> global (the weight gradients read them) and LDS ----------------------------
  auto epilogue = [&](int tile, const f32x4& dz) {
    const int f0 = 16 * tile + 4 * q;
    const float4 m4 = *reinterpret_cast<const float4*>(a.mean + n * E + f0);
    const float4 l4 = *reinterpret_cast<const float4*>(a.logvar + n * E + f0);
    const float4 e4 = a.eps ? *reinterpret_cast<const float4*>(a.eps + n * E + f0) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float mu[4] = {m4.x, m4.y, m4.z, m4.w}, lv[4] = {l4.x, l4.y, l4.z, l4.w}, ep[4] = {e4.x, e4.y, e4.z, e4.w};
    const float4 gm4 = a.g_mean ? *reinterpret_cast<const float4*>(a.g_mean + n * E + f0) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 gl4 = a.g_logvar ? *reinterpret_cast<const float4*>(a.g_logvar + n * E + f0) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float gm[4] = {gm4.x, gm4.y, gm4.z, gm4.w}, gl[4] = {gl4.x, gl4.y, gl4.z, gl4.w};
    float dm[4], dl[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      dm[r] = rowok ? (dz[r] + ckl * mu[r]) + gm[r] : 0.f;
      dl[r] = rowok ? (dz[r] * (0.5f * expf(0.5f * lv[r]) * ep[r]) + ckl * (0.5f * (expf(lv[r]) - 1.0f))) + gl[r] : 0.f;
    }
    *reinterpret_cast<float4*>(DM + i * LD + f0) = make_float4(dm[0], dm[1], dm[2], dm[3]);
    *reinterpret_cast<float4*>(DS + i * LD + f0) = make_float4(dl[0], dl[1], dl[2], dl[3]);
    if (rowok) {
      *reinterpret_cast<float4*>(a.dmean + n * E + f0) = make_float4(dm[0], dm[1], dm[2], dm[3]);
      *reinterpret_cast<float4*>(a.dlogvar + n * E + f0) = make_float4(dl[0], dl[1], dl[2], dl[3]);
    }
  };
  for (int t = wave; t < ntile; t += 2 * NW) {
    if (t + NW < ntile) {
      f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      wave_gemm_t<2>(acc, a.w_dec, E, 16 * t, TS, E, Gs, LD, lane);
      epilogue(t, acc[0]);
      epilogue(t + NW, acc[1]);
    } else {
      f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
      wave_gemm_t<1>(acc, a.w_dec, E, 16 * t, TS, E, Gs, LD, lane);
      epilogue(t, acc[0]);
    }
  }
  lds_barrier();                       // DM / DS complete

  // ---- dh = dmean W_mean + dlogvar W_std: ONE accumulation over the concatenated K = 2 E, into the (L,B,H) layout -------------------
  auto store_dh = [&](int tile, const f32x4& acc) {
    const int f0 = 16 * tile + 4 * q;
    if (rowok) *reinterpret_cast<float4*>(a.dh + seg_off(n, f0, B, H)) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  };
  for (int t = wave; t < ntile; t += 2 * NW) {
    if (t + NW < ntile) {
      f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      wave_gemm_t<2>(acc, a.w_mean, E, 16 * t, TS, E, DM, LD, lane);
      wave_gemm_t<2>(acc, a.w_std, E, 16 * t, TS, E, DS, LD, lane);
      store_dh(t, acc[0]);
      store_dh(t + NW, acc[1]);
    } else {
      f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
      wave_gemm_t<1>(acc, a.w_mean, E, 16 * t, TS, E, DM, LD, lane);
      wave_gemm_t<1>(acc, a.w_std, E, 16 * t, TS, E, DS, LD, lane);
      store_dh(t, acc[0]);
    }
  }
}

inline bool a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Workgroups of sixteen waves while the row blocks alone leave CUs idle (measured), four beyond
constexpr int VAE_WIDE_MAX_BLOCKS = 128;
constexpr int VAE_NW_WIDE = 16;

template <int NW>
int launch_fwd(const VaeFwdArgs& a, int nblk, size_t lds, hipStream_t st) {
  if (!g2v_internal_lds_reserve((const void*)vae_latent_fwd_kernel<NW>, lds)) return G2V_ERR_LAUNCH;
  hipLaunchKernelGGL(vae_latent_fwd_kernel<NW>, dim3(nblk), dim3(64 * NW), lds, st, a);
  return G2V_OK;
}
template <int NW>
int launch_bwd(const VaeBwdArgs& a, int nblk, size_t lds, hipStream_t st) {
  if (!g2v_internal_lds_reserve((const void*)vae_latent_bwd_kernel<NW>, lds)) return G2V_ERR_LAUNCH;
  hipLaunchKernelGGL(vae_latent_bwd_kernel<NW>, dim3(nblk), dim3(64 * NW), lds, st, a);
  return G2V_OK;
}

}  // namespace
}  // namespace g2v

using namespace g2v;

extern "C" int g2v_vae_latent_ok(int B, int E) { return (B > 0 && E > 0 && (E % 16) == 0 && E <= VAE_MAX_E) ? 1 : 0; }
extern "C" int g2v_vae_latent_blocks(int B) { return B > 0 ? cdiv(B, VAE_ROWS) : 0; }
extern "C" size_t g2v_vae_latent_fwd_workspace(int B, int E) {
  return g2v_vae_latent_ok(B, E) ? (size_t)round_up(g2v_vae_latent_blocks(B), 4) * sizeof(float) : 0;
}

extern "C" int g2v_vae_latent_fwd(const float* h, const float* w_mean, const float* b_mean, const float* w_std, const float* b_std,
                                  const float* w_dec, const float* b_dec, const float* eps_in, uint64_t seed,
                                  int64_t* offset_counter, int sample, float* mean, float* logvar, float* z, float* eps_out,
                                  float* hf, float* d, float* kl, void* workspace, size_t workspace_bytes, int B, int L, int H,
                                  g2v_stream_t stream) {
  G2V_REQUIRE(h && w_mean && b_mean && w_std && b_std, "null pointer");
  G2V_REQUIRE(mean && logvar && z && kl && workspace, "null output pointer");
  G2V_REQUIRE((w_dec != nullptr) == (d != nullptr) && (!w_dec || b_dec), "w_dec, b_dec and d go together");
  G2V_REQUIRE(B > 0 && L > 0 && H > 0 && (H % 4) == 0, "bad size (H must be a multiple of 4)");
  const int64_t E64 = (int64_t)L * H;
  if (E64 > VAE_MAX_E || !g2v_vae_latent_ok(B, (int)E64)) {
    set_error("g2v_vae_latent_fwd: shape not served (see g2v_vae_latent_ok)");
    return G2V_ERR_UNSUPPORTED;
  }
  const int E = (int)E64;
  const bool draw = sample && !eps_in;
  G2V_REQUIRE(!draw || (offset_counter && eps_out), "drawing the noise needs offset_counter and eps_out (the backward reads eps)");
  G2V_REQUIRE(workspace_bytes >= g2v_vae_latent_fwd_workspace(B, E), "workspace too small");
  G2V_REQUIRE(a16(h) && a16(w_mean) && a16(b_mean) && a16(w_std) && a16(b_std) && a16(w_dec) && a16(b_dec) && a16(eps_in) &&
                  a16(mean) && a16(logvar) && a16(z) && a16(eps_out) && a16(hf) && a16(d) && a16(workspace),
              "16-byte alignment");
  VaeFwdArgs a;
  a.h = h; a.w_mean = w_mean; a.b_mean = b_mean; a.w_std = w_std; a.b_std = b_std; a.w_dec = w_dec; a.b_dec = b_dec;
  a.eps_in = sample ? eps_in : nullptr; a.offset_counter = offset_counter; a.seed = seed;
  a.mean = mean; a.logvar = logvar; a.z = z; a.eps_out = sample ? eps_out : nullptr; a.hf = hf; a.d = d;
  a.kl_partial = static_cast<float*>(workspace);
  a.B = B; a.E = E; a.H = H; a.sample = sample ? 1 : 0;
  const int nblk = g2v_vae_latent_blocks(B);
  const size_t lds = (size_t)(2 * VAE_ROWS * (E + 4) + VAE_NW_WIDE) * sizeof(float);
  if ((nblk <= VAE_WIDE_MAX_BLOCKS ? launch_fwd<VAE_NW_WIDE>(a, nblk, lds, (hipStream_t)stream)
                                   : launch_fwd<4>(a, nblk, lds, (hipStream_t)stream)) != G2V_OK)
    return G2V_ERR_LAUNCH;
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(vae_kl_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a.kl_partial, nblk,
                     0.5f / ((float)B * (float)E), kl);
  G2V_CHECK_LAUNCH();
  if (draw) return g2v_counter_add(offset_counter, 1, stream);
  return G2V_OK;
}

extern "C" int g2v_vae_latent_bwd(const float* g_d, const float* g_kl, const float* g_mean, const float* g_logvar, const float* mean, const float* logvar, const float* eps,
                                  const float* w_mean, const float* w_std, const float* w_dec, float* dmean, float* dlogvar,
                                  float* dh, int B, int L, int H, g2v_stream_t stream) {
  G2V_REQUIRE(g_d && mean && logvar && w_mean && w_std && w_dec, "null pointer");
  G2V_REQUIRE(dmean && dlogvar && dh, "null output pointer");
  G2V_REQUIRE(B > 0 && L > 0 && H > 0 && (H % 4) == 0, "bad size (H must be a multiple of 4)");
  const int64_t E64 = (int64_t)L * H;
  if (E64 > VAE_MAX_E || !g2v_vae_latent_ok(B, (int)E64)) {
    set_error("g2v_vae_latent_bwd: shape not served (see g2v_vae_latent_ok)");
    return G2V_ERR_UNSUPPORTED;
  }
  const int E = (int)E64;
  G2V_REQUIRE(a16(g_d) && a16(g_mean) && a16(g_logvar) && a16(mean) && a16(logvar) && a16(eps) && a16(w_mean) && a16(w_std) && a16(w_dec) && a16(dmean) &&
                  a16(dlogvar) && a16(dh),
              "16-byte alignment");
  VaeBwdArgs a;
  a.g_d = g_d; a.g_kl = g_kl; a.g_mean = g_mean; a.g_logvar = g_logvar; a.mean = mean; a.logvar = logvar; a.eps = eps;
  a.w_mean = w_mean; a.w_std = w_std; a.w_dec = w_dec; a.dmean = dmean; a.dlogvar = dlogvar; a.dh = dh;
  a.inv_n = 1.0f / ((float)B * (float)E);
  a.B = B; a.E = E; a.H = H;
  const size_t lds = (size_t)(3 * VAE_ROWS * (E + 4)) * sizeof(float);
  const int nblk = cdiv(B, VAE_ROWS);
  if ((nblk <= VAE_WIDE_MAX_BLOCKS ? launch_bwd<VAE_NW_WIDE>(a, nblk, lds, (hipStream_t)stream)
                                   : launch_bwd<4>(a, nblk, lds, (hipStream_t)stream)) != G2V_OK)
    return G2V_ERR_LAUNCH;
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
