// dec_chain.hip -- gesture generation: the pose decoder's eval-mode chain over the chunks of a clip in ONE launch
// (g2v_dec_chain_fwd), and the tail of a generated clip: blend across chunk boundaries, un-normalise, Savitzky-Golay
// (g2v_clip_finish).  include/g2v.h states both; DESIGN.md section 3.6d has the layout and the budget.
//
// In eval mode BatchNorm1d is a fixed affine map per hidden unit, so the rows of a batch never interact: a workgroup owns 16
// clips and runs every step of every chunk of those clips alone.  There is no exchange, no wait and nothing a fault latch would
// have to know about.  The hidden states (ping-pong), the carried frame and the step's activations stay in LDS for the whole
// launch; the weights are packed once per call into MFMA fragment order (BatchNorm folded into pre_linear by the pack kernel)
// and streamed from the workspace (L2) every step through the same wave-level products the per-step kernels use; at H = 64,
// D = 135 every wave keeps its fragments in registers for the whole launch instead.  The GRU cells are gru_cell_fwd /
// gru_cell_fwd_epilogue of gru_cells.hpp, called with no global outputs (nrows = 0): the gate arithmetic is not restated here.
#include "common.hpp"
#include "gru_cells.hpp"

namespace g2v {

constexpr int CHAIN_MAX_DIM = 256;      // D and H: 5 x 16 x (Hp + 4) + 3 x 16 x (Dp + 4) floats of LDS <= 130 KB

struct ChainPack {      // the packed weights in the workspace
  const float* pre;    // rows H, K = D, scaled by bn_w / sqrt(running_var + eps)
  const float* ih0; const float* hh0; const float* ih1; const float* hh1;   // 3 gate groups x H rows, K = H
  const float* out;    // rows D, K = H, zero tiles up to chain_out_tiles(D)
  const float* bf;     // (H)  (b_pre - running_mean) * scale + bn_b
  const float* bih0; const float* bhh0; const float* bih1; const float* bhh1;   // (3H) each, 16-byte aligned copies
  const float* bout;   // (D), zeros up to 16 * chain_out_tiles(D)
};

struct ChainLayout {      // offsets in floats; every region starts on a 256-byte boundary
  size_t pre, g[4], out, bf, bg[4], bout, total;
};
// out_layer's tiles: a multiple of 12, so that each of four waves may load three of them without a bounds test (the rest: zeros)
static int chain_out_tiles(int D) { return round_up(pack_ntile_g(D), 12); }
static ChainLayout chain_layout(int D, int H) {
  ChainLayout l;
  size_t o = 0;
  auto take = [&](size_t n) { const size_t r = o; o += (n + 63) / 64 * 64; return r; };
  l.pre = take(pack_floats(H, 1, D));
  for (int k = 0; k < 4; ++k) l.g[k] = take(pack_floats(H, 3, H));
  l.out = take((size_t)chain_out_tiles(D) * pack_ks(H) * 256);
  l.bf = take(H);
  for (int k = 0; k < 4; ++k) l.bg[k] = take(3 * (size_t)H);
  l.bout = take(16 * (size_t)chain_out_tiles(D));
  l.total = o;
  return l;
}

struct ChainPackArgs {
  PackBatch pb;              // d[0]: pre_linear (folded below), d[1..4]: the GRU matrices, d[5]: out_layer
  const float* b_pre; const float* bn_w; const float* bn_b; const float* rm; const float* rv;
  float* bf;
  const float* bsrc[5];      // b_ih0, b_hh0, b_ih1, b_hh1, b_out
  float* bdst[5];
  int bn[5];
  int H, bout_pad;           // bout_pad: floats of the b_out copy, zero beyond D
};
// BatchNorm1d in eval mode as the scale of a pre_linear row and a bias: a = ReLU(xin (s W)^T + ((b_pre - mean) s + bn_b)),
// s = bn_w / sqrt(var + 1e-5) with the correctly rounded division and square root (once per call, not on the step path)
__device__ __forceinline__ float chain_bn_scale(const ChainPackArgs& a, int h) { return a.bn_w[h] / sqrtf(a.rv[h] + 1e-5f); }
static __global__ __launch_bounds__(256) void chain_pack_kernel(ChainPackArgs a) {
  const int y = blockIdx.y;
  if (y == 0) {      // pack_one with the row scale
    const PackDesc& d = a.pb.d[0];
    const int ntg = (d.rows_per_group + 15) >> 4, KS = (d.K + 15) >> 4;
    for (int blk = blockIdx.x; blk < ntg * KS; blk += gridDim.x) {
      const int s = blk % KS, f = blk / KS;
      const int lane = threadIdx.x >> 2, e = threadIdx.x & 3;
      const int rg = 16 * f + (lane & 15), c = 16 * s + 4 * (lane >> 4) + e;
      float v = 0.f;
      if (rg < d.rows_per_group && c < d.K) v = d.src[(int64_t)rg * d.ld + c] * chain_bn_scale(a, rg);
      d.dst[(int64_t)blk * 256 + threadIdx.x] = v;
    }
  } else if (y < 6) {
    pack_one(a.pb.d[y]);
  } else {
    const int e0 = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
    for (int h = e0; h < a.H; h += step) a.bf[h] = (a.b_pre[h] - a.rm[h]) * chain_bn_scale(a, h) + a.bn_b[h];
    for (int k = 0; k < 5; ++k)
      for (int e = e0; e < a.bn[k]; e += step) a.bdst[k][e] = a.bsrc[k][e];
    for (int e = a.bn[4] + e0; e < a.bout_pad; e += step) a.bdst[4][e] = 0.f;
  }
}

struct ChainArgs {
  const float* rows; const int64_t* ids; const float* start; const float* teacher; const uint8_t* keep95;
  float* out; float* h_last;
  ChainPack pk;
  int64_t R;
  int n_pre, conditioned, C, T, W, B, D, H;
};

// FAST (H = 64, D = 135, four waves: wave w owns hidden-unit tile w and pose tiles w, w + 4, w + 8): every weight fragment the wave
// multiplies with is loaded ONCE, before the first step, and stays in its registers for the whole launch -- 5 x 48 + 36 of them
// plus the biases -- so a step touches no memory but LDS and the arrays of the call.  Same products in the same k order as the
// generic path: the two give the same bits.
constexpr int CHAIN_FAST_H = 64, CHAIN_FAST_D = 135;
template <int NW, bool FAST>
__global__ __launch_bounds__(NW * 64) void dec_chain_kernel(ChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NTHR = NW * 64;
  static_assert(!FAST || NW == 4, "the register-resident path deals one hidden-unit tile to each of four waves");
  const int D = FAST ? CHAIN_FAST_D : a.D, H = FAST ? CHAIN_FAST_H : a.H, T = a.T, W = a.W, C = a.C, B = a.B;
  const int Hp = (H + 15) & ~15, Dp = (D + 15) & ~15, ldh = Hp + 4, ldd = Dp + 4;
  float* Xa = smem;                                              // a_t                        [16][ldh]
  float* Xh0[2] = {Xa + 16 * ldh, Xa + 2 * 16 * ldh};            // layer-0 state, ping-pong (the new one is layer 1's input)
  float* Xh1[2] = {Xa + 3 * 16 * ldh, Xa + 4 * 16 * ldh};        // layer-1 state, ping-pong
  float* Xy = Xa + 5 * 16 * ldh;                                 // xin_t                      [16][ldd]
  float* Xc = Xy + 16 * ldd;                                     // the next input, undropped (the carried frame)
  float* Yt = Xc + 16 * ldd;                                     // y_t
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b0 = blockIdx.x * 16;
  const int nrows = min(16, B - b0);
  const int i = lane & 15, q = lane >> 4;
  const int KSD = Dp >> 4, KSH = Hp >> 4;
  const int S = W + T - 1;
  const int64_t F = (int64_t)C * T;
  const ChainPack& pk = a.pk;
  constexpr int FKSH = FAST ? CHAIN_FAST_H / 16 : 1, FKSD = FAST ? (CHAIN_FAST_D + 15) / 16 : 1;
  WFrag<1, FKSD> f_pre;
  WFrag<3, FKSH> f_ih0, f_hh0, f_ih1, f_hh1, f_out;
  float4 bi0[3], bh0[3], bi1[3], bh1[3], bf4, bo4[3];
  if constexpr (FAST) {
    const int f0 = 16 * wave + 4 * q;
    frag_load(f_pre, pk.pre, wave, 0, lane);
    frag_load(f_ih0, pk.ih0, wave, 4, lane);
    frag_load(f_hh0, pk.hh0, wave, 4, lane);
    frag_load(f_ih1, pk.ih1, wave, 4, lane);
    frag_load(f_hh1, pk.hh1, wave, 4, lane);
    frag_load(f_out, pk.out, wave, 4, lane);      // (the pack pads out_layer to 12 tiles: tiles 9..11 are zeros)
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      bi0[g] = *reinterpret_cast<const float4*>(pk.bih0 + g * H + f0);
      bh0[g] = *reinterpret_cast<const float4*>(pk.bhh0 + g * H + f0);
      bi1[g] = *reinterpret_cast<const float4*>(pk.bih1 + g * H + f0);
      bh1[g] = *reinterpret_cast<const float4*>(pk.bhh1 + g * H + f0);
      bo4[g] = *reinterpret_cast<const float4*>(pk.bout + 16 * (wave + 4 * g) + 4 * q);      // (bout is zero-padded to 12 tiles)
    }
    bf4 = *reinterpret_cast<const float4*>(pk.bf + f0);
  }

  // Everything an MFMA contraction reads must be a number: padding columns and the rows past the batch stay zero for the whole
  // launch (the loops below write rows < nrows and columns < D / < H only).
  for (int e = tid; e < 5 * 16 * ldh + 3 * 16 * ldd; e += NTHR) smem[e] = 0.f;
  lds_barrier();
  // The element loops over a [16][D] tile all use the same e -> (row, column) map: a thread re-reads in Xc only what it wrote.
  if (a.start) {
    for (int e = tid; e < 16 * D; e += NTHR) {
      const int r = e / D, d = e - r * D;
      if (r < nrows) Xc[r * ldd + d] = a.start[(int64_t)(b0 + r) * D + d];
    }
  }
  // The keep flags of one step for this thread's elements of the [16][D] tile, in registers: keep95 is (C, S, B, D), so step
  // g = c S + s of this workgroup's rows starts at (g B + b0) D.
  constexpr int KPF = (16 * (FAST ? CHAIN_FAST_D : CHAIN_MAX_DIM) + NTHR - 1) / NTHR;
  uint32_t kreg[KPF] = {};
  auto load_keep = [&](int64_t g) {
    const uint8_t* k = a.keep95 + (g * B + b0) * D;
#pragma unroll
    for (int j = 0; j < KPF; ++j) {
      const int e = tid + j * NTHR;
      kreg[j] = (e < nrows * D) ? k[e] : 0;
    }
  };
  if (a.conditioned) load_keep(0);
  int p = 0;
  for (int c = 0; c < C; ++c) {
    // ---- the chunk's initial hidden state: row id of `rows`, [layer 0 | layer 1]; an id outside [0, R) reads nothing: zeros ----
    for (int e = tid; e < 16 * H; e += NTHR) {
      const int r = e / H, f = e - r * H;
      float v0 = 0.f, v1 = 0.f;
      if (r < nrows) {
        const int64_t id = a.ids ? a.ids[(int64_t)(b0 + r) * C + c] : (int64_t)(b0 + r) * C + c;
        if (id >= 0 && id < a.R) {
          const float* row = a.rows + id * 2 * H;
          v0 = row[f];
          v1 = row[H + f];
        }
      }
      Xh0[p][r * ldh + f] = v0;
      Xh1[p][r * ldh + f] = v1;
    }
    for (int e = tid; e < 16 * D; e += NTHR) {      // out[c, 0] = the carried frame
      const int r = e / D, d = e - r * D;
      if (r < nrows) a.out[((int64_t)(b0 + r) * F + (int64_t)c * T) * D + d] = Xc[r * ldd + d];
    }
    for (int s = 0; s < S; ++s) {
      // ---- xin = keep * input / 0.05 (the inline Dropout(0.95)); unconditioned: Xy stays zero ----
      if (a.conditioned) {
#pragma unroll
        for (int j = 0; j < KPF; ++j) {
          const int e = tid + j * NTHR;
          if (e < nrows * D) {
            const int r = e / D, d = e - r * D;
            Xy[r * ldd + d] = kreg[j] ? Xc[r * ldd + d] * 20.0f : 0.f;
          }
        }
        // the next step's flags: a fresh line from memory each step, requested a whole step ahead of its use
        const int64_t gn = (int64_t)c * S + s + 1;
        if (gn < (int64_t)C * S) load_keep(gn);
      }
      lds_barrier();
      // ---- a = ReLU(BatchNorm(pre_linear(xin))), folded ----
      if constexpr (FAST) {
        f32x4 acc[1] = {(f32x4){0.f, 0.f, 0.f, 0.f}};
        frag_mma(acc, f_pre, Xy, ldd, lane);
        const float b[4] = {bf4.x, bf4.y, bf4.z, bf4.w};
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(acc[0][r] + b[r], 0.f);
        *reinterpret_cast<float4*>(Xa + i * ldh + 16 * wave + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
      } else
      for (int ft = wave; ft < KSH; ft += NW) {
        f32x4 acc[1] = {(f32x4){0.f, 0.f, 0.f, 0.f}};
        wave_gemm_p<1, 0>(acc, pk.pre, KSD, ft, 0, Xy, ldd, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f = 16 * ft + 4 * q + r;
          if (f < H) Xa[i * ldh + f] = fmaxf(acc[0][r] + pk.bf[f], 0.f);
        }
      }
      lds_barrier();
      // ---- the two GRU cells (no inter-layer dropout in eval mode); no global outputs: nrows = 0 ----
      if constexpr (FAST) {
        auto cell = [&](const WFrag<3, FKSH>& fi, const WFrag<3, FKSH>& fh, const float4 (&bi)[3], const float4 (&bh)[3],
                        const float* Xin, const float* Xh, float* Xnew) {
          f32x4 ai[3], ah[3];
#pragma unroll
          for (int g = 0; g < 3; ++g) {
            ai[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
            ah[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
          }
          frag_mma(ai, fi, Xin, ldh, lane);
          frag_mma(ah, fh, Xh, ldh, lane);
          gru_cell_fwd_epilogue(ai, ah, bi, bh, 0x01010101u, false, 1.0f, Xh, ldh, H, Xnew, nullptr, nullptr, nullptr, 0, i,
                                16 * wave + 4 * q);
        };
        cell(f_ih0, f_hh0, bi0, bh0, Xa, Xh0[p], Xh0[p ^ 1]);
        lds_barrier();
        cell(f_ih1, f_hh1, bi1, bh1, Xh0[p ^ 1], Xh1[p], Xh1[p ^ 1]);
        lds_barrier();
      } else {
        gru_cell_fwd<0>(pk.ih0, pk.hh0, pk.bih0, pk.bhh0, Xa, Xh0[p], ldh, H, Hp, Xh0[p ^ 1], nullptr, nullptr, nullptr, 1.0f, nullptr,
                        0, lane, wave, NW, true);
        lds_barrier();
        gru_cell_fwd<0>(pk.ih1, pk.hh1, pk.bih1, pk.bhh1, Xh0[p ^ 1], Xh1[p], ldh, H, Hp, Xh1[p ^ 1], nullptr, nullptr, nullptr, 1.0f,
                        nullptr, 0, lane, wave, NW, true);
        lds_barrier();
      }
      p ^= 1;
      if (s < W) continue;      // a warm-up step: its output is discarded, so the out_layer is not run
      // ---- y_t = out_layer(h1_t); the next input ----
      const int t = s - W + 1;
      if constexpr (FAST) {
        f32x4 acc[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
        frag_mma(acc, f_out, Xh1[p], ldh, lane);
#pragma unroll
        for (int g = 0; g < 3; ++g) {
          const int d0 = 16 * (wave + 4 * g) + 4 * q;
          const float b[4] = {bo4[g].x, bo4[g].y, bo4[g].z, bo4[g].w};
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (d0 + r < D) Yt[i * ldd + d0 + r] = acc[g][r] + b[r];
        }
      } else
      for (int ft = wave; ft < KSD; ft += NW) {
        f32x4 acc[1] = {(f32x4){0.f, 0.f, 0.f, 0.f}};
        wave_gemm_p<1, 0>(acc, pk.out, KSH, ft, 0, Xh1[p], ldh, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int d = 16 * ft + 4 * q + r;
          if (d < D) Yt[i * ldd + d] = acc[0][r] + pk.bout[d];
        }
      }
      lds_barrier();
      const bool forced = a.teacher && t < a.n_pre;
      for (int e = tid; e < 16 * D; e += NTHR) {
        const int r = e / D, d = e - r * D;
        if (r >= nrows) continue;
        const float y = Yt[r * ldd + d];
        a.out[((int64_t)(b0 + r) * F + (int64_t)c * T + t) * D + d] = y;
        Xc[r * ldd + d] = forced ? a.teacher[(((int64_t)(b0 + r) * C + c) * T + t) * D + d] : y;
      }
    }
    if (!a.conditioned) {      // the reference's loop leaves a zero input behind
      for (int e = tid; e < 16 * D; e += NTHR) {
        const int r = e / D, d = e - r * D;
        if (r < nrows) Xc[r * ldd + d] = 0.f;
      }
    }
  }
  if (a.h_last) {
    for (int e = tid; e < 16 * H; e += NTHR) {
      const int r = e / H, f = e - r * H;
      if (r < nrows) {
        a.h_last[(int64_t)(b0 + r) * H + f] = Xh0[p][r * ldh + f];
        a.h_last[((int64_t)B + b0 + r) * H + f] = Xh1[p][r * ldh + f];
      }
    }
  }
}

static size_t chain_lds_bytes(int D, int H) {
  const int Hp = (H + 15) & ~15, Dp = (D + 15) & ~15;
  return ((size_t)5 * 16 * (Hp + 4) + (size_t)3 * 16 * (Dp + 4)) * sizeof(float);
}

// ---- the tail of a generated clip ---------------------------------------------------------------------------------------------
// blend + un-normalise, one thread per element of (B, F, Dr)
static __global__ __launch_bounds__(256) void clip_blend_kernel(const float* __restrict__ r, float* __restrict__ out,
                                                                const float* __restrict__ mean, const float* __restrict__ std,
                                                                int T, int n, int64_t total, int F, int Dr) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int d = (int)(e % Dr);
  const int f = (int)((e / Dr) % F);
  const int c = f / T, k = f - c * T;
  float v = r[e];
  if (n > 0 && c >= 1 && k < n) {
    const float prev = r[e - (int64_t)2 * k * Dr];      // frame o - k, o = c T
    v = __fadd_rn(__fdiv_rn(__fmul_rn(prev, (float)(n - k)), (float)(n + 1)), __fdiv_rn(__fmul_rn(v, (float)(k + 1)), (float)(n + 1)));
  }
  if (std) v = __fadd_rn(__fmul_rn(v, fmaxf(std[d], 0.01f)), mean[d]);
  out[e] = v;
}
// Savitzky-Golay along time from a host-made table: taps[25], then the edge matrices first[12][25] and last[12][25]
constexpr int SG_WIN = 25, SG_HALF = 12;
static __global__ __launch_bounds__(256) void clip_savgol_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                 const float* __restrict__ table, int64_t total, int F, int Dr) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int f = (int)((e / Dr) % F);
  const float* co;
  int f_first;
  if (f < SG_HALF) {
    co = table + SG_WIN + f * SG_WIN;
    f_first = 0;
  } else if (f >= F - SG_HALF) {
    co = table + SG_WIN + (SG_HALF + f - (F - SG_HALF)) * SG_WIN;
    f_first = F - SG_WIN;
  } else {
    co = table;
    f_first = f - SG_HALF;
  }
  const float* xs = x + e + (int64_t)(f_first - f) * Dr;
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < SG_WIN; ++k) acc = fmaf(co[k], xs[(int64_t)k * Dr], acc);
  out[e] = acc;
}

}  // namespace g2v

using namespace g2v;

extern "C" int g2v_dec_chain_ok(int C, int T, int warmup, int B, int D, int H) {
  return (C >= 1 && T >= 2 && warmup >= 0 && B >= 1 && D >= 1 && D <= CHAIN_MAX_DIM && H >= 1 && H <= CHAIN_MAX_DIM &&
          (int64_t)warmup + T - 1 <= (1 << 20) && C <= (1 << 20))
             ? 1
             : 0;
}

extern "C" size_t g2v_dec_chain_workspace(int D, int H) {
  if (D < 1 || H < 1 || D > CHAIN_MAX_DIM || H > CHAIN_MAX_DIM) return 0;
  return chain_layout(D, H).total * sizeof(float);
}

extern "C" int g2v_dec_chain_fwd(const float* rows, int64_t R, const int64_t* ids, const float* start, const float* teacher,
                                 const uint8_t* keep95, const g2v_dec_weights* w, float* out, float* h_last, int n_pre_poses,
                                 int conditioned, int C, int T, int warmup, int B, int D, int H, void* workspace,
                                 size_t workspace_bytes, g2v_stream_t stream) {
  G2V_REQUIRE(rows && w && out && workspace, "null pointer");
  G2V_REQUIRE(!conditioned || keep95, "a conditioned decoder needs keep95");
  G2V_REQUIRE(w->w_pre && w->b_pre && w->bn_w && w->bn_b && w->bn_running_mean && w->bn_running_var && w->w_ih0 && w->w_hh0 &&
                  w->b_ih0 && w->b_hh0 && w->w_ih1 && w->w_hh1 && w->b_ih1 && w->b_hh1 && w->w_out && w->b_out,
              "missing weight (eval mode needs the running statistics)");
  G2V_REQUIRE(R >= 1 && n_pre_poses >= 1, "bad size");
  if (!g2v_dec_chain_ok(C, T, warmup, B, D, H)) {
    set_error("g2v_dec_chain_fwd: g2v_dec_chain_ok(C, T, warmup, B, D, H) does not hold");
    return G2V_ERR_UNSUPPORTED;
  }
  G2V_REQUIRE(ids || (int64_t)B * C <= R, "without ids, rows must hold B * C rows");
  G2V_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "workspace: 16-byte alignment");
  if (workspace_bytes < g2v_dec_chain_workspace(D, H)) {
    set_error("g2v_dec_chain_fwd: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  float* base = static_cast<float*>(workspace);
  const ChainLayout l = chain_layout(D, H);
  ChainPackArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.pb.n = 6;
  pa.pb.d[0] = PackDesc{w->w_pre, base + l.pre, H, 1, 0, D, D, 0, 0};
  const float* gsrc[4] = {w->w_ih0, w->w_hh0, w->w_ih1, w->w_hh1};
  for (int k = 0; k < 4; ++k) pa.pb.d[1 + k] = PackDesc{gsrc[k], base + l.g[k], H, 3, H, H, H, 0, 0};
  pa.pb.d[5] = PackDesc{w->w_out, base + l.out, D, 1, 0, H, H, 0, chain_out_tiles(D)};
  pa.b_pre = w->b_pre; pa.bn_w = w->bn_w; pa.bn_b = w->bn_b; pa.rm = w->bn_running_mean; pa.rv = w->bn_running_var;
  pa.bf = base + l.bf;
  const float* bsrc[5] = {w->b_ih0, w->b_hh0, w->b_ih1, w->b_hh1, w->b_out};
  for (int k = 0; k < 5; ++k) {
    pa.bsrc[k] = bsrc[k];
    pa.bdst[k] = base + (k < 4 ? l.bg[k] : l.bout);
    pa.bn[k] = k < 4 ? 3 * H : D;
  }
  pa.H = H;
  pa.bout_pad = 16 * chain_out_tiles(D);
  hipLaunchKernelGGL(chain_pack_kernel, dim3(64, 7), dim3(256), 0, st, pa);
  G2V_CHECK_LAUNCH();

  ChainArgs a;
  a.rows = rows; a.ids = ids; a.start = start; a.teacher = teacher; a.keep95 = keep95; a.out = out; a.h_last = h_last;
  a.pk = ChainPack{base + l.pre, base + l.g[0], base + l.g[1], base + l.g[2], base + l.g[3], base + l.out, base + l.bf,
                   base + l.bg[0], base + l.bg[1], base + l.bg[2], base + l.bg[3], base + l.bout};
  a.R = R; a.n_pre = n_pre_poses; a.conditioned = conditioned; a.C = C; a.T = T; a.W = warmup; a.B = B; a.D = D; a.H = H;
  const size_t lds = chain_lds_bytes(D, H);
  const bool wide = ((H + 15) >> 4) > 4;      // more than four hidden-unit tiles: two waves per SIMD, as the generic step kernels
  const bool fast = H == CHAIN_FAST_H && D == CHAIN_FAST_D;
  const void* fn = fast ? (const void*)dec_chain_kernel<4, true>
                        : wide ? (const void*)dec_chain_kernel<8, false> : (const void*)dec_chain_kernel<4, false>;
  if (!g2v_internal_lds_reserve(fn, lds)) {
    set_error("g2v_dec_chain_fwd: %zu bytes of LDS refused", lds);
    return G2V_ERR_LAUNCH;
  }
  if (fast) hipLaunchKernelGGL((dec_chain_kernel<4, true>), dim3(cdiv(B, 16)), dim3(256), lds, st, a);
  else if (wide) hipLaunchKernelGGL((dec_chain_kernel<8, false>), dim3(cdiv(B, 16)), dim3(512), lds, st, a);
  else hipLaunchKernelGGL((dec_chain_kernel<4, false>), dim3(cdiv(B, 16)), dim3(256), lds, st, a);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int g2v_clip_finish(const float* r, float* out, const float* mean, const float* std, const float* savgol, float* tmp,
                               int T, int blend, int B, int F, int Dr, g2v_stream_t stream) {
  G2V_REQUIRE(r && out, "null pointer");
  G2V_REQUIRE(r != out, "in-place is not supported: the blend reads un-blended frames");
  G2V_REQUIRE((mean == nullptr) == (std == nullptr), "mean / std: both or neither");
  G2V_REQUIRE(B >= 1 && F >= 1 && Dr >= 1 && T >= 1 && blend >= 0 && F % T == 0, "bad size");
  G2V_REQUIRE(blend == 0 || T >= 2 * blend - 1, "the blend equals the reference's in-place loop only for T >= 2 * blend - 1");
  G2V_REQUIRE(!savgol || F >= SG_WIN, "the Savitzky-Golay filter needs at least 25 frames");
  G2V_REQUIRE(!savgol || (tmp && tmp != out && tmp != r), "the filter needs a (B, F, Dr) scratch array of its own");
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = (int64_t)B * F * Dr;
  G2V_REQUIRE(total <= (int64_t)0x7fffffff * 256, "too many elements");
  hipLaunchKernelGGL(clip_blend_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, r, savgol ? tmp : out, mean, std, T, blend, total,
                     F, Dr);
  G2V_CHECK_LAUNCH();
  if (savgol) {
    hipLaunchKernelGGL(clip_savgol_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, (const float*)tmp, out, savgol, total, F, Dr);
    G2V_CHECK_LAUNCH();
  }
  return G2V_OK;
}
