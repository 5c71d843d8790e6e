// tsne.hip -- exact t-SNE of (N, d) fp32 rows into the plane (gesture2vec_amd/embedding.py; the reference's codebook and latent maps:
// train_autoencoder_VQVAE.py:450-505, Clustering.py:1046-1056, sklearn.manifold.TSNE(method="exact")).  The math is sklearn 1.7's
// (sklearn.manifold._t_sne / _utils._binary_search_perplexity); the N x N joint P is dense fp32 with row stride N.
//
// g2v_tsne_affinities
//   tsne_pad_kernel     x -> xp (N, E4 = d rounded up to 4, zero filled): rows 16-byte aligned whatever d and ld are
//   pd_norm_kernel      |x_i|^2 in float64 (pair_dist.hpp)
//   tsne_dist_kernel    one workgroup (4 waves) per 64 x 64 tile of D = squared Euclidean distances, written into P: pd_tile
//                       (pair_dist.hpp, which states the arithmetic and its error) over the padded copy, the row set against
//                       itself.  A bitwise equal pair has d^2 = 0 exactly, the diagonal is 0 by rule, and D[i][j] == D[j][i] bit
//                       for bit.  Rows far from the origin should be centred first (embedding.PCA does): |G| is then small
//                       wherever the pair is not near.
//   tsne_search_kernel  one workgroup per row i, the row of D staged in LDS (N * 4 B <= 128 KiB beside the reduction scratch: every
//                       supported N fits, so there is no path that re-reads the row from global memory).  sklearn's bisection of the
//                       precision beta in float64 (tsne_cells.hpp), the sums over the block, the term j = i left out.  The row is
//                       overwritten with c_j|i = exp(-beta d^2) / sum as fp32; the float64 sum of those fp32 values goes to rowsum[i].
//   tsne_total_kernel   sigma = max(2 sum_i rowsum[i], eps) (= sum (C + C^T); one workgroup, rows dealt by index, fixed tree)
//   tsne_sym_kernel     P_ij = max((c_ij + c_ji) / sigma, eps) in float64, rounded to fp32, in place: the workgroup of tile (a, b),
//                       a <= b, owns tiles (a, b) and (b, a), both through LDS.  eps = DBL_EPSILON, as sklearn's MACHINE_EPSILON.
// g2v_tsne_gradient     q_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} q_ij, p_ij = exaggeration * P_ij,
//                       grad_i = 4 sum_j (p_ij - q_ij / Z) q_ij (y_i - y_j),  KL = sum_{i != j} p_ij log(max(p_ij, eps) / (q_ij / Z))
//   tsne_sweep_kernel   ONE pass over P: a wave owns two rows and walks the columns 64 at a time (four column groups in flight), the y
//                       of 2048 columns at a time in LDS.  y_i - y_j and q in fp32 (q within 2 ulp); the attractive sum
//                       sum p q (y_i - y_j), the repulsive sum sum q^2 (y_i - y_j), sum q, and with want_kl
//                       sum p (log max(p, eps) - log q) and sum p accumulate SEPARATELY in float64 per lane, then over the wave in
//                       a fixed xor tree: Z is not known during the sweep.  (sklearn clamps q / Z at eps inside the gradient and the
//                       KL as well; that needs Z and changes a term by < eps q, below float64 resolution of the sums: left out.)
//   tsne_finish_kernel  one workgroup: Z and KL = A + log(Z) S_p in a fixed order, then grad_i = 4 (att_i - rep_i / Z) as fp32 and the
//                       float64 sum of the squared fp32 gradients.  out = { KL (NaN without want_kl, as sklearn), sum grad^2, Z }
// g2v_tsne_update       sklearn's _gradient_descent step per component (tsne_cells.hpp: ts_step); gnorm2 (may be NULL) = float64
//                       sum of (gains grad)^2, the norm sklearn's stop rule reads.
// Every sum is formed in an order fixed by (N, d): no floating-point atomics, the same input gives the same bits.  All offsets into P
// are 64-bit; N <= 32768 (4 GiB of P), G2V_ERR_UNSUPPORTED beyond.  No environment variable is read.
#include <float.h>

#include "common.hpp"
#include "km_sort.hpp"
#include "pair_dist.hpp"
#include "tsne_cells.hpp"

namespace g2v {
namespace {

constexpr int64_t TSNE_MAX_N = 32768;
constexpr int TSNE_MAX_D = 512;
constexpr int TS_YCH = 2048;                // columns of y per LDS stage of the sweep
constexpr int TS_SWEEP_ROWS = 8;            // rows per workgroup of the sweep (2 per wave)
constexpr int TS_PART = 8;                  // doubles per row of the sweep's partials

struct TsneLayout {
  int E4;
  size_t xp, norm, rowsum, sigma, total;
};

inline TsneLayout tsne_layout(int64_t N, int d) {
  TsneLayout l;
  l.E4 = (d + 3) & ~3;
  size_t o = 0;
  l.xp = o;      o = km_align(o + (size_t)N * l.E4 * sizeof(float));
  l.norm = o;    o = km_align(o + (size_t)N * sizeof(double));
  l.rowsum = o;  o = km_align(o + (size_t)N * sizeof(double));
  l.sigma = o;   o = km_align(o + sizeof(double));
  l.total = o;
  return l;
}

__global__ __launch_bounds__(256) void tsne_pad_kernel(const float* __restrict__ x, int64_t ld, int64_t N, int d, int E4,
                                                      float* __restrict__ xp) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= N * E4) return;
  const int64_t r = e / E4;
  const int k = (int)(e - r * E4);
  xp[e] = k < d ? x[r * ld + k] : 0.f;
}

__global__ __launch_bounds__(256) void tsne_dist_kernel(const float* __restrict__ xp, int E4, int N, const double* __restrict__ norm,
                                                       float* __restrict__ D) {
  __shared__ __attribute__((aligned(16))) float sa[PD_TILE * PD_LD];
  __shared__ __attribute__((aligned(16))) float sb[PD_TILE * PD_LD];
  __builtin_assume((E4 & 3) == 0);                            // (the padded copy, d = E4: none of pd_tile's loads is masked)
  const int64_t i0 = (int64_t)blockIdx.y * PD_TILE;
  double nr[4];
  pd_row_norms(norm, N, i0, nr);
  pd_tile(xp, E4, N, i0, nr, xp, E4, N, (int)blockIdx.x * PD_TILE, norm, E4, true, sa, sb,
          [&](int64_t row, int col, const float (&dd)[4]) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (row + r < N && col < N) D[(row + r) * N + col] = dd[r];
          });
}

// sum of (a, b) over the 256 threads in a fixed tree; every thread returns the same bits.  sh: 8 doubles
__device__ __forceinline__ void ts_block_sum2(double& a, double& b, double* sh) {
  a = km_wave_sum(a);
  b = km_wave_sum(b);
  const int w = threadIdx.x >> 6;
  __syncthreads();                                            // sh may still be read from the previous call
  if ((threadIdx.x & 63) == 0) {
    sh[w] = a;
    sh[4 + w] = b;
  }
  __syncthreads();
  a = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  b = (sh[4] + sh[5]) + (sh[6] + sh[7]);
}

// dynamic LDS: the row of D (N floats)
__global__ __launch_bounds__(256) void tsne_search_kernel(float* __restrict__ P, int N, double log_perp, double* __restrict__ rowsum) {
  extern __shared__ __attribute__((aligned(16))) float drow[];
  __shared__ double sh[8];
  const int tid = threadIdx.x, i = blockIdx.x;
  float* prow = P + (int64_t)i * N;
  for (int j = tid; j < N; j += 256) drow[j] = prow[j];
  __syncthreads();

  TsBisect bs;
  for (int step = 0; step < TS_BISECT_STEPS; ++step) {
    double s0 = 0.0, s1 = 0.0;
    for (int j = tid; j < N; j += 256) {
      if (j != i) {
        const double dj = (double)drow[j];
        const double e = exp(-dj * bs.beta);
        s0 += e;
        s1 = fma(dj, e, s1);
      }
    }
    ts_block_sum2(s0, s1, sh);
    if (ts_bisect_next(bs, s0, s1, log_perp)) break;          // (uniform: every thread holds the same bits)
  }
  double rs = 0.0, unused = 0.0;
  for (int j = tid; j < N; j += 256) {
    float c = 0.f;
    if (j != i) c = (float)(exp(-(double)drow[j] * bs.beta_eval) / bs.sum_p);
    prow[j] = c;
    rs += (double)c;
  }
  ts_block_sum2(rs, unused, sh);
  if (tid == 0) rowsum[i] = rs;
}

__global__ __launch_bounds__(1024) void tsne_total_kernel(const double* __restrict__ rowsum, int N, double* __restrict__ sigma) {
  __shared__ double sh[1024];
  double acc = 0.0;
  for (int n = threadIdx.x; n < N; n += 1024) acc += rowsum[n];
  const double tot = km_block_sum(acc, sh);
  if (threadIdx.x == 0) sigma[0] = fmax(2.0 * tot, DBL_EPSILON);
}

__global__ __launch_bounds__(256) void tsne_sym_kernel(float* __restrict__ P, int N, const double* __restrict__ sigma) {
  __shared__ float ta[PD_TILE][PD_TILE + 1];
  __shared__ float tb[PD_TILE][PD_TILE + 1];
  const int a = blockIdx.y, b = blockIdx.x;
  if (a > b) return;
  const int i0 = a * PD_TILE, j0 = b * PD_TILE;
  const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
  const double sg = sigma[0];
  for (int r = r0; r < PD_TILE; r += 4) {
    ta[r][c] = (i0 + r < N && j0 + c < N) ? P[(int64_t)(i0 + r) * N + j0 + c] : 0.f;
    tb[r][c] = (j0 + r < N && i0 + c < N) ? P[(int64_t)(j0 + r) * N + i0 + c] : 0.f;
  }
  __syncthreads();
  for (int r = r0; r < PD_TILE; r += 4) {
    if (i0 + r < N && j0 + c < N) {
      const double v = ((double)ta[r][c] + (double)tb[c][r]) / sg;
      P[(int64_t)(i0 + r) * N + j0 + c] = (i0 + r == j0 + c) ? 0.f : (float)fmax(v, DBL_EPSILON);
    }
    if (a != b && j0 + r < N && i0 + c < N) {
      const double v = ((double)ta[c][r] + (double)tb[r][c]) / sg;
      P[(int64_t)(j0 + r) * N + i0 + c] = (float)fmax(v, DBL_EPSILON);
    }
  }
}

// part[row][TS_PART] = { att_x, att_y, rep_x, rep_y, sum q, sum p (log max(p, eps) - log q), sum p, - }
__global__ __launch_bounds__(256) void tsne_sweep_kernel(const float* __restrict__ P, const float* __restrict__ y, int N, double exag,
                                                        int want_kl, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float2 ys[TS_YCH];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row_a = blockIdx.x * TS_SWEEP_ROWS + 2 * wave;
  const float2* y2 = reinterpret_cast<const float2*>(y);
  int rows[2];
  float2 yi[2];
  const float* prow[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    rows[h] = row_a + h;
    const int rc = min(rows[h], N - 1);                       // (a row past the end reads row N - 1 and is not written)
    yi[h] = y2[rc];
    prow[h] = P + (int64_t)rc * N;
  }
  double att_x[2] = {0.0, 0.0}, att_y[2] = {0.0, 0.0}, rep_x[2] = {0.0, 0.0}, rep_y[2] = {0.0, 0.0}, zq[2] = {0.0, 0.0},
         kla[2] = {0.0, 0.0}, sp[2] = {0.0, 0.0};

  for (int c0 = 0; c0 < N; c0 += TS_YCH) {
    __syncthreads();
    for (int c = tid; c < TS_YCH; c += 256) ys[c] = c0 + c < N ? y2[c0 + c] : make_float2(0.f, 0.f);
    __syncthreads();
    const int cend = min(TS_YCH, N - c0);
    for (int cb = 0; cb < cend; cb += 256) {
      float pv[2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int c = cb + 64 * u + lane;
          pv[h][u] = c < cend ? prow[h][c0 + c] : 0.f;
        }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = cb + 64 * u + lane;
        if (c < cend) {
          const float2 yj = ys[c];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const float dx = yi[h].x - yj.x, dy = yi[h].y - yj.y;
            const float q = ts_q(dx, dy);
            const double qd = (double)q, p = exag * (double)pv[h][u];
            const double wa = p * qd, wr = qd * qd;
            att_x[h] = fma(wa, (double)dx, att_x[h]);
            att_y[h] = fma(wa, (double)dy, att_y[h]);
            rep_x[h] = fma(wr, (double)dx, rep_x[h]);
            rep_y[h] = fma(wr, (double)dy, rep_y[h]);
            if (c0 + c != rows[h]) zq[h] += qd;
            if (want_kl) {
              kla[h] = fma(p, log(fmax(p, DBL_EPSILON)) - log(qd), kla[h]);
              sp[h] += p;
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const double v[7] = {km_wave_sum(att_x[h]), km_wave_sum(att_y[h]), km_wave_sum(rep_x[h]), km_wave_sum(rep_y[h]),
                         km_wave_sum(zq[h]),    km_wave_sum(kla[h]),   km_wave_sum(sp[h])};
    if (lane == 0 && rows[h] < N) {
      double* o = part + (int64_t)rows[h] * TS_PART;
#pragma unroll
      for (int k = 0; k < 7; ++k) o[k] = v[k];
      o[7] = 0.0;
    }
  }
}

__global__ __launch_bounds__(1024) void tsne_finish_kernel(const double* __restrict__ part, int N, int want_kl, float* __restrict__ grad,
                                                          double* __restrict__ out) {
  __shared__ double sh[1024];
  __shared__ double tot[3];
  const int tid = threadIdx.x;
  double z = 0.0, a = 0.0, s = 0.0;
  for (int n = tid; n < N; n += 1024) {
    const double* p = part + (int64_t)n * TS_PART;
    z += p[4];
    a += p[5];
    s += p[6];
  }
  const double zt = km_block_sum(z, sh);
  if (tid == 0) tot[0] = zt;
  __syncthreads();
  const double at = km_block_sum(a, sh);
  if (tid == 0) tot[1] = at;
  __syncthreads();
  const double st = km_block_sum(s, sh);
  if (tid == 0) tot[2] = st;
  __syncthreads();
  const double Z = fmax(tot[0], DBL_EPSILON);
  double g2 = 0.0;
  for (int n = tid; n < N; n += 1024) {
    const double* p = part + (int64_t)n * TS_PART;
    const float gx = (float)(4.0 * (p[0] - p[2] / Z)), gy = (float)(4.0 * (p[1] - p[3] / Z));
    grad[2 * n] = gx;
    grad[2 * n + 1] = gy;
    g2 = fma((double)gx, (double)gx, g2);
    g2 = fma((double)gy, (double)gy, g2);
  }
  const double g2t = km_block_sum(g2, sh);
  if (tid == 0) {
    out[0] = want_kl ? tot[1] + log(Z) * tot[2] : __builtin_nan("");
    out[1] = g2t;
    out[2] = tot[0];
  }
}

__global__ __launch_bounds__(1024) void tsne_update_kernel(float* __restrict__ y, float* __restrict__ vel, float* __restrict__ gains,
                                                          const float* __restrict__ grad, int64_t n, float momentum, float lr,
                                                          double* __restrict__ gnorm2) {
  __shared__ double sh[1024];
  double acc = 0.0;
  for (int64_t e = threadIdx.x; e < n; e += 1024) {
    float ye = y[e], v = vel[e], gn = gains[e];
    const float gg = ts_step(grad[e], momentum, lr, ye, v, gn);
    gains[e] = gn;
    vel[e] = v;
    y[e] = ye;
    acc = fma((double)gg, (double)gg, acc);
  }
  if (gnorm2) {                                               // (uniform)
    const double t = km_block_sum(acc, sh);
    if (threadIdx.x == 0) gnorm2[0] = t;
  }
}

inline int tsne_rows_ok(const char* fn, int64_t N) {
  if (N > TSNE_MAX_N) {
    set_error("%s: N = %lld rows; the dense N x N joint is built for N <= %lld", fn, (long long)N, (long long)TSNE_MAX_N);
    return G2V_ERR_UNSUPPORTED;
  }
  return G2V_OK;
}

}  // namespace
}  // namespace g2v

using namespace g2v;

extern "C" int64_t g2v_tsne_max_rows(void) { return TSNE_MAX_N; }

extern "C" size_t g2v_tsne_affinities_workspace(int64_t N, int d) {
  if (N < 2 || N > TSNE_MAX_N || d < 1 || d > TSNE_MAX_D) return 0;
  return tsne_layout(N, d).total;
}

extern "C" int g2v_tsne_affinities(const float* x, int64_t ld, int64_t N, int d, double perplexity, float* P, void* workspace,
                                   size_t workspace_bytes, g2v_stream_t stream) {
  G2V_REQUIRE(x && P && workspace, "null pointer");
  G2V_REQUIRE(N >= 2 && d >= 1, "sizes: N >= 2, d >= 1");
  if (const int rc = tsne_rows_ok(__func__, N)) return rc;
  if (d > TSNE_MAX_D) {
    set_error("g2v_tsne_affinities: needs d <= %d (d = %d)", TSNE_MAX_D, d);
    return G2V_ERR_UNSUPPORTED;
  }
  G2V_REQUIRE(ld >= d && (ld & 3) == 0, "row stride smaller than d or not a multiple of 4");
  G2V_REQUIRE(perplexity > 0.0 && perplexity < (double)N, "perplexity must be in (0, N)");
  G2V_REQUIRE((reinterpret_cast<uintptr_t>(P) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
              "P and workspace must be 16-byte aligned");
  const TsneLayout l = tsne_layout(N, d);
  if (workspace_bytes < l.total) {
    set_error("g2v_tsne_affinities: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  if (!g2v_internal_lds_reserve((const void*)tsne_search_kernel, (size_t)N * sizeof(float))) {
    set_error("g2v_tsne_affinities: cannot reserve LDS");
    return G2V_ERR_LAUNCH;
  }
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* xp = (float*)(ws + l.xp);
  double* norm = (double*)(ws + l.norm);
  double* rowsum = (double*)(ws + l.rowsum);
  double* sigma = (double*)(ws + l.sigma);
  const int n = (int)N, T = cdiv(N, PD_TILE);
  hipLaunchKernelGGL(tsne_pad_kernel, dim3(cdiv(N * l.E4, 256)), dim3(256), 0, st, x, ld, N, d, l.E4, xp);
  hipLaunchKernelGGL(pd_norm_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, (const float*)xp, (int64_t)l.E4, N, l.E4, norm);
  hipLaunchKernelGGL(tsne_dist_kernel, dim3(T, T), dim3(256), 0, st, (const float*)xp, l.E4, n, (const double*)norm, P);
  hipLaunchKernelGGL(tsne_search_kernel, dim3(n), dim3(256), (size_t)N * sizeof(float), st, P, n, log(perplexity), rowsum);
  hipLaunchKernelGGL(tsne_total_kernel, dim3(1), dim3(1024), 0, st, (const double*)rowsum, n, sigma);
  hipLaunchKernelGGL(tsne_sym_kernel, dim3(T, T), dim3(256), 0, st, P, n, (const double*)sigma);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" size_t g2v_tsne_gradient_workspace(int64_t N) {
  if (N < 2 || N > TSNE_MAX_N) return 0;
  return km_align((size_t)N * TS_PART * sizeof(double));
}

extern "C" int g2v_tsne_gradient(const float* P, const float* y, int64_t N, double exaggeration, int want_kl, float* grad, double* out,
                                 void* workspace, size_t workspace_bytes, g2v_stream_t stream) {
  G2V_REQUIRE(P && y && grad && out && workspace, "null pointer");
  G2V_REQUIRE(N >= 2, "sizes: N >= 2");
  if (const int rc = tsne_rows_ok(__func__, N)) return rc;
  G2V_REQUIRE(exaggeration > 0.0, "exaggeration must be positive");
  G2V_REQUIRE((reinterpret_cast<uintptr_t>(y) & 7) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
              "y must be 8-byte and workspace 16-byte aligned");
  if (workspace_bytes < g2v_tsne_gradient_workspace(N)) {
    set_error("g2v_tsne_gradient: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  hipLaunchKernelGGL(tsne_sweep_kernel, dim3(cdiv(N, TS_SWEEP_ROWS)), dim3(256), 0, st, P, y, (int)N, exaggeration, want_kl ? 1 : 0,
                     part);
  hipLaunchKernelGGL(tsne_finish_kernel, dim3(1), dim3(1024), 0, st, (const double*)part, (int)N, want_kl ? 1 : 0, grad, out);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int g2v_tsne_update(float* y, float* velocity, float* gains, const float* grad, int64_t N, float momentum,
                               float learning_rate, double* gnorm2, g2v_stream_t stream) {
  G2V_REQUIRE(y && velocity && gains && grad, "null pointer");
  G2V_REQUIRE(N >= 1, "sizes: N >= 1");
  if (const int rc = tsne_rows_ok(__func__, N)) return rc;
  hipLaunchKernelGGL(tsne_update_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, y, velocity, gains, grad, 2 * N, momentum,
                     learning_rate, gnorm2);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
