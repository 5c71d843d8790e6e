// softdtw.hip -- soft-DTW (Cuturi & Blondel 2017) between (N, T, F) fp32 series and float64 centres: the values and their argmin, the
// soft alignment matrices against one centre, and value and gradient of a barycentre objective: what gesture2vec_amd/timeseries.py
// builds tslearn's TimeSeriesKMeans(metric="softdtw") from (the reference's Clustering.py:670-691).  The definitions are in
// include/g2v.h.  Everything is float64.  The cost tile, the grouping rule and the argmin are the DTW ones (dtw_tile.hpp).
//
// The tile's rows are the series (t, the header's j) and its lanes the centre (s, the header's i), as in dtw.hip.
//   forward   the T + S - 1 anti-diagonals in order: lane s takes cell (s, t = d - s).  R(s, t-1) is the lane's own last value,
//             R(s-1, t) the left neighbour's last value (one __shfl_up), R(s-1, t-1) the one it sent a diagonal earlier; lanes outside
//             the tile hold +inf, whose exponent term is exp(-inf) = 0: an absent predecessor contributes nothing, and since every
//             cell but (0, 0) has a finite predecessor, m is finite and -inf never meets +inf.  R stays in registers (KEEP: it is
//             also stored in a second LDS tile).
//   backward  the anti-diagonals in reverse: E(s, t+1) is the lane's own last value, E(s+1, t) the right neighbour's (one
//             __shfl_down), E(s+1, t+1) the one it sent a diagonal earlier; lanes outside the tile hold 0.  R and the cost of the three
//             successors come from the two LDS tiles: neighbouring lanes of a diagonal are 63 doubles apart, an odd stride.
//
//   softdtw_pair_kernel   one workgroup per (n, group of G centres): v[n][m] = sdtw(y_m, x_n); then dtw_argmin_kernel
//   softdtw_align_kernel  one wave per member row r: cost tile, forward with R kept, backward -> E_r (strided: (S, T) for the caller,
//                         (T, S) in the workspace, where the lanes of a diagonal write next to each other), value_r
//   softdtw_slab_kernel   grid (slab, s), threads over f: the slab's members in order, per member sum_t E(s, t) x[t][f] (t ascending,
//                         fused) and sum_t E(s, t), each added times w -> part[slab][s][f], partr[slab][s]; the block of s == 0 adds
//                         w value -> partv[slab]
//   softdtw_fold_kernel   grid (s): the slabs in slab order -> G[s][f] = 2 (z[s][f] rsum - A[s][f]); the block of s == 0: obj
// SDTW_SLAB is a constant, so the order of every sum is a function of `rows` alone: the same bits on every call.  No
// floating-point atomics, no workgroup waits on another.
#include "common.hpp"
#include "dtw_tile.hpp"

namespace g2v {
namespace {

constexpr int SDTW_SLAB = 128;              // member rows per partial sum

inline size_t sdtw_align(size_t v) { return (v + 255) & ~(size_t)255; }
// the cost tile, the series slice, then the R tile
inline size_t sdtw_lds_bytes(int T) { return dtw_lds_bytes(T) + (size_t)T * 64 * sizeof(double); }

struct SdtwLayout {
  int64_t slabs;
  size_t v, E, value, part, partr, partv, total;
};

// N rows (member rows for the gradient) against M centres
inline SdtwLayout sdtw_layout(int64_t N, int64_t M, int T, int S, int F) {
  SdtwLayout l;
  l.slabs = (N + SDTW_SLAB - 1) / SDTW_SLAB;
  size_t o = 0;
  l.v = 0;                                                   // (the values of a cdist call lie over the gradient's blocks)
  l.E = o;      o = sdtw_align(o + (size_t)N * S * T * sizeof(double));
  l.value = o;   o = sdtw_align(o + (size_t)N * sizeof(double));
  l.part = o;    o = sdtw_align(o + (size_t)l.slabs * S * F * sizeof(double));
  l.partr = o;   o = sdtw_align(o + (size_t)l.slabs * S * sizeof(double));
  l.partv = o;   o = sdtw_align(o + (size_t)l.slabs * sizeof(double));
  const size_t vb = sdtw_align((size_t)N * M * sizeof(double));
  l.total = o > vb ? o : vb;
  return l;
}

// the header's softmin, its three terms added in the header's order
__device__ __forceinline__ double sdtw_softmin(double a, double b, double c, double gamma) {
  const double ap = -a / gamma, bp = -b / gamma, cp = -c / gamma;
  const double m = fmax(ap, fmax(bp, cp));
  const double s = exp(ap - m) + exp(bp - m) + exp(cp - m);
  return -gamma * (log(s) + m);
}

// The forward sweep over the cost tile; s the lane's centre row, `col` whether the lane owns a column of the tile.  Returns the lane's
// last R: sdtw in the lane of row S - 1.  KEEP: rt[t * 64 + lane] = R(s, t).  Every lane of the wave must call it.
template <bool KEEP>
__device__ __forceinline__ double sdtw_forward(const double* tile, double* rt, bool col, int s, int T, int S, double gamma) {
  const int lane = threadIdx.x;
  const double inf = (double)__builtin_inff();
  double cur = inf, left = inf;
  for (int d = 0; d < T + S - 1; ++d) {
    const double diag = left;                                // R(s-1, t-1): what the left neighbour held two diagonals ago
    const double up = cur;                                   // R(s, t-1)
    left = __shfl_up(cur, 1);                                // R(s-1, t)
    if (s == 0) left = inf;
    const int t = d - s;
    if (col && t >= 0 && t < T) {
      const double c = tile[t * 64 + lane];
      cur = (s == 0 && t == 0) ? c : c + sdtw_softmin(left, diag, up, gamma);
      if (KEEP) rt[t * 64 + lane] = cur;
    } else {
      cur = inf;
    }
  }
  return cur;
}

__global__ __launch_bounds__(64) void softdtw_pair_kernel(const float* __restrict__ x, int T, const double* __restrict__ y, int64_t M,
                                                         int S, int F, int P, int MB, double gamma, double* __restrict__ v) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sdtw_lds[];
  double* tile = reinterpret_cast<double*>(sdtw_lds);
  float* as = reinterpret_cast<float*>(sdtw_lds + (size_t)T * 64 * sizeof(double));
  const int lane = threadIdx.x;
  const int64_t n = blockIdx.x / MB;                         // (the centres fastest: neighbouring workgroups share a series)
  const int64_t m = (int64_t)(blockIdx.x % MB) * (64 / P) + lane / P;
  const int j = lane % P;
  const bool active = m < M && j < S;
  const double* b = y + ((size_t)(active ? m : 0) * S + (active ? j : 0)) * F;
  dtw_cost_tile(x + (size_t)n * T * F, b, active, T, F, tile, as);
  const double r = sdtw_forward<false>(tile, nullptr, active, j, T, S, gamma);
  if (active && j == S - 1) v[n * M + m] = r;
}

// rows == nullptr: member r is row r of x.  E_r[s][t] at E + r * es_r + s * es_s + t * es_t.
__global__ __launch_bounds__(64) void softdtw_align_kernel(const float* __restrict__ x, int64_t N, int T, const int64_t* __restrict__ rows,
                                                          const double* __restrict__ z, int S, int F, double gamma,
                                                          double* __restrict__ value, double* __restrict__ E, size_t es_r, size_t es_s,
                                                          size_t es_t) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sdtw_lds[];
  double* tile = reinterpret_cast<double*>(sdtw_lds);
  float* as = reinterpret_cast<float*>(sdtw_lds + (size_t)T * 64 * sizeof(double));
  double* rt = reinterpret_cast<double*>(as + (size_t)T * DTW_FC);          // (at dtw_lds_bytes(T))
  const int lane = threadIdx.x, s = lane;
  const int64_t r = blockIdx.x;
  const int64_t n = rows ? rows[r] : r;
  const bool col = s < S;
  double* Er = E + (size_t)r * es_r;
  if (n < 0 || n >= N) {                                     // (workgroup-uniform) an id outside contributes nothing
    if (col)
      for (int t = 0; t < T; ++t) Er[s * es_s + t * es_t] = 0.0;
    if (lane == 0) value[r] = 0.0;
    return;
  }
  dtw_cost_tile(x + (size_t)n * T * F, z + (size_t)(col ? s : 0) * F, col, T, F, tile, as);
  const double last = sdtw_forward<true>(tile, rt, col, s, T, S, gamma);
  if (s == S - 1) value[r] = last;
  __syncthreads();
  double cur = 0.0, right = 0.0;
  for (int d = T + S - 2; d >= 0; --d) {
    const double dg = right;                                 // E(s+1, t+1): what the right neighbour held two diagonals ago
    const double down = cur;                                 // E(s, t+1)
    right = __shfl_down(cur, 1);                             // E(s+1, t)
    if (s + 1 >= S) right = 0.0;
    const int t = d - s;
    if (col && t >= 0 && t < T) {
      double e = 1.0;
      if (d != T + S - 2) {
        const bool hs = s + 1 < S, ht = t + 1 < T;
        const double r0 = rt[t * 64 + lane];
        e = 0.0;                                             // the header's order: a, b, c
        if (hs) e = right * exp((rt[t * 64 + lane + 1] - r0 - tile[t * 64 + lane + 1]) / gamma);
        if (ht) e += down * exp((rt[(t + 1) * 64 + lane] - r0 - tile[(t + 1) * 64 + lane]) / gamma);
        if (hs && ht) e += dg * exp((rt[(t + 1) * 64 + lane + 1] - r0 - tile[(t + 1) * 64 + lane + 1]) / gamma);
      }
      cur = e;
      Er[s * es_s + t * es_t] = e;
    } else {
      cur = 0.0;
    }
  }
}

__global__ __launch_bounds__(256) void softdtw_slab_kernel(const float* __restrict__ x, int64_t N, int T, int S, int F,
                                                          const int64_t* __restrict__ rows, int64_t R, const double* __restrict__ w,
                                                          const double* __restrict__ E, const double* __restrict__ value,
                                                          double* __restrict__ part, double* __restrict__ partr,
                                                          double* __restrict__ partv) {
  const int64_t c = blockIdx.x;
  const int s = (int)blockIdx.y;
  const int64_t start = c * SDTW_SLAB;
  const int len = (int)(R - start < SDTW_SLAB ? R - start : SDTW_SLAB);
  const int tid = threadIdx.x;
  double acc[2] = {0.0, 0.0};                                // columns tid and tid + 256
  double accr = 0.0, accv = 0.0;
  for (int q = 0; q < len; ++q) {
    const int64_t r = start + q;
    const int64_t n = rows[r];
    const double wr = w ? w[r] : 1.0;
    if (s == 0 && tid == 0) accv = fma(wr, value[r], accv);
    if (n < 0 || n >= N) continue;                           // (its E and value are 0)
    const float* xr = x + (size_t)n * T * F;
    const double* Er = E + ((size_t)r * T) * S + s;          // the workspace's layout: (T, S)
    double a0 = 0.0, a1 = 0.0, rs = 0.0;
    for (int t = 0; t < T; ++t) {
      const double e = Er[(size_t)t * S];
      rs += e;
      if (tid < F) a0 = fma(e, (double)xr[(size_t)t * F + tid], a0);
      if (tid + 256 < F) a1 = fma(e, (double)xr[(size_t)t * F + tid + 256], a1);
    }
    acc[0] = fma(wr, a0, acc[0]);
    acc[1] = fma(wr, a1, acc[1]);
    accr = fma(wr, rs, accr);
  }
  double* p = part + ((size_t)c * S + s) * F;
  if (tid < F) p[tid] = acc[0];
  if (tid + 256 < F) p[tid + 256] = acc[1];
  if (tid == 0) {
    partr[(size_t)c * S + s] = accr;
    if (s == 0) partv[c] = accv;
  }
}

__global__ __launch_bounds__(256) void softdtw_fold_kernel(int S, int F, int64_t slabs, const double* __restrict__ z,
                                                          const double* __restrict__ part, const double* __restrict__ partr,
                                                          const double* __restrict__ partv, double* __restrict__ value,
                                                          double* __restrict__ grad) {
  const int s = (int)blockIdx.x;
  double rsum = 0.0;                                         // (every thread adds the same values in the same order)
  for (int64_t c = 0; c < slabs; ++c) rsum += partr[(size_t)c * S + s];
  for (int f = threadIdx.x; f < F; f += 256) {
    double a = 0.0;
    for (int64_t c = 0; c < slabs; ++c) a += part[((size_t)c * S + s) * F + f];
    grad[(size_t)s * F + f] = 2.0 * (z[(size_t)s * F + f] * rsum - a);
  }
  if (s == 0 && threadIdx.x == 0) {
    double v = 0.0;
    for (int64_t c = 0; c < slabs; ++c) v += partv[c];
    value[0] = v;
  }
}

int sdtw_refuse(const char* fn, int64_t N, int64_t M, int T, int S, int F) {
  set_error("%s: needs 1 <= T, S <= %d, 1 <= F <= %d and fewer than 2^31 series and centres (N = %lld, M = %lld, T = %d, S = %d, F = %d)",
            fn, DTW_MAX_LEN, DTW_MAX_F, (long long)N, (long long)M, T, S, F);
  return G2V_ERR_UNSUPPORTED;
}

inline bool sdtw_gamma_ok(double gamma) { return gamma > 0.0 && gamma <= 1.7976931348623157e308; }     // (false for NaN)

}  // namespace
}  // namespace g2v

using namespace g2v;

extern "C" size_t g2v_softdtw_workspace(int64_t N, int64_t M, int T, int S, int F) {
  if (!dtw_shape_ok(N, M, T, S, F)) return 0;
  return sdtw_layout(N, M, T, S, F).total;
}

extern "C" int g2v_softdtw_cdist(const float* x, int64_t N, int T, const double* y, int64_t M, int S, int F, double gamma, double* out,
                                 int64_t* labels, double* best, void* workspace, size_t workspace_bytes, g2v_stream_t stream) {
  G2V_REQUIRE(x && y && workspace, "null pointer");
  G2V_REQUIRE((labels == nullptr) == (best == nullptr), "labels and best are given together or not at all");
  G2V_REQUIRE(out || labels, "nothing to write: out, labels and best are all null");
  G2V_REQUIRE(N >= 1 && M >= 1 && T >= 1 && S >= 1 && F >= 1, "sizes: N, M, T, S, F >= 1");
  G2V_REQUIRE(sdtw_gamma_ok(gamma), "gamma must be finite and > 0");
  if (!dtw_shape_ok(N, M, T, S, F)) return sdtw_refuse("g2v_softdtw_cdist", N, M, T, S, F);
  G2V_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "workspace must be 16-byte aligned");
  const int P = dtw_group_width(S), MB = cdiv(M, 64 / P);
  G2V_REQUIRE(N * MB <= 0x7fffffff, "N * M exceeds the launch grid");
  const SdtwLayout l = sdtw_layout(N, M, T, S, F);
  if (workspace_bytes < l.total) {
    set_error("g2v_softdtw_cdist: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  const size_t lds = dtw_lds_bytes(T);
  if (!g2v_internal_lds_reserve((const void*)softdtw_pair_kernel, lds)) return G2V_ERR_LAUNCH;
  hipStream_t st = (hipStream_t)stream;
  double* v = (double*)((char*)workspace + l.v);
  hipLaunchKernelGGL(softdtw_pair_kernel, dim3((unsigned)(N * MB)), dim3(64), lds, st, x, T, y, M, S, F, P, MB, gamma, v);
  hipLaunchKernelGGL(dtw_argmin_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, (const double*)v, N, M, 1, out, labels, best);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int g2v_softdtw_alignment(const float* x, int64_t R, int T, const double* z, int S, int F, double gamma, double* value,
                                     double* E, g2v_stream_t stream) {
  G2V_REQUIRE(x && z && value && E, "null pointer");
  G2V_REQUIRE(R >= 1 && T >= 1 && S >= 1 && F >= 1, "sizes: R, T, S, F >= 1");
  G2V_REQUIRE(sdtw_gamma_ok(gamma), "gamma must be finite and > 0");
  if (!dtw_shape_ok(R, 1, T, S, F)) return sdtw_refuse("g2v_softdtw_alignment", R, 1, T, S, F);
  const size_t lds = sdtw_lds_bytes(T);
  if (!g2v_internal_lds_reserve((const void*)softdtw_align_kernel, lds)) return G2V_ERR_LAUNCH;
  hipLaunchKernelGGL(softdtw_align_kernel, dim3((unsigned)R), dim3(64), lds, (hipStream_t)stream, x, R, T, (const int64_t*)nullptr, z, S,
                     F, gamma, value, E, (size_t)S * T, (size_t)T, (size_t)1);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int g2v_softdtw_grad(const float* x, int64_t N, int T, const int64_t* rows, int64_t R, const double* weights, const double* z,
                                int S, int F, double gamma, double* value, double* grad, void* workspace, size_t workspace_bytes,
                                g2v_stream_t stream) {
  G2V_REQUIRE(x && rows && z && value && grad && workspace, "null pointer");
  G2V_REQUIRE(N >= 1 && R >= 1 && T >= 1 && S >= 1 && F >= 1, "sizes: N, R, T, S, F >= 1");
  G2V_REQUIRE(sdtw_gamma_ok(gamma), "gamma must be finite and > 0");
  if (!dtw_shape_ok(N, 1, T, S, F) || !dtw_shape_ok(R, 1, T, S, F)) return sdtw_refuse("g2v_softdtw_grad", N, R, T, S, F);
  G2V_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "workspace must be 16-byte aligned");
  const SdtwLayout l = sdtw_layout(R, 1, T, S, F);
  if (workspace_bytes < l.total) {
    set_error("g2v_softdtw_grad: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  const size_t lds = sdtw_lds_bytes(T);
  if (!g2v_internal_lds_reserve((const void*)softdtw_align_kernel, lds)) return G2V_ERR_LAUNCH;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* E = (double*)(ws + l.E);
  double* val = (double*)(ws + l.value);
  double* part = (double*)(ws + l.part);
  double* partr = (double*)(ws + l.partr);
  double* partv = (double*)(ws + l.partv);
  hipLaunchKernelGGL(softdtw_align_kernel, dim3((unsigned)R), dim3(64), lds, st, x, N, T, rows, z, S, F, gamma, val, E, (size_t)S * T,
                     (size_t)1, (size_t)S);
  hipLaunchKernelGGL(softdtw_slab_kernel, dim3((unsigned)l.slabs, S), dim3(256), 0, st, x, N, T, S, F, rows, R, weights, (const double*)E,
                     (const double*)val, part, partr, partv);
  hipLaunchKernelGGL(softdtw_fold_kernel, dim3(S), dim3(256), 0, st, S, F, l.slabs, z, (const double*)part, (const double*)partr,
                     (const double*)partv, value, grad);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
