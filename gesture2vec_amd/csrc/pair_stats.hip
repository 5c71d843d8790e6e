// pair_stats.hip -- statistics over all pairwise Euclidean distances between fp32 rows, reduced as the pairs are formed, and the distances
// of every row to its temporal neighbours (gesture2vec_amd/repdist.py; the reference's calculate_distances, Clustering.py:410-505, whose
// np.mean(pdist(latents)) stores N (N - 1) / 2 float64 values).  No distance is stored here, so the row count is bounded by the index
// width and not by memory.
//
//   pd_norm_kernel (pair_dist.hpp)   |x_i|^2 (and |y_j|^2) in float64
//   ps_init_kernel      clears the histogram
//   ps_pair_kernel      one workgroup (4 waves) takes the 64-row strip s of x and the run g of `run` consecutive 64-row tiles of the
//                       other set (of x itself without y).  Every tile goes through pd_tile_f64: d^2 on the float64 MFMA, near pairs
//                       again from differences, d = sqrt(d^2) in the callback.  Without y the pairs are i < j: a tile below the
//                       diagonal is never visited and a diagonal tile counts row < column only.  A lane adds its values in the order
//                       it meets them (tile, column group, register); the lanes are folded in a fixed tree, and the workgroup writes
//                       ONE partial { sum d, sum d^2, min, max, pairs, pairs not finite } to slot s * groups + g.  A workgroup whose
//                       run lies wholly below the diagonal writes the empty partial, so every slot is written in every call.  Bins
//                       are counted in LDS and flushed with 64-bit integer adds: integer sums do not depend on their order.
//   ps_fold_kernel      (one workgroup) thread t adds the slots [t per, (t + 1) per) in ascending order, then the threads in a fixed tree
//   ps_lag_kernel       one wave per row: for every lag (|x_{i - lag} - x_i| + |x_{i + lag} - x_i|) / 2 from pd_pair_sq
// `run` is a function of the two row counts alone (ps_run), never of the device: the same input gives the same bits on any device.
// No floating-point atomics.  No workgroup waits on another, so nothing here needs the launch ledger.
#include "common.hpp"
#include "km_sort.hpp"
#include "pair_dist.hpp"

namespace g2v {
namespace {

constexpr int PS_MAX_E = 512;
constexpr int64_t PS_MAX_ROWS = (int64_t)1 << 24;   // 2^18 strips x 64 groups of workgroups; pd_tile_f64 indexes the second set with int
constexpr int PS_MAX_BINS = 1024;                  // edges (8 KiB) and counters (4 KiB) of a workgroup live in LDS
constexpr int PS_GROUPS = 64;                      // a strip is split over at most this many workgroups
constexpr int PS_MAX_LAGS = 8;
constexpr int PS_FOLD_THREADS = 1024;

inline bool ps_shape_ok(int64_t N, int64_t M, int E, int bins) {
  return N >= 1 && N <= PS_MAX_ROWS && M >= 0 && M <= PS_MAX_ROWS && E >= 1 && E <= PS_MAX_E && bins >= 0 && bins <= PS_MAX_BINS;
}

// tiles of the second set per workgroup; nb = rows of the second set
inline int ps_run(int64_t nb) { return (int)std::max<int64_t>(1, ((nb + PD_TILE - 1) / PD_TILE + PS_GROUPS - 1) / PS_GROUPS); }

struct PsLayout {
  size_t norm_x, norm_y, pd, pc, total;
  int64_t slots;
  int run, groups;
};

inline PsLayout ps_layout(int64_t N, int64_t M) {
  PsLayout l;
  const int64_t nb = M > 0 ? M : N;
  const int64_t Wa = (N + PD_TILE - 1) / PD_TILE, Wb = (nb + PD_TILE - 1) / PD_TILE;
  l.run = ps_run(nb);
  l.groups = (int)((Wb + l.run - 1) / l.run);
  l.slots = Wa * l.groups;
  size_t o = 0;
  l.norm_x = o;  o = km_align(o + (size_t)N * sizeof(double));
  l.norm_y = o;  o = km_align(o + (size_t)M * sizeof(double));
  l.pd = o;      o = km_align(o + (size_t)l.slots * 4 * sizeof(double));      // [4][slots]: sum, sum of squares, min, max
  l.pc = o;      o = km_align(o + (size_t)l.slots * 2 * sizeof(int64_t));     // [2][slots]: pairs, pairs not finite
  l.total = o;
  return l;
}

__global__ __launch_bounds__(256) void ps_init_kernel(int64_t* __restrict__ hist, int bins) {
  const int b = (int)blockIdx.x * 256 + threadIdx.x;
  if (b < bins) hist[b] = 0;
}

// numpy.histogram's rule over ascending edges e[0 .. bins]: the bin b with e[b] <= d < e[b + 1], the last one closed; -1 for none (NaN too)
__device__ __forceinline__ int ps_bin(const double* __restrict__ e, int bins, double d) {
  if (!(d >= e[0]) || !(d <= e[bins])) return -1;
  int lo = 0, hi = bins;                                     // e[lo] <= d, and d < e[hi] or hi == bins
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (d >= e[mid]) lo = mid; else hi = mid;
  }
  return lo;
}

// (four waves per SIMD: the tile's 32 accumulator registers then live among the 128 vector registers, without scratch, and a fourth
// workgroup per CU covers the others' barriers and epilogues; 4 x 31 KB of LDS fit the CU's 160 KB)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void ps_pair_kernel(const float* __restrict__ x, int64_t ldx, int na, const float* __restrict__ y,
                                                     int64_t ldy, int nb, int E, const double* __restrict__ norm_x,
                                                     const double* __restrict__ norm_y, int same, int run, int groups,
                                                     int64_t slots, const double* __restrict__ edges, int bins,
                                                     double* __restrict__ pd, int64_t* __restrict__ pc, int64_t* __restrict__ hist) {
  __shared__ __attribute__((aligned(16))) float sa[PD_TILE * PD_LD];
  __shared__ __attribute__((aligned(16))) float sb[PD_TILE * PD_LD];
  __shared__ double s_edges[PS_MAX_BINS + 1];
  __shared__ unsigned s_hist[PS_MAX_BINS];
  __shared__ double s_red[4][4];
  __shared__ int64_t s_cnt[4][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t slot = blockIdx.x;
  const int s = (int)(slot / groups), g = (int)(slot % groups);
  const int Wb = (nb + PD_TILE - 1) / PD_TILE;
  const int t_end = min(Wb, (g + 1) * run);
  const int t_begin = same ? max(g * run, s) : g * run;      // (workgroup-uniform) tiles below the diagonal are never visited
  const int64_t a0 = (int64_t)s * PD_TILE;

  for (int b = tid; b < bins; b += 256) s_hist[b] = 0u;
  for (int b = tid; b <= bins && bins > 0; b += 256) s_edges[b] = edges[b];
  // (pd_tile_f64's first barrier orders the two loops above against the callbacks)

  double sum = 0.0, sq = 0.0, lo = (double)__builtin_inff(), hi = -(double)__builtin_inff();
  int64_t cnt = 0, bad = 0;
  if (t_begin < t_end) {
    double nr[4];
    pd_row_norms_f64(norm_x, na, a0, nr);
    for (int t = t_begin; t < t_end; ++t) {
      pd_tile_f64(x, ldx, na, a0, nr, y, ldy, nb, t * PD_TILE, norm_y, E, same != 0, sa, sb,
                  [&](int64_t row, int col, const double (&dd)[4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t rr = row + 4 * r;
          if (rr >= na || col >= nb || (same && rr >= col)) continue;
          const double d2 = dd[r], d = sqrt(d2);
          sum += d;
          sq += d2;
          lo = fmin(lo, d);                                  // (fmin, fmax: a NaN is not a minimum; it is counted in `bad`)
          hi = fmax(hi, d);
          cnt += 1;
          bad += (d - d == 0.0) ? 0 : 1;                     // NaN or infinite
          if (bins > 0) {
            const int b = ps_bin(s_edges, bins, d);
            if (b >= 0) atomicAdd(&s_hist[b], 1u);           // (at most 64 x 64 x run <= 2^30 pairs per workgroup)
          }
        }
      });
    }
  }

  sum = km_wave_sum(sum);
  sq = km_wave_sum(sq);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, o));
    hi = fmax(hi, __shfl_xor(hi, o));
    cnt += __shfl_xor(cnt, o);
    bad += __shfl_xor(bad, o);
  }
  if (lane == 0) {
    s_red[wave][0] = sum;
    s_red[wave][1] = sq;
    s_red[wave][2] = lo;
    s_red[wave][3] = hi;
    s_cnt[wave][0] = cnt;
    s_cnt[wave][1] = bad;
  }
  __syncthreads();                                           // also: every s_hist add of the workgroup has landed
  if (tid == 0) {
    pd[0 * slots + slot] = (s_red[0][0] + s_red[1][0]) + (s_red[2][0] + s_red[3][0]);
    pd[1 * slots + slot] = (s_red[0][1] + s_red[1][1]) + (s_red[2][1] + s_red[3][1]);
    pd[2 * slots + slot] = fmin(fmin(s_red[0][2], s_red[1][2]), fmin(s_red[2][2], s_red[3][2]));
    pd[3 * slots + slot] = fmax(fmax(s_red[0][3], s_red[1][3]), fmax(s_red[2][3], s_red[3][3]));
    pc[0 * slots + slot] = (s_cnt[0][0] + s_cnt[1][0]) + (s_cnt[2][0] + s_cnt[3][0]);
    pc[1 * slots + slot] = (s_cnt[0][1] + s_cnt[1][1]) + (s_cnt[2][1] + s_cnt[3][1]);
  }
  for (int b = tid; b < bins; b += 256) {
    const unsigned c = s_hist[b];
    if (c) atomicAdd(reinterpret_cast<unsigned long long*>(hist + b), (unsigned long long)c);
  }
}

__global__ __launch_bounds__(PS_FOLD_THREADS) void ps_fold_kernel(const double* __restrict__ pd, const int64_t* __restrict__ pc,
                                                                 int64_t slots, double* __restrict__ out,
                                                                 int64_t* __restrict__ counts) {
  __shared__ double s_d[4][PS_FOLD_THREADS];
  __shared__ int64_t s_c[2][PS_FOLD_THREADS];
  const int tid = threadIdx.x;
  const int64_t per = (slots + PS_FOLD_THREADS - 1) / PS_FOLD_THREADS;
  const int64_t b = min(slots, tid * per), e = min(slots, b + per);
  double sum = 0.0, sq = 0.0, lo = (double)__builtin_inff(), hi = -(double)__builtin_inff();
  int64_t cnt = 0, bad = 0;
  for (int64_t k = b; k < e; ++k) {
    sum += pd[k];
    sq += pd[slots + k];
    lo = fmin(lo, pd[2 * slots + k]);
    hi = fmax(hi, pd[3 * slots + k]);
    cnt += pc[k];
    bad += pc[slots + k];
  }
  s_d[0][tid] = sum;
  s_d[1][tid] = sq;
  s_d[2][tid] = lo;
  s_d[3][tid] = hi;
  s_c[0][tid] = cnt;
  s_c[1][tid] = bad;
  __syncthreads();
  for (int o = PS_FOLD_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
      s_d[0][tid] += s_d[0][tid + o];
      s_d[1][tid] += s_d[1][tid + o];
      s_d[2][tid] = fmin(s_d[2][tid], s_d[2][tid + o]);
      s_d[3][tid] = fmax(s_d[3][tid], s_d[3][tid + o]);
      s_c[0][tid] += s_c[0][tid + o];
      s_c[1][tid] += s_c[1][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = s_d[0][0];
    out[1] = s_d[1][0];
    out[2] = s_d[2][0];
    out[3] = s_d[3][0];
    counts[0] = s_c[0][0];
    counts[1] = s_c[1][0];
  }
}

struct PsLags {
  int v[PS_MAX_LAGS];
};

__global__ __launch_bounds__(256) void ps_lag_kernel(const float* __restrict__ x, int64_t ld, int64_t N, int E, PsLags lags, int n_lags,
                                                    const int64_t* __restrict__ clip, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;                                        // (wave-uniform)
  const float* xi = x + i * ld;
  for (int l = 0; l < n_lags; ++l) {
    const int64_t lag = lags.v[l];
    double v = __builtin_nan("");
    bool ok = i - lag >= 0 && i + lag < N;                   // (wave-uniform)
    if (ok && clip) ok = clip[i - lag] == clip[i] && clip[i + lag] == clip[i];
    if (ok) {
      const double d0 = sqrt(pd_pair_sq(x + (i - lag) * ld, xi, E, lane));
      const double d1 = sqrt(pd_pair_sq(x + (i + lag) * ld, xi, E, lane));
      v = (d0 + d1) / 2;
    }
    if (lane == 0) out[(int64_t)l * N + i] = v;
  }
}

}  // namespace
}  // namespace g2v

using namespace g2v;

extern "C" int64_t g2v_pair_stats_max_rows(void) { return PS_MAX_ROWS; }

extern "C" int g2v_pair_stats_max_bins(void) { return PS_MAX_BINS; }

extern "C" int g2v_pair_stats_run(int64_t N, int64_t M) {
  if (!ps_shape_ok(N, M, 1, 0)) return 0;
  return ps_run(M > 0 ? M : N);
}

extern "C" size_t g2v_pair_stats_workspace(int64_t N, int64_t M, int E, int bins) {
  if (!ps_shape_ok(N, M, E, bins)) return 0;
  return ps_layout(N, M).total;
}

extern "C" int g2v_pair_stats(const float* x, int64_t ldx, int64_t N, const float* y, int64_t ldy, int64_t M, int E, const double* edges,
                              int bins, double* out, int64_t* counts, int64_t* hist, void* workspace, size_t workspace_bytes,
                              g2v_stream_t stream) {
  G2V_REQUIRE(x && out && counts && workspace, "null pointer");
  G2V_REQUIRE(N >= 1 && E >= 1 && bins >= 0 && M >= 0, "sizes: N >= 1, E >= 1, M >= 0, bins >= 0");
  G2V_REQUIRE(y ? M >= 1 : M == 0, "M: the rows of y, 0 without y");
  if (!ps_shape_ok(N, M, E, bins)) {
    set_error("g2v_pair_stats: needs N, M <= %lld, E <= %d and bins <= %d (N = %lld, M = %lld, E = %d, bins = %d)",
              (long long)PS_MAX_ROWS, PS_MAX_E, PS_MAX_BINS, (long long)N, (long long)M, E, bins);
    return G2V_ERR_UNSUPPORTED;
  }
  G2V_REQUIRE(bins == 0 || (edges && hist), "bins > 0 needs edges and hist");
  G2V_REQUIRE(ldx >= E && (ldx & 3) == 0 && (!y || (ldy >= E && (ldy & 3) == 0)), "row stride smaller than E or not a multiple of 4");
  G2V_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
              "x, y and workspace must be 16-byte aligned");
  G2V_REQUIRE(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(hist) |
                reinterpret_cast<uintptr_t>(edges)) & 7) == 0,
              "out, counts, hist and edges must be 8-byte aligned");
  const PsLayout l = ps_layout(N, M);
  if (workspace_bytes < l.total) {
    set_error("g2v_pair_stats: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* norm_x = (double*)(ws + l.norm_x);
  double* norm_y = y ? (double*)(ws + l.norm_y) : norm_x;
  double* pd = (double*)(ws + l.pd);
  int64_t* pc = (int64_t*)(ws + l.pc);
  hipLaunchKernelGGL(pd_norm_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, x, ldx, N, E, norm_x);
  if (y) hipLaunchKernelGGL(pd_norm_kernel, dim3(cdiv(M, 256)), dim3(256), 0, st, y, ldy, M, E, norm_y);
  if (bins > 0) hipLaunchKernelGGL(ps_init_kernel, dim3(cdiv(bins, 256)), dim3(256), 0, st, hist, bins);
  hipLaunchKernelGGL(ps_pair_kernel, dim3((unsigned)l.slots), dim3(256), 0, st, x, ldx, (int)N, y ? y : x, y ? ldy : ldx,
                     (int)(y ? M : N), E, (const double*)norm_x, (const double*)norm_y, y ? 0 : 1, l.run, l.groups, l.slots, edges, bins,
                     pd, pc, hist);
  hipLaunchKernelGGL(ps_fold_kernel, dim3(1), dim3(PS_FOLD_THREADS), 0, st, (const double*)pd, (const int64_t*)pc, l.slots, out, counts);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int g2v_lag_distances(const float* x, int64_t ld, int64_t N, int E, const int32_t* lags, int n_lags, const int64_t* clip_ids,
                                 double* out, g2v_stream_t stream) {
  G2V_REQUIRE(x && lags && out, "null pointer");
  G2V_REQUIRE(N >= 1 && E >= 1, "sizes: N >= 1, E >= 1");
  G2V_REQUIRE(n_lags >= 1 && n_lags <= PS_MAX_LAGS, "1 <= n_lags <= 8");
  if (E > PS_MAX_E || N > PS_MAX_ROWS) {
    set_error("g2v_lag_distances: needs N <= %lld and E <= %d (N = %lld, E = %d)", (long long)PS_MAX_ROWS, PS_MAX_E, (long long)N, E);
    return G2V_ERR_UNSUPPORTED;
  }
  PsLags lv;
  for (int l = 0; l < PS_MAX_LAGS; ++l) lv.v[l] = l < n_lags ? lags[l] : 1;
  for (int l = 0; l < n_lags; ++l) G2V_REQUIRE(lv.v[l] >= 1, "every lag must be >= 1");
  G2V_REQUIRE(ld >= E && (ld & 3) == 0, "row stride smaller than E or not a multiple of 4");
  G2V_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0 &&
                  (reinterpret_cast<uintptr_t>(clip_ids) & 7) == 0,
              "x must be 16-byte aligned, out and clip_ids 8-byte aligned");
  hipLaunchKernelGGL(ps_lag_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, ld, N, E, lv, n_lags, clip_ids,
                     out);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
