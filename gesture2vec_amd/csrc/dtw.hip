// dtw.hip -- dynamic time warping between (N, T, F) fp32 series and (M, S, F) float64 centres, and the two halves of a DTW barycentre
// averaging (DBA) step: what gesture2vec_amd/timeseries.py builds tslearn's TimeSeriesKMeans(metric="dtw") from (the reference's
// Clustering.py:629-669).  The definitions are in include/g2v.h.  Everything is float64; a wavefront dynamic programme, no contraction.
//
// One wave (a workgroup of 64 threads) owns one series n and DTW_G = 64 / P centres, P the power of two >= max(S, 16): lane l holds
// column j = l % P of centre g = l / P.  dtw_fill:
//   cost     dtw_cost_tile (dtw_tile.hpp, shared with softdtw.hip): tile[i][l] (T x 64 float64 in LDS) = sum_f (a_if - b_jf)^2
//   sweep    the T + S - 1 anti-diagonals in order: lane j takes cell (d - j, j).  acc(i-1, j) is the lane's own last value,
//            acc(i, j-1) the left neighbour's last value (one __shfl_up), acc(i-1, j-1) the one it sent a diagonal earlier; lanes
//            outside the tile hold +inf, and a lane with j == 0 reads +inf, so groups do not leak into each other.  The lane that
//            holds (T-1, S-1) ends with dtw^2.  With WALK the move of every cell is decided here, where the three values are in
//            registers (the header's tie order), and stored as a byte in the LDS the series slice no longer needs.
// tile[i * 64 + l]: neighbouring lanes of a diagonal are 63 doubles apart, an odd stride, so the sweep's reads and writes are free
// of bank conflicts, and the cost phase's are consecutive.
//
//   dtw_pair_kernel    one workgroup per (n, group of G centres), the groups of one series next to each other: d2[n][m]
//   dtw_argmin_kernel  (dtw_tile.hpp) one wave per n: out[n][:] = d2 or sqrt(d2), labels[n], best[n]; (value, index) lexicographic, lowest index
//   dtw_path_kernel    one wave per member n of a live cluster k: the tile of (x_n, c_k), one lane walks the moves back from
//                      (T-1, S-1) and notes, per centre row s, the range [lo, hi] of series rows matched with it (a warping path is
//                      monotone: the rows matched with one s are consecutive) -> span[n][s] (2 bytes), d2row[n]
//   km_sort.hpp        the members sorted by (label, n) and cut into slabs of DTW_SLAB members of one cluster
//   dtw_slab_kernel    grid (slab, s), threads over f: the slab's members in order, sum of x[n][lo..hi][f] -> part[slab][s][f];
//                      the thread of f == 0 adds the counts, the block of s == 0 the members' dtw^2
//   dtw_fold_kernel    grid (k, s): the slabs of a live cluster in slab order -> sums, counts, cost.  DTW_SLAB is a constant, so the
//                      order of every sum is a function of the labels alone: the same bits on every call, whatever the CU count
//   dtw_update_kernel  one workgroup per cluster: centres = sums / counts, then the stop rule on the device
// No floating-point atomics.
#include "common.hpp"
#include "dtw_tile.hpp"
#include "km_sort.hpp"

namespace g2v {
namespace {

constexpr int DTW_SLAB = 128;               // members of one cluster per partial sum
// the header's moves in its order, the centre being its first index: both step back, the centre steps back, the series steps back
enum { DTW_DIAG = 0, DTW_CENTRE = 1, DTW_SERIES = 2 };

struct DtwLayout {
  int nb;                  // sort blocks
  int64_t max_slabs;
  size_t d2, hdr, hist, counts, cl_start, ch_first, sorted, span, d2row, part, partcnt, partcost, total;
};

inline DtwLayout dtw_layout(int64_t N, int64_t M, int T, int S, int F) {
  DtwLayout l;
  const int K = (int)M;
  l.nb = cdiv(N, KM_SORT_ROWS);
  l.max_slabs = N / DTW_SLAB + K;
  size_t o = 0;
  l.d2 = o;         o = km_align(o + (size_t)N * M * sizeof(double));
  l.hdr = o;        o = km_align(o + HD_WORDS * sizeof(unsigned long long));
  l.hist = o;       o = km_align(o + (size_t)l.nb * K * sizeof(int));
  l.counts = o;     o = km_align(o + (size_t)K * sizeof(int64_t));
  l.cl_start = o;   o = km_align(o + (size_t)(K + 1) * sizeof(int));
  l.ch_first = o;   o = km_align(o + (size_t)(K + 1) * sizeof(int));
  l.sorted = o;     o = km_align(o + (size_t)N * sizeof(int));
  l.span = o;       o = km_align(o + (size_t)N * S * 2);
  l.d2row = o;      o = km_align(o + (size_t)N * sizeof(double));
  l.part = o;       o = km_align(o + (size_t)l.max_slabs * S * F * sizeof(double));
  l.partcnt = o;    o = km_align(o + (size_t)l.max_slabs * S * sizeof(int));
  l.partcost = o;   o = km_align(o + (size_t)l.max_slabs * sizeof(double));
  l.total = o;
  return l;
}

// The accumulated-cost tile of series `a` (T x F fp32) against the centre column this lane owns (`b`: F float64, read only when
// `active`; j its column).  Returns the lane's last accumulated value: dtw^2 in the lane of column S - 1.  lds: dtw_lds_bytes(T).
// WALK: moves[i * 64 + lane] (bytes, over the series slice) = the move out of cell (i, j).  Every lane of the wave must call it.
template <bool WALK>
__device__ __forceinline__ double dtw_fill(const float* __restrict__ a, const double* __restrict__ b, bool active, int j, int T, int S,
                                           int F, unsigned char* lds) {
  double* tile = reinterpret_cast<double*>(lds);
  float* as = reinterpret_cast<float*>(lds + (size_t)T * 64 * sizeof(double));
  const int lane = threadIdx.x;
  dtw_cost_tile(a, b, active, T, F, tile, as);
  unsigned char* moves = reinterpret_cast<unsigned char*>(as);
  const double inf = (double)__builtin_inff();
  double cur = inf, left = inf;
  const bool col = active && j < S;
  for (int d = 0; d < T + S - 1; ++d) {
    const double diag = left;                                // what the left neighbour held two diagonals ago
    const double up = cur;
    left = __shfl_up(cur, 1);
    if (j == 0) left = inf;
    const int i = d - j;
    if (col && i >= 0 && i < T) {
      int mv = DTW_DIAG;                                     // strict <: on equal values the earlier of DIAG, CENTRE, SERIES stays
      double m = diag;
      if (left < m) { m = left; mv = DTW_CENTRE; }
      if (up < m) { m = up; mv = DTW_SERIES; }
      if (i == 0 && j == 0) m = 0.0;
      cur = tile[i * 64 + lane] + m;
      if (WALK) moves[i * 64 + lane] = (unsigned char)mv;
    } else {
      cur = inf;
    }
  }
  return cur;
}

__global__ __launch_bounds__(64) void dtw_pair_kernel(const float* __restrict__ x, int T, const double* __restrict__ y, int64_t M, int S,
                                                     int F, int P, int MB, double* __restrict__ d2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dtw_lds[];
  const int lane = threadIdx.x;
  const int64_t n = blockIdx.x / MB;                         // (the centres fastest: neighbouring workgroups share a series)
  const int64_t m = (int64_t)(blockIdx.x % MB) * (64 / P) + lane / P;
  const int j = lane % P;
  const bool active = m < M && j < S;
  const double* b = y + ((size_t)(active ? m : 0) * S + (active ? j : 0)) * F;
  const double v = dtw_fill<false>(x + (size_t)n * T * F, b, active, j, T, S, F, dtw_lds);
  if (active && j == S - 1) d2[n * M + m] = v;
}

// The tile's rows are the series and its columns the centre: the header's tile (centre first) transposed.  Its values are the
// header's bit for bit -- the cost is symmetric, and so are min and + -- and dtw_fill names the moves by what steps back, not by axis.
__global__ __launch_bounds__(64) void dtw_path_kernel(const float* __restrict__ x, int T, const int64_t* __restrict__ labels,
                                                     const double* __restrict__ centers, int K, int S, int F,
                                                     const uint8_t* __restrict__ live, unsigned char* __restrict__ span,
                                                     double* __restrict__ d2row) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dtw_lds[];
  __shared__ unsigned char lo[DTW_MAX_LEN], hi[DTW_MAX_LEN];
  const int lane = threadIdx.x;
  const int64_t n = blockIdx.x;
  const int64_t k = labels[n];
  if (k < 0 || k >= K || (live && !live[k])) return;         // (workgroup-uniform)
  const bool active = lane < S;
  const double* b = centers + ((size_t)k * S + (active ? lane : 0)) * F;
  const double v = dtw_fill<true>(x + (size_t)n * T * F, b, active, lane, T, S, F, dtw_lds);
  if (lane == S - 1) d2row[n] = v;
  __syncthreads();
  if (lane == 0) {
    const unsigned char* moves = dtw_lds + (size_t)T * 64 * sizeof(double);
    int i = T - 1, j = S - 1;                                // i: series row, j: centre row
    hi[j] = (unsigned char)i;
    while (i > 0 || j > 0) {                                 // (on an edge the two absent moves were +inf: the only move was chosen)
      const int mv = i == 0 ? DTW_CENTRE : (j == 0 ? DTW_SERIES : moves[i * 64 + j]);     // (a NaN could name an absent move)
      if (mv == DTW_SERIES) {
        --i;
      } else {
        lo[j] = (unsigned char)i;
        --j;
        if (mv == DTW_DIAG) --i;
        hi[j] = (unsigned char)i;
      }
    }
    lo[0] = 0;
  }
  __syncthreads();
  if (lane < S) {
    span[((size_t)n * S + lane) * 2] = lo[lane];
    span[((size_t)n * S + lane) * 2 + 1] = hi[lane];
  }
}

// the cluster k with ch_first[k] <= c < ch_first[k + 1]
__device__ __forceinline__ int dtw_slab_cluster(const int* __restrict__ ch_first, int K, int c) {
  int lo = 0, hi = K;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ch_first[mid] <= c) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void dtw_slab_kernel(const float* __restrict__ x, int T, int S, int F, int K,
                                                      const uint8_t* __restrict__ live, const int* __restrict__ sorted,
                                                      const int* __restrict__ cl_start, const int* __restrict__ ch_first,
                                                      const unsigned long long* __restrict__ hdr, const unsigned char* __restrict__ span,
                                                      const double* __restrict__ d2row, double* __restrict__ part,
                                                      int* __restrict__ partcnt, double* __restrict__ partcost) {
  const int c = (int)blockIdx.x, s = (int)blockIdx.y;
  if ((unsigned long long)c >= hdr[HD_CHUNKS]) return;
  const int k = dtw_slab_cluster(ch_first, K, c);
  if (live && !live[k]) return;
  const int start = cl_start[k] + (c - ch_first[k]) * DTW_SLAB;
  const int len = min(DTW_SLAB, cl_start[k + 1] - start);
  const int tid = threadIdx.x;
  double acc[2] = {0.0, 0.0};                                // columns tid and tid + 256
  int cnt = 0;
  double cost = 0.0;
  for (int r = 0; r < len; ++r) {
    const int64_t n = sorted[start + r];
    const int lo = span[((size_t)n * S + s) * 2], hi = min((int)span[((size_t)n * S + s) * 2 + 1], T - 1);
    const float* xr = x + (size_t)n * T * F;
    for (int t = lo; t <= hi; ++t) {
      if (tid < F) acc[0] += (double)xr[(size_t)t * F + tid];
      if (tid + 256 < F) acc[1] += (double)xr[(size_t)t * F + tid + 256];
    }
    cnt += hi - lo + 1;
    if (s == 0 && tid == 0) cost += d2row[n];
  }
  double* p = part + ((size_t)c * S + s) * F;
  if (tid < F) p[tid] = acc[0];
  if (tid + 256 < F) p[tid + 256] = acc[1];
  if (tid == 0) {
    partcnt[(size_t)c * S + s] = cnt;
    if (s == 0) partcost[c] = cost;
  }
}

__global__ __launch_bounds__(256) void dtw_fold_kernel(int S, int F, const uint8_t* __restrict__ live, const int* __restrict__ ch_first,
                                                      const double* __restrict__ part, const int* __restrict__ partcnt,
                                                      const double* __restrict__ partcost, double* __restrict__ sums,
                                                      int64_t* __restrict__ counts, double* __restrict__ cost) {
  const int k = (int)blockIdx.x, s = (int)blockIdx.y;
  if (live && !live[k]) return;
  const int c0 = ch_first[k], c1 = ch_first[k + 1];
  for (int f = threadIdx.x; f < F; f += 256) {
    double v = 0.0;
    for (int c = c0; c < c1; ++c) v += part[((size_t)c * S + s) * F + f];
    sums[((size_t)k * S + s) * F + f] = v;
  }
  if (threadIdx.x == 0) {
    int64_t n = 0;
    for (int c = c0; c < c1; ++c) n += partcnt[(size_t)c * S + s];
    counts[(size_t)k * S + s] = n;
    if (s == 0) {
      double v = 0.0;
      for (int c = c0; c < c1; ++c) v += partcost[c];
      cost[k] = v;
    }
  }
}

__global__ __launch_bounds__(256) void dtw_update_kernel(const double* __restrict__ sums, const int64_t* __restrict__ counts,
                                                        const double* __restrict__ cost, const int64_t* __restrict__ members,
                                                        double* __restrict__ prev, uint8_t* __restrict__ live,
                                                        double* __restrict__ centers, int K, int S, int F, double tol) {
  const int k = (int)blockIdx.x;
  const bool on = live[k] != 0;
  __syncthreads();                                           // (every thread has read live[k] before thread 0 may clear it)
  if (!on) return;
  if (members[k] <= 0) {                                     // an empty cluster has no barycentre: it keeps its centre and stops
    if (threadIdx.x == 0) live[k] = 0;
    return;
  }
  for (int e = threadIdx.x; e < S * F; e += 256) {
    const size_t at = (size_t)k * S * F + e;
    centers[at] = sums[at] / (double)counts[(size_t)k * S + e / F];
  }
  if (threadIdx.x == 0) {
    const double c = cost[k] / (double)members[k], p = prev[k];
    if (fabs(p - c) < tol || p < c) live[k] = 0;
    else prev[k] = c;
  }
}

}  // namespace
}  // namespace g2v

using namespace g2v;

extern "C" int g2v_dtw_max_len(void) { return DTW_MAX_LEN; }

extern "C" size_t g2v_dtw_workspace(int64_t N, int64_t M, int T, int S, int F) {
  if (!dtw_shape_ok(N, M, T, S, F)) return 0;
  return dtw_layout(N, M, T, S, F).total;
}

static int dtw_refuse(const char* fn, int64_t N, int64_t M, int T, int S, int F) {
  set_error("%s: needs 1 <= T, S <= %d, 1 <= F <= %d and fewer than 2^31 series and centres (N = %lld, M = %lld, T = %d, S = %d, F = %d)",
            fn, DTW_MAX_LEN, DTW_MAX_F, (long long)N, (long long)M, T, S, F);
  return G2V_ERR_UNSUPPORTED;
}

extern "C" int g2v_dtw_cdist(const float* x, int64_t N, int T, const double* y, int64_t M, int S, int F, int squared, double* out,
                             int64_t* labels, double* best, void* workspace, size_t workspace_bytes, g2v_stream_t stream) {
  G2V_REQUIRE(x && y && workspace, "null pointer");
  G2V_REQUIRE((labels == nullptr) == (best == nullptr), "labels and best are given together or not at all");
  G2V_REQUIRE(out || labels, "nothing to write: out, labels and best are all null");
  G2V_REQUIRE(N >= 1 && M >= 1 && T >= 1 && S >= 1 && F >= 1, "sizes: N, M, T, S, F >= 1");
  if (!dtw_shape_ok(N, M, T, S, F)) return dtw_refuse("g2v_dtw_cdist", N, M, T, S, F);
  G2V_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "workspace must be 16-byte aligned");
  const int P = dtw_group_width(S), MB = cdiv(M, 64 / P);
  G2V_REQUIRE(N * MB <= 0x7fffffff, "N * M exceeds the launch grid");
  const DtwLayout l = dtw_layout(N, M, T, S, F);
  if (workspace_bytes < l.total) {
    set_error("g2v_dtw_cdist: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  const size_t lds = dtw_lds_bytes(T);
  if (!g2v_internal_lds_reserve((const void*)dtw_pair_kernel, lds)) return G2V_ERR_LAUNCH;
  hipStream_t st = (hipStream_t)stream;
  double* d2 = (double*)((char*)workspace + l.d2);
  hipLaunchKernelGGL(dtw_pair_kernel, dim3((unsigned)(N * MB)), dim3(64), lds, st, x, T, y, M, S, F, P, MB, d2);
  hipLaunchKernelGGL(dtw_argmin_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, (const double*)d2, N, M, squared, out, labels, best);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int g2v_dtw_dba_accumulate(const float* x, int64_t N, int T, const int64_t* labels, const double* centers, int K, int S,
                                      int F, const uint8_t* live, double* sums, int64_t* counts, double* cost, void* workspace,
                                      size_t workspace_bytes, g2v_stream_t stream) {
  G2V_REQUIRE(x && labels && centers && sums && counts && cost && workspace, "null pointer");
  G2V_REQUIRE(N >= 1 && K >= 1 && T >= 1 && S >= 1 && F >= 1, "sizes: N, K, T, S, F >= 1");
  if (!dtw_shape_ok(N, K, T, S, F)) return dtw_refuse("g2v_dtw_dba_accumulate", N, K, T, S, F);
  G2V_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "workspace must be 16-byte aligned");
  const DtwLayout l = dtw_layout(N, K, T, S, F);
  if (workspace_bytes < l.total) {
    set_error("g2v_dtw_dba_accumulate: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  const size_t lds = dtw_lds_bytes(T);
  if (!g2v_internal_lds_reserve((const void*)dtw_path_kernel, lds)) return G2V_ERR_LAUNCH;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  unsigned long long* hdr = (unsigned long long*)(ws + l.hdr);
  int* hist = (int*)(ws + l.hist);
  int64_t* members = (int64_t*)(ws + l.counts);
  int* cl_start = (int*)(ws + l.cl_start);
  int* ch_first = (int*)(ws + l.ch_first);
  int* sorted = (int*)(ws + l.sorted);
  unsigned char* span = (unsigned char*)(ws + l.span);
  double* d2row = (double*)(ws + l.d2row);
  double* part = (double*)(ws + l.part);
  int* partcnt = (int*)(ws + l.partcnt);
  double* partcost = (double*)(ws + l.partcost);
  const int use_lds = K <= KM_LDS_BINS ? 1 : 0;

  (void)hipMemsetAsync(hdr, 0, HD_WORDS * sizeof(unsigned long long), st);
  if (!use_lds) (void)hipMemsetAsync(hist, 0, (size_t)l.nb * K * sizeof(int), st);
  hipLaunchKernelGGL(km_hist_kernel, dim3(l.nb), dim3(256), 0, st, labels, (const int64_t*)nullptr, N, K, hist, hdr, use_lds,
                     (const double*)nullptr);
  hipLaunchKernelGGL(km_prefix_kernel, dim3(cdiv(K, 64)), dim3(1024), 0, st, hist, l.nb, K, members, (const double*)nullptr);
  hipLaunchKernelGGL(km_scan_kernel, dim3(1), dim3(1024), 0, st, K, DTW_SLAB, (const int64_t*)members, cl_start, ch_first, hdr,
                     (const double*)nullptr);
  int label_bits = 0;
  while (label_bits < 31 && ((int64_t)1 << label_bits) < K) ++label_bits;
  hipLaunchKernelGGL(km_scatter_kernel, dim3(l.nb), dim3(64), 0, st, labels, N, K, label_bits, hist, (const int*)cl_start, sorted,
                     use_lds, (const double*)nullptr);
  hipLaunchKernelGGL(dtw_path_kernel, dim3((unsigned)N), dim3(64), lds, st, x, T, labels, centers, K, S, F, live, span, d2row);
  hipLaunchKernelGGL(dtw_slab_kernel, dim3((unsigned)l.max_slabs, S), dim3(256), 0, st, x, T, S, F, K, live, (const int*)sorted,
                     (const int*)cl_start, (const int*)ch_first, (const unsigned long long*)hdr, (const unsigned char*)span,
                     (const double*)d2row, part, partcnt, partcost);
  hipLaunchKernelGGL(dtw_fold_kernel, dim3(K, S), dim3(256), 0, st, S, F, live, (const int*)ch_first, (const double*)part,
                     (const int*)partcnt, (const double*)partcost, sums, counts, cost);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int g2v_dtw_dba_update(const double* sums, const int64_t* counts, const double* cost, const int64_t* members, void* state,
                                  double* centers, int K, int S, int F, double tol, g2v_stream_t stream) {
  G2V_REQUIRE(sums && counts && cost && members && state && centers, "null pointer");
  G2V_REQUIRE(K >= 1 && S >= 1 && F >= 1, "sizes: K, S, F >= 1");
  if (S > DTW_MAX_LEN || F > DTW_MAX_F) return dtw_refuse("g2v_dtw_dba_update", 1, K, 1, S, F);
  G2V_REQUIRE((reinterpret_cast<uintptr_t>(state) & 7) == 0, "state must be 8-byte aligned");
  double* prev = (double*)state;
  uint8_t* live = (uint8_t*)(prev + K);
  hipLaunchKernelGGL(dtw_update_kernel, dim3(K), dim3(256), 0, (hipStream_t)stream, sums, counts, cost, members, prev, live, centers, K,
                     S, F, tol);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
