// ward.hip -- Ward agglomerative clustering over (N, E) fp32 latent rows, with the tree of scipy.cluster.hierarchy.ward and therefore of
// sklearn.cluster.AgglomerativeClustering(linkage="ward") (gesture2vec_amd/agglomerative.py; the reference's Clustering.py:751-755).
// scipy runs a serial nearest-neighbour chain over a float64 condensed matrix.  Ward linkage is reducible: merging x and y moves no
// other cluster closer to a third than the nearer of x and y was.  Two clusters that are each other's nearest neighbour can therefore
// be merged at any time, all such pairs of a round at once, and without exact ties the dendrogram is the one the chain finds.
//
// A slot is a cluster; slot k starts as row k, and a merged pair lives on in its smaller slot (a slot is the smallest row of its
// cluster).  D is the dense N x N float64 matrix of unsquared distances, +inf on the diagonal, bitwise symmetric.
//
//   pd_norm_kernel (pair_dist.hpp)   |x_i|^2 in float64
//   ward_dist_kernel    one workgroup (4 waves) per 64 x 64 tile on or above the diagonal: pd_tile_f64 forms d^2 on the float64 MFMA
//                       (near pairs again from differences), and the lane that holds (i, j), i < j, stores sqrt(d^2) to (i, j) and
//                       to (j, i): one value, two places
//   one round:
//   ward_nn_kernel      nn[i] = the nearest active slot of slot i, ties to the smallest index, one wave per slot that needs it: a slot
//                       that merged last round, or whose cached neighbour did.  Every other slot keeps its cache: neither it nor its
//                       neighbour changed, and by reducibility no merged cluster came closer than that neighbour.
//   ward_pair_kernel    (one workgroup) part[k] = nn[k] where nn[nn[k]] == k, else -1; the pairs k < part[k] are logged in ascending k
//                       behind the earlier rounds' (a prefix sum gives the places): (k, part[k]), the height D[k][part[k]], the size
//   ward_update_kernel  one thread per (merged pair A = (i, j), surviving slot k): the Lance-Williams update as scipy's _ward forms it,
//                       on unsquared distances.  k unmerged: d(A, k) from D[i][k], D[j][k] and A's height.  k = x the survivor of a
//                       pair B = (x, y) merged in the same round: the thread of the pair with the smaller slot owns (A, B); it merges
//                       the columns first, d(i, B) and d(j, B) from the 2 x 2 block D[i|j][x|y] and B's height, then the rows.  The
//                       result goes to D[i][k] and D[k][i].  A thread reads only entries between members of its own two groups and
//                       writes two of them, and the entry between the two members of one group (its height) is written by none, so
//                       no entry is read after another thread wrote it and the result does not depend on the order of workgroups.
//   ward_finish_kernel  size[i] = the logged size, size[j] = 0: a dead slot is never read again
// A round with one active cluster finds no pair and changes nothing, so rounds can be enqueued without reading back in between.
// No floating-point atomics: the same input gives the same bits.
#include "common.hpp"
#include "km_sort.hpp"
#include "pair_dist.hpp"

namespace g2v {
namespace {

constexpr int WARD_MAX_E = 512;
constexpr int64_t WARD_MAX_ROWS = 32768;    // D is 8 N^2 bytes: 8 GiB here
constexpr int WARD_GROUPS = 64;             // merged pairs that ward_update_kernel walks side by side (gridDim.y)
enum { WC_MERGES = 0, WC_ROUNDS = 1, WC_LAST = 2, WC_BASE = 3, WC_COUNT = 4 };    // counters: merges logged, rounds that merged,
                                                                                  // the last round's merges and where its log begins

inline bool ward_shape_ok(int64_t N, int E) { return N >= 1 && N <= WARD_MAX_ROWS && E >= 1 && E <= WARD_MAX_E; }

__global__ __launch_bounds__(256) void ward_dist_kernel(const float* __restrict__ x, int64_t ld, int N, int E,
                                                       const double* __restrict__ norm, double* __restrict__ D) {
  __shared__ __attribute__((aligned(16))) float sa[PD_TILE * PD_LD];
  __shared__ __attribute__((aligned(16))) float sb[PD_TILE * PD_LD];
  if (blockIdx.x < blockIdx.y) return;                       // (workgroup-uniform) below the diagonal: written from above
  const int64_t a0 = (int64_t)blockIdx.y * PD_TILE;
  const int b0 = (int)blockIdx.x * PD_TILE;
  double nr[4];
  pd_row_norms_f64(norm, N, a0, nr);
  pd_tile_f64(x, ld, N, a0, nr, x, ld, N, b0, norm, E, true, sa, sb, [&](int64_t row, int col, const double (&dd)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t rr = row + 4 * r;
      if (rr >= N || col >= N) continue;
      if (rr == col) {
        D[rr * N + col] = (double)__builtin_inff();
      } else if (rr < col) {                                 // (a diagonal tile holds (i, j) and (j, i): the upper one is stored)
        const double v = sqrt(dd[r]);
        D[rr * N + col] = v;
        D[(int64_t)col * N + rr] = v;
      }
    }
  });
}

__global__ __launch_bounds__(256) void ward_init_kernel(int N, int* __restrict__ size, int* __restrict__ nn, int* __restrict__ part,
                                                       int64_t* __restrict__ counters) {
  const int k = (int)blockIdx.x * 256 + threadIdx.x;
  if (k < WC_COUNT) counters[k] = 0;
  if (k >= N) return;
  size[k] = 1;
  nn[k] = -1;
  part[k] = k;                                               // >= 0: every slot scans in the first round
}

__global__ __launch_bounds__(256) void ward_nn_kernel(const double* __restrict__ D, int N, const int* __restrict__ size,
                                                     const int* __restrict__ part, int* __restrict__ nn) {
  const int lane = threadIdx.x & 63;
  const int i = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N || size[i] == 0) return;                        // (wave-uniform)
  const int c = nn[i];
  const bool cached = part[i] < 0 && (c < 0 || ((unsigned)c < (unsigned)N && part[c] < 0));
  if (cached) return;
  const double* row = D + (int64_t)i * N;
  double best = (double)__builtin_inff();
  int bj = -1;
  for (int j = lane; j < N; j += 64) {
    if (j == i || size[j] == 0) continue;
    const double v = row[j];
    if (bj < 0 || v < best) {
      best = v;
      bj = j;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {                         // (value, index) in lexicographic order: ties to the smallest index
    const double ob = __shfl_xor(best, o);
    const int oj = __shfl_xor(bj, o);
    if (oj >= 0 && (bj < 0 || ob < best || (ob == best && oj < bj))) {
      best = ob;
      bj = oj;
    }
  }
  if (lane == 0) nn[i] = bj;
}

__device__ __forceinline__ int ward_mutual(int k, int N, const int* __restrict__ size, const int* __restrict__ nn) {
  if (size[k] == 0) return -1;
  const int j = nn[k];
  return (unsigned)j < (unsigned)N && j != k && size[j] > 0 && nn[j] == k ? j : -1;
}

__global__ __launch_bounds__(1024) void ward_pair_kernel(const double* __restrict__ D, int N, const int* __restrict__ size,
                                                        const int* __restrict__ nn, int* __restrict__ part, int* __restrict__ pairs,
                                                        double* __restrict__ heights, int* __restrict__ sizes,
                                                        int64_t* __restrict__ counters) {
  __shared__ int s[1024];
  const int tid = threadIdx.x;
  const int per = (N + 1023) / 1024, lo = min(N, tid * per), hi = min(N, lo + per);
  const int64_t base = counters[WC_MERGES];
  int c = 0;
  for (int k = lo; k < hi; ++k) {
    const int j = ward_mutual(k, N, size, nn);
    part[k] = j;
    c += j > k ? 1 : 0;
  }
  s[tid] = c;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {                       // inclusive scan
    const int a = tid >= o ? s[tid - o] : 0;
    __syncthreads();
    s[tid] += a;
    __syncthreads();
  }
  int64_t pos = base + s[tid] - c;
  for (int k = lo; k < hi; ++k) {
    const int j = ward_mutual(k, N, size, nn);
    if (j > k && pos < N - 1) {                              // (N - 1 merges end in one cluster: never beyond the log)
      pairs[2 * pos] = k;
      pairs[2 * pos + 1] = j;
      heights[pos] = D[(int64_t)k * N + j];
      sizes[pos] = size[k] + size[j];
      ++pos;
    }
  }
  if (tid == 1023) {
    const int64_t m = min((int64_t)s[1023], (int64_t)(N - 1) - base);
    counters[WC_MERGES] = base + m;
    counters[WC_ROUNDS] += m > 0 ? 1 : 0;
    counters[WC_LAST] = m;
    counters[WC_BASE] = base;
  }
}

// scipy's _ward: the distance from cluster i to the union of x and y, from unsquared distances (a negative rounding residue of a
// difference that is zero in exact arithmetic gives 0, not NaN)
__device__ __forceinline__ double ward_dist(double dxi, double dyi, double dxy, int nx, int ny, int ni) {
  const double t = 1.0 / (double)(nx + ny + ni);
  return sqrt(fmax((double)(ni + nx) * t * dxi * dxi + (double)(ni + ny) * t * dyi * dyi - (double)ni * t * dxy * dxy, 0.0));
}

__global__ __launch_bounds__(256) void ward_update_kernel(double* __restrict__ D, int N, const int* __restrict__ size,
                                                         const int* __restrict__ part, const int* __restrict__ pairs,
                                                         const double* __restrict__ heights, const int64_t* __restrict__ counters) {
  const int k = (int)blockIdx.x * 256 + threadIdx.x;
  const int m = (int)counters[WC_LAST];
  const int64_t base = counters[WC_BASE];
  if (k >= N || size[k] == 0) return;
  const int pk = part[k];
  if (pk >= 0 && pk < k) return;                             // the larger slot of a pair: dead after this round
  const int nk = size[k];
  for (int p = blockIdx.y; p < m; p += gridDim.y) {
    const int i = pairs[2 * (base + p)], j = pairs[2 * (base + p) + 1];
    if (pk >= 0 && k <= i) continue;                         // k survives a pair of its own: the pair with the smaller slot owns it
    const double hA = heights[base + p];
    const int ni = size[i], nj = size[j];
    const double* ri = D + (int64_t)i * N;
    const double* rj = D + (int64_t)j * N;
    double v;
    if (pk < 0) {
      v = ward_dist(ri[k], rj[k], hA, ni, nj, nk);
    } else {                                                 // columns first: B = (k, pk) as seen from i and from j; then the rows
      const int ny = size[pk];
      const double hB = D[(int64_t)k * N + pk];              // (written by no thread: the height ward_pair_kernel logged for B)
      const double diB = ward_dist(ri[k], ri[pk], hB, nk, ny, ni);
      const double djB = ward_dist(rj[k], rj[pk], hB, nk, ny, nj);
      v = ward_dist(diB, djB, hA, ni, nj, nk + ny);
    }
    D[(int64_t)i * N + k] = v;
    D[(int64_t)k * N + i] = v;
  }
}

__global__ __launch_bounds__(256) void ward_finish_kernel(int* __restrict__ size, const int* __restrict__ pairs,
                                                         const int* __restrict__ sizes, const int64_t* __restrict__ counters) {
  const int p = (int)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int)counters[WC_LAST]) return;
  const int64_t at = counters[WC_BASE] + p;
  size[pairs[2 * at]] = sizes[at];
  size[pairs[2 * at + 1]] = 0;
}

}  // namespace
}  // namespace g2v

using namespace g2v;

extern "C" int64_t g2v_ward_max_rows(void) { return WARD_MAX_ROWS; }

extern "C" size_t g2v_ward_workspace(int64_t N, int E) {
  if (!ward_shape_ok(N, E)) return 0;
  return km_align((size_t)N * sizeof(double));
}

extern "C" int g2v_ward_distances(const float* x, int64_t ld, int64_t N, int E, double* D, void* workspace, size_t workspace_bytes,
                                  g2v_stream_t stream) {
  G2V_REQUIRE(x && D && workspace, "null pointer");
  G2V_REQUIRE(N >= 1 && E >= 1, "sizes: N >= 1, E >= 1");
  if (!ward_shape_ok(N, E)) {
    set_error("g2v_ward_distances: needs N <= %lld (the distance matrix is 8 N^2 bytes) and E <= %d (N = %lld, E = %d)",
              (long long)WARD_MAX_ROWS, WARD_MAX_E, (long long)N, E);
    return G2V_ERR_UNSUPPORTED;
  }
  G2V_REQUIRE(ld >= E && (ld & 3) == 0, "row stride smaller than E or not a multiple of 4");
  G2V_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(D) & 7) == 0,
              "x and workspace must be 16-byte aligned, D 8-byte aligned");
  if (workspace_bytes < g2v_ward_workspace(N, E)) {
    set_error("g2v_ward_distances: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  double* norm = (double*)workspace;
  const int W = cdiv(N, PD_TILE);
  hipLaunchKernelGGL(pd_norm_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, x, ld, N, E, norm);
  hipLaunchKernelGGL(ward_dist_kernel, dim3(W, W), dim3(256), 0, st, x, ld, (int)N, E, (const double*)norm, D);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int g2v_ward_rounds(double* D, int64_t N, int32_t* size, int32_t* nn, int32_t* part, int init, int rounds, int32_t* pairs,
                               double* heights, int32_t* sizes, int64_t* counters, g2v_stream_t stream) {
  G2V_REQUIRE(D && size && nn && part && pairs && heights && sizes && counters, "null pointer");
  G2V_REQUIRE(N >= 1 && rounds >= 1, "sizes: N >= 1, rounds >= 1");
  if (N > WARD_MAX_ROWS) {
    set_error("g2v_ward_rounds: needs N <= %lld (N = %lld)", (long long)WARD_MAX_ROWS, (long long)N);
    return G2V_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  const int n = (int)N;
  if (init) hipLaunchKernelGGL(ward_init_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, n, (int*)size, (int*)nn, (int*)part, counters);
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(ward_nn_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, (const double*)D, n, (const int*)size, (const int*)part,
                       (int*)nn);
    hipLaunchKernelGGL(ward_pair_kernel, dim3(1), dim3(1024), 0, st, (const double*)D, n, (const int*)size, (const int*)nn, (int*)part,
                       (int*)pairs, heights, (int*)sizes, counters);
    hipLaunchKernelGGL(ward_update_kernel, dim3(cdiv(N, 256), WARD_GROUPS), dim3(256), 0, st, D, n, (const int*)size, (const int*)part,
                       (const int*)pairs, (const double*)heights, (const int64_t*)counters);
    hipLaunchKernelGGL(ward_finish_kernel, dim3(cdiv(cdiv(N, 2), 256)), dim3(256), 0, st, (int*)size, (const int*)pairs,
                       (const int*)sizes, (const int64_t*)counters);
  }
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
