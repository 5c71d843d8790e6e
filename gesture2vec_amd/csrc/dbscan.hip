// dbscan.hip -- DBSCAN over (N, E) fp32 latent rows, labelled as sklearn.cluster.DBSCAN(eps, min_samples).fit labels them
// (gesture2vec_amd/dbscan.py; the reference's Clustering.py:742-750).  sklearn's dbscan_inner is sequential, but its result is fixed
// by the eps-graph alone.  With adj(i, j) <=> |x_i - x_j| <= eps (a row is its own neighbour):
//   core(i)  <=> #{j : adj(i, j)} >= min_samples
//   root(i), for core i = the smallest index in i's connected component of the graph of core rows under adj
//   the cluster id of a component = the rank of its root among all roots in ascending order
//   a non-core row with a core neighbour gets the smallest cluster id among its core neighbours (= the id of the smallest root
//   among them: the first cluster to reach it keeps it); without one it gets -1
//
//   pd_norm_kernel (pair_dist.hpp)   |x_i|^2 in float64
//   dbs_adj_kernel      one workgroup (4 waves) per 64 x 64 tile of the N x N matrix: pd_tile forms d^2, and the callback decides
//                       d^2 <= eps^2.  A pair with |d^2 - eps^2| <= DBS_BAND (n_i + n_j) is not decided on the Gram form: the wave
//                       evaluates it again as sum (x_i - x_j)^2 in float64 (pd_pair_sq through pd_near_pairs) and decides on that, so
//                       every bit is the float64 decision of the fp32 rows.  The 16 lanes that hold 16 consecutive columns of one
//                       row give their bits with one ballot; after the four column groups a lane holds the row's whole 64-bit word
//                       and stores it.  Every word of the bitmap has one writer; tile (a, b) is the transpose of tile (b, a) bit for
//                       bit (pd_tile's property; pd_pair_sq(a, b) has the bits of pd_pair_sq(b, a); n_i + n_j commutes).
//   dbs_count_kernel    counts[i] = popcount of row i, one wave per row
//   dbs_init_kernel     L[i] = i for a core row, N for any other: N is larger than every index, so a minimum over neighbours skips
//                       the rows that are not core without a second array
//   dbs_min_kernel      one round, one wave per core row: B[i] = min(A[i], min {A[j] : adj(i, j)}) over the bitmap row
//   dbs_jump_kernel     pointer jumping A[i] = B[B[i]] (B[k] <= k, so it only descends), and flag = 1 where a row ends the round
//                       with another value than it began with.  A round reads one array and writes the other: what it gives does
//                       not depend on the order in which workgroups run, and none waits on another.  L is monotone and bounded
//                       below by the root, so the rounds end; at the fixed point L is constant on a component and L[root] = root.
//   dbs_rank_kernel     exclusive prefix sum of the flag L[i] == i over all rows (one workgroup): the rank of every root
//   dbs_label_kernel    a core row gets rank[L[i]]; any other row the rank of the smallest L among its neighbours, or -1
//   dbs_finish_kernel   out = { clusters, core rows, noise rows } (integer sums)
// Distances are formed once; everything after dbs_adj_kernel reads the bitmap.  No floating-point atomics: the same input gives the
// same bits.
#include "common.hpp"
#include "km_sort.hpp"
#include "pair_dist.hpp"

namespace g2v {
namespace {

typedef unsigned long long u64;

constexpr int DBS_MAX_E = 512;
constexpr int64_t DBS_MAX_ROWS = 131072;    // the bitmap is N^2 / 8 bytes: 2 GiB here
// The band.  G = x_i.x_j is summed in fp32 chains of PD_KC = 32 columns that are folded in float64 (pair_dist.hpp): a chain of m
// fmas is within m 2^-24 sum_k |a_k b_k| <= m 2^-25 sum_k (a_k^2 + b_k^2) of its exact value, so over all chunks
// |G - x_i.x_j| <= 32 * 2^-25 (n_i + n_j), and d^2 = n_i + n_j - 2 G is within 32 * 2^-24 (n_i + n_j).  Rounding d^2 <= 2 (n_i + n_j)
// to fp32 once adds 2 * 2^-24 (n_i + n_j); the float64 norms and folds are 1e-9 of that.  34 * 2^-24 in all; the band is 64 * 2^-24.
// (pair_dist.hpp states the typical error, 2e-5 at E = 400 on rows of unit entries = 2.5e-8 (n_i + n_j): 150 times inside.)
constexpr double DBS_BAND = 1.0 / 262144.0;

struct DbsLayout {
  size_t norm, rank, hdr, total;
};

inline DbsLayout dbs_layout(int64_t N) {
  DbsLayout l;
  size_t o = 0;
  l.norm = o;  o = km_align(o + (size_t)N * sizeof(double));
  l.rank = o;  o = km_align(o + (size_t)N * sizeof(int));
  l.hdr = o;   o = km_align(o + sizeof(int64_t));
  l.total = o;
  return l;
}

inline bool dbs_shape_ok(int64_t N, int E) { return N >= 1 && N <= DBS_MAX_ROWS && E >= 1 && E <= DBS_MAX_E; }

__global__ __launch_bounds__(256) void dbs_adj_kernel(const float* __restrict__ x, int64_t ld, int N, int E,
                                                     const double* __restrict__ norm, double eps2, u64* __restrict__ bitmap,
                                                     int W) {
  __shared__ __attribute__((aligned(16))) float sa[PD_TILE * PD_LD];
  __shared__ __attribute__((aligned(16))) float sb[PD_TILE * PD_LD];
  const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t a0 = (int64_t)blockIdx.y * PD_TILE;
  const int b0 = (int)blockIdx.x * PD_TILE;
  const int64_t wrow = a0 + 16 * wave;
  double nr[4];
  pd_row_norms(norm, N, a0, nr);
  u64 word[4] = {0ull, 0ull, 0ull, 0ull};                    // word[r]: row wrow + 4 q + r, columns b0 .. b0 + 63
  pd_tile(x, ld, N, a0, nr, x, ld, N, b0, norm, E, true, sa, sb, [&](int64_t row, int col, const float (&dd)[4]) {
    const int j = (col - b0) >> 4;                           // col = b0 + 16 j + i
    const double nc = col < N ? norm[col] : 0.0;
    double ex[4];
    unsigned nm = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ex[r] = (double)dd[r];                                 // +inf where the row or the column is past the end
      const bool band = dd[r] < __builtin_inff() && fabs(ex[r] - eps2) <= DBS_BAND * (nr[r] + nc);
      nm |= band ? (1u << r) : 0u;
    }
    pd_near_pairs(nm, lane, ex, [&](int L, int r) {
      return pd_pair_sq(x + (wrow + 4 * (L >> 4) + r) * ld, x + (int64_t)(b0 + 16 * j + (L & 15)) * ld, E, lane);
    });
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const u64 bal = __ballot(ex[r] <= eps2);               // bits 16 q' .. 16 q' + 15: row 4 q' + r, columns 16 j .. 16 j + 15
      word[r] |= ((bal >> (16 * q)) & 0xffffull) << (16 * j);
    }
  });
  if (i < 4) {
    const int64_t row = wrow + 4 * q + i;
    const u64 w = i == 0 ? word[0] : i == 1 ? word[1] : i == 2 ? word[2] : word[3];
    if (row < N) bitmap[row * W + blockIdx.x] = w;
  }
}

__global__ __launch_bounds__(256) void dbs_count_kernel(const u64* __restrict__ bitmap, int N, int W, int64_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int row = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const u64* p = bitmap + (int64_t)row * W;
  int c = 0;
  for (int w = lane; w < W; w += 64) c += __popcll(p[w]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) counts[row] = c;
}

__global__ __launch_bounds__(256) void dbs_init_kernel(const int64_t* __restrict__ counts, int N, int64_t min_samples,
                                                      int* __restrict__ L) {
  const int r = (int)blockIdx.x * 256 + threadIdx.x;
  if (r < N) L[r] = counts[r] >= min_samples ? r : N;
}

// the smallest A[j] over the set bits j of bitmap row `row`, by a whole wave; every lane returns the same value (N: none)
__device__ __forceinline__ int dbs_row_min(const u64* __restrict__ bitmap, int row, int N, int W, const int* __restrict__ A, int lane) {
  const u64* p = bitmap + (int64_t)row * W;
  int m = N;
  for (int w = lane; w < W; w += 64) {
    u64 bits = p[w];
    while (bits) {
      const int j = 64 * w + __ffsll((long long)bits) - 1;
      bits &= bits - 1;
      if (j < N) m = min(m, A[j]);                           // (g2v_dbscan_neighbors leaves the bits past N zero; a caller's own bitmap may not)
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
  return m;
}

__global__ __launch_bounds__(256) void dbs_min_kernel(const u64* __restrict__ bitmap, int N, int W, const int* __restrict__ A,
                                                     int* __restrict__ B) {
  const int lane = threadIdx.x & 63;
  const int row = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const int own = A[row];
  int m = own;
  if (own < N) m = min(own, dbs_row_min(bitmap, row, N, W, A, lane));     // (wave-uniform: a core row)
  if (lane == 0) B[row] = m;
}

__global__ __launch_bounds__(256) void dbs_jump_kernel(const int* __restrict__ B, int N, int* __restrict__ A, int* __restrict__ flag) {
  const int r = (int)blockIdx.x * 256 + threadIdx.x;
  if (r >= N) return;
  const int b = B[r];
  const int v = (unsigned)b < (unsigned)N ? B[b] : N;        // (never an address outside L, whatever L held on entry)
  if (v != A[r]) *flag = 1;                                  // (every writer stores the same value)
  A[r] = v;
}

__global__ __launch_bounds__(1024) void dbs_rank_kernel(const int* __restrict__ L, int N, int* __restrict__ rank,
                                                       int64_t* __restrict__ hdr) {
  __shared__ int s[1024];
  const int tid = threadIdx.x;
  const int per = (N + 1023) / 1024, lo = min(N, tid * per), hi = min(N, lo + per);
  int c = 0;
  for (int r = lo; r < hi; ++r) c += L[r] == r ? 1 : 0;
  s[tid] = c;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {                       // inclusive scan
    const int a = tid >= o ? s[tid - o] : 0;
    __syncthreads();
    s[tid] += a;
    __syncthreads();
  }
  int run = s[tid] - c;
  for (int r = lo; r < hi; ++r) {
    rank[r] = run;
    run += L[r] == r ? 1 : 0;
  }
  if (tid == 1023) hdr[0] = s[1023];
}

__global__ __launch_bounds__(256) void dbs_label_kernel(const u64* __restrict__ bitmap, int N, int W, const int* __restrict__ L,
                                                       const int* __restrict__ rank, int64_t* __restrict__ labels,
                                                       uint8_t* __restrict__ core) {
  const int lane = threadIdx.x & 63;
  const int row = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const int own = L[row];
  const int m = own < N ? own : dbs_row_min(bitmap, row, N, W, L, lane);
  if (lane == 0) {
    labels[row] = (unsigned)m < (unsigned)N ? (int64_t)rank[m] : (int64_t)-1;
    core[row] = (unsigned)own < (unsigned)N ? 1 : 0;
  }
}

__global__ __launch_bounds__(1024) void dbs_finish_kernel(const int64_t* __restrict__ labels, const uint8_t* __restrict__ core, int N,
                                                         const int64_t* __restrict__ hdr, int64_t* __restrict__ out) {
  __shared__ int sc[1024], sn[1024];
  const int tid = threadIdx.x;
  int c = 0, n = 0;
  for (int r = tid; r < N; r += 1024) {
    c += core[r];
    n += labels[r] < 0 ? 1 : 0;
  }
  sc[tid] = c;
  sn[tid] = n;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (tid < s) {
      sc[tid] += sc[tid + s];
      sn[tid] += sn[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = hdr[0];
    out[1] = sc[0];
    out[2] = sn[0];
  }
}

}  // namespace
}  // namespace g2v

using namespace g2v;

extern "C" int64_t g2v_dbscan_max_rows(void) { return DBS_MAX_ROWS; }

extern "C" size_t g2v_dbscan_workspace(int64_t N, int E) {
  if (!dbs_shape_ok(N, E)) return 0;
  return dbs_layout(N).total;
}

extern "C" int g2v_dbscan_neighbors(const float* x, int64_t ld, int64_t N, int E, double eps, uint64_t* bitmap, int64_t* counts,
                                    void* workspace, size_t workspace_bytes, g2v_stream_t stream) {
  G2V_REQUIRE(x && bitmap && counts && workspace, "null pointer");
  G2V_REQUIRE(N >= 1 && E >= 1, "sizes: N >= 1, E >= 1");
  G2V_REQUIRE(eps >= 0.0 && eps < (double)__builtin_inff(), "eps must be finite and >= 0");
  if (!dbs_shape_ok(N, E)) {
    set_error("g2v_dbscan_neighbors: needs N <= %lld (the adjacency bitmap is N^2 / 8 bytes) and E <= %d (N = %lld, E = %d)",
              (long long)DBS_MAX_ROWS, DBS_MAX_E, (long long)N, E);
    return G2V_ERR_UNSUPPORTED;
  }
  G2V_REQUIRE(ld >= E && (ld & 3) == 0, "row stride smaller than E or not a multiple of 4");
  G2V_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(bitmap) & 7) == 0,
              "x and workspace must be 16-byte aligned, bitmap 8-byte aligned");
  const DbsLayout l = dbs_layout(N);
  if (workspace_bytes < l.total) {
    set_error("g2v_dbscan_neighbors: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  double* norm = (double*)((char*)workspace + l.norm);
  const int W = cdiv(N, 64);
  hipLaunchKernelGGL(pd_norm_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, x, ld, N, E, norm);
  hipLaunchKernelGGL(dbs_adj_kernel, dim3(W, W), dim3(256), 0, st, x, ld, (int)N, E, (const double*)norm, eps * eps, (u64*)bitmap, W);
  hipLaunchKernelGGL(dbs_count_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, (const u64*)bitmap, (int)N, W, counts);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int g2v_dbscan_propagate(const uint64_t* bitmap, const int64_t* counts, int64_t N, int64_t min_samples, int init, int rounds,
                                    int32_t* L, int32_t* tmp, int32_t* flags, g2v_stream_t stream) {
  G2V_REQUIRE(bitmap && counts && L && tmp && flags, "null pointer");
  G2V_REQUIRE(N >= 1 && rounds >= 1, "sizes: N >= 1, rounds >= 1");
  if (N > DBS_MAX_ROWS) {
    set_error("g2v_dbscan_propagate: needs N <= %lld (N = %lld)", (long long)DBS_MAX_ROWS, (long long)N);
    return G2V_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  const int W = cdiv(N, 64);
  if (init) hipLaunchKernelGGL(dbs_init_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, counts, (int)N, min_samples, (int*)L);
  (void)hipMemsetAsync(flags, 0, (size_t)rounds * sizeof(int32_t), st);
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(dbs_min_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, (const u64*)bitmap, (int)N, W, (const int*)L, (int*)tmp);
    hipLaunchKernelGGL(dbs_jump_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, (const int*)tmp, (int)N, (int*)L, (int*)flags + r);
  }
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int g2v_dbscan_labels(const uint64_t* bitmap, const int32_t* L, int64_t N, int64_t* labels, uint8_t* core, int64_t* out,
                                 void* workspace, size_t workspace_bytes, g2v_stream_t stream) {
  G2V_REQUIRE(bitmap && L && labels && core && out && workspace, "null pointer");
  G2V_REQUIRE(N >= 1, "sizes: N >= 1");
  if (N > DBS_MAX_ROWS) {
    set_error("g2v_dbscan_labels: needs N <= %lld (N = %lld)", (long long)DBS_MAX_ROWS, (long long)N);
    return G2V_ERR_UNSUPPORTED;
  }
  G2V_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "workspace must be 16-byte aligned");
  const DbsLayout l = dbs_layout(N);
  if (workspace_bytes < l.total) {
    set_error("g2v_dbscan_labels: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  int* rank = (int*)((char*)workspace + l.rank);
  int64_t* hdr = (int64_t*)((char*)workspace + l.hdr);
  const int W = cdiv(N, 64);
  hipLaunchKernelGGL(dbs_rank_kernel, dim3(1), dim3(1024), 0, st, (const int*)L, (int)N, rank, hdr);
  hipLaunchKernelGGL(dbs_label_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, (const u64*)bitmap, (int)N, W, (const int*)L,
                     (const int*)rank, labels, core);
  hipLaunchKernelGGL(dbs_finish_kernel, dim3(1), dim3(1024), 0, st, (const int64_t*)labels, (const uint8_t*)core, (int)N,
                     (const int64_t*)hdr, out);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
