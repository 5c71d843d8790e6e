// map_quality.hip -- the rank of given neighbours among ALL rows, without the M x N distance matrix: the kernel behind
// trustworthiness and continuity of a latent map (gesture2vec_amd/embedding.py: trustworthiness, continuity, map_quality,
// placement_quality; sklearn.manifold.trustworthiness, sklearn 1.7, Euclidean).  X (N, d) are the reference rows, Z (M, d) the
// query rows, idx (M, k) rows of X listed per query (its k nearest rows in the OTHER space, from g2v_tsne_place_neighbors).
//   rank[m][s] = 1 + #{ l in [0, N), l != self[m] : (D(m, l), l) < (D(m, j), j) },  j = idx[m][s], lexicographic,
//   D(m, l) = sum (z_m - x_l)^2 in float64 from the differences (pd_pair_sq).  An entry outside [0, N) or equal to self[m]: rank 0.
//
//   pd_norm_kernel (pair_dist.hpp)   |row|^2 in float64 of both row sets
//   nr_rank_kernel      one workgroup (4 waves) per 64 query rows and per slice of the column tiles.  First the thresholds
//                       D(m, j) of its 64 x k listed pairs, exactly (pd_pair_sq, one wave per pair), into LDS beside j and a zeroed
//                       count.  Then it walks its 64-column tiles of X: pd_tile forms the fp32 d^2, and the callback compares
//                       each with the k thresholds of its row.  The 16 lanes that hold 16 consecutive columns of one row give
//                       their verdicts with one ballot, and a popcount is added to the row's count in LDS (integer atomics: every
//                       count is the same number in whatever order the adds land).  A comparison with
//                       |d^2 - thr| <= NR_BAND (n_m + n_l) is not trusted: the wave evaluates that pair again as sum (z - x)^2
//                       in float64 (pd_pair_sq through pd_near_pairs, as dbscan.hip does around eps^2), compares exact with exact
//                       -- equal distances go to the lower index -- and corrects the counts it had added.  The listed pair
//                       itself (l == j) is never less than itself and is not looked at.  At the end the counts are added to
//                       rank (zeroed by the entry point) with integer atomics; the slice that holds column tile 0 adds the 1.
// Integer sums only: the same input gives the same bits, whatever the number of slices.  No environment variable is read.
#include "common.hpp"
#include "km_sort.hpp"
#include "pair_dist.hpp"

namespace g2v {
namespace {

constexpr int NR_MAX_D = 512;
constexpr int NR_MAX_K = 127;
constexpr int64_t NR_MAX_N = (1 << 24) - 1;
constexpr int64_t NR_MAX_M = 2147483647LL;
constexpr int NR_MAX_SLICES = 1024;
// The band (the derivation at DBS_BAND in dbscan.hip, restated).  G = z_m.x_l is summed in fp32 chains of PD_KC = 32 columns that
// are folded in float64 (pair_dist.hpp): a chain of c fmas is within c 2^-24 sum_k |a_k b_k| <= c 2^-25 sum_k (a_k^2 + b_k^2) of
// its exact value, so over all chunks |G - z_m.x_l| <= 32 * 2^-25 (n_m + n_l), and d^2 = n_m + n_l - 2 G is within
// 32 * 2^-24 (n_m + n_l).  Rounding d^2 <= 2 (n_m + n_l) to fp32 once adds 2 * 2^-24 (n_m + n_l); the float64 norms and folds
// are 1e-9 of that.  34 * 2^-24 in all; the band is 64 * 2^-24.  The threshold is exact (float64 from differences, 1e-16
// relative), so a comparison outside the band has the sign of the exact one.
constexpr double NR_BAND = 1.0 / 262144.0;

inline size_t nr_norm_offset(int64_t N) { return km_align((size_t)N * sizeof(double)); }

inline bool nr_shape_ok(int64_t N, int64_t M, int d, int k) {
  return N >= 1 && N <= NR_MAX_N && M >= 1 && M <= NR_MAX_M && d >= 1 && d <= NR_MAX_D && k >= 1 && k <= NR_MAX_K;
}

// dynamic LDS of 64 rows x k entries: thr double | cnt int | lj int (16 k bytes per row: 127 KiB at k = 127)
inline size_t nr_lds_bytes(int k) { return (size_t)PD_TILE * k * 16; }

__global__ __launch_bounds__(256) void nr_rank_kernel(const float* __restrict__ X, int64_t ldx, int N, const float* __restrict__ Z,
                                                     int64_t ldz, int64_t M, int d, const int64_t* __restrict__ self,
                                                     const int* __restrict__ idx, int k, const double* __restrict__ nx,
                                                     const double* __restrict__ nz, int* __restrict__ rank,
                                                     unsigned long long* __restrict__ redecided) {
  __shared__ __attribute__((aligned(16))) float sa[PD_TILE * PD_LD];
  __shared__ __attribute__((aligned(16))) float sb[PD_TILE * PD_LD];
  extern __shared__ __attribute__((aligned(16))) double nr_lds[];
  double* thr = nr_lds;
  int* cnt = reinterpret_cast<int*>(nr_lds + PD_TILE * k);
  int* lj = cnt + PD_TILE * k;
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t i0 = (int64_t)blockIdx.x * PD_TILE;
  const double inf = (double)__builtin_inff();

  // the thresholds: one wave per listed pair (e is wave-uniform)
  for (int e = wave; e < PD_TILE * k; e += 4) {
    const int64_t m = i0 + e / k;
    int j = -1;
    if (m < M) {
      j = idx[m * k + (e % k)];
      const int64_t sf = self ? self[m] : -1;
      if ((unsigned)j >= (unsigned)N || (int64_t)j == sf) j = -1;
    }
    const double v = j >= 0 ? pd_pair_sq(Z + m * ldz, X + (int64_t)j * ldx, d, lane) : -inf;
    if (lane == 0) {
      thr[e] = v;                                             // -inf: nothing is below it and nothing is near it
      lj[e] = j;
      cnt[e] = 0;
    }
  }

  const int64_t wrow = i0 + 16 * wave, row0 = wrow + 4 * q;   // this lane's rows in pd_tile's epilogue: row0 + r
  const int lr0 = 16 * wave + 4 * q;
  double nr[4];
  pd_row_norms(nz, M, i0, nr);
  int sf[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t s = (self && row0 + r < M) ? self[row0 + r] : -1;
    sf[r] = (s >= 0 && s < N) ? (int)s : -1;
  }
  const int tiles = (N + PD_TILE - 1) / PD_TILE;
  const int t_lo = (int)((int64_t)blockIdx.y * tiles / gridDim.y), t_hi = (int)((int64_t)(blockIdx.y + 1) * tiles / gridDim.y);
  unsigned redo = 0;

  for (int t = t_lo; t < t_hi; ++t) {
    const int b0 = t * PD_TILE;
    // (pd_tile's first barrier: the thresholds are set)
    pd_tile(Z, ldz, M, i0, nr, X, ldx, N, b0, nx, d, false, sa, sb, [&](int64_t row, int col, const float (&dd)[4]) {
      const int jt = (col - b0) >> 4;                         // col = b0 + 16 jt + i
      const double nc = col < N ? nx[col] : 0.0;
      double ap[4];
      unsigned nm = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) ap[r] = col == sf[r] ? inf : (double)dd[r];     // +inf past the end of either set, too
      for (int s0 = 0; s0 < k; s0 += 16) {
        int mine[4] = {0, 0, 0, 0};
        const int sn = min(16, k - s0);
        for (int u = 0; u < sn; ++u) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int e = (lr0 + r) * k + s0 + u;
            const double th = thr[e];
            const bool other = col != lj[e];
            const bool less = other && ap[r] < th;
            const bool band = other && ap[r] < inf && fabs(ap[r] - th) <= NR_BAND * (nr[r] + nc);
            nm |= band ? (1u << r) : 0u;
            const unsigned long long bal = __ballot(less);   // bits 16 q' .. 16 q' + 15: row 4 q' + r, columns 16 jt .. 16 jt + 15
            const int c = __popc((unsigned)(bal >> (16 * q)) & 0xffffu);
            mine[r] = i == u ? c : mine[r];
          }
        }
        if (i < sn) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (mine[r]) atomicAdd(&cnt[(lr0 + r) * k + s0 + i], mine[r]);
        }
      }
      if (__ballot(nm != 0)) {                                // (wave-uniform, rare) decide the pairs inside the band again
        double ex[4] = {ap[0], ap[1], ap[2], ap[3]};
        pd_near_pairs(nm, lane, ex, [&](int L, int r) {
          return pd_pair_sq(Z + (wrow + 4 * (L >> 4) + r) * ldz, X + (int64_t)(b0 + 16 * jt + (L & 15)) * ldx, d, lane);
        });
        redo += __popc(nm);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if ((nm >> r) & 1u) {
            for (int s = 0; s < k; ++s) {
              const int e = (lr0 + r) * k + s;
              const double th = thr[e];
              const int js = lj[e];
              const bool other = col != js;
              const bool was = other && ap[r] < th;
              const bool is = other && (ex[r] < th || (ex[r] == th && col < js));
              if (was != is) atomicAdd(&cnt[e], is ? 1 : -1);
            }
          }
        }
      }
    });
  }
  __syncthreads();
  for (int e = tid; e < PD_TILE * k; e += 256) {
    const int64_t m = i0 + e / k;
    const int v = cnt[e] + ((blockIdx.y == 0 && lj[e] >= 0) ? 1 : 0);
    if (m < M && v != 0) atomicAdd(&rank[m * k + (e % k)], v);
  }
  if (redecided) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) redo += __shfl_xor(redo, o);
    if (lane == 0 && redo) atomicAdd(redecided, (unsigned long long)redo);
  }
}

}  // namespace
}  // namespace g2v

using namespace g2v;

extern "C" int g2v_neighbor_ranks_ok(int64_t N, int64_t M, int d, int k) { return nr_shape_ok(N, M, d, k) ? 1 : 0; }

extern "C" size_t g2v_neighbor_ranks_workspace(int64_t N, int64_t M, int d, int k) {
  if (!nr_shape_ok(N, M, d, k)) return 0;
  return nr_norm_offset(N) + km_align((size_t)M * sizeof(double));
}

extern "C" int g2v_neighbor_ranks(const float* X, int64_t ldx, int64_t N, const float* Z, int64_t ldz, int64_t M, int d,
                                  const int64_t* self, const int32_t* idx, int k, int32_t* rank, int64_t* redecided, void* workspace,
                                  size_t workspace_bytes, g2v_stream_t stream) {
  G2V_REQUIRE(X && Z && idx && rank && workspace, "null pointer");
  if (!nr_shape_ok(N, M, d, k) || (ldx & 3) || (ldz & 3) || ldx < d || ldz < d) {
    set_error("g2v_neighbor_ranks: needs 1 <= d <= %d, ldx and ldz multiples of 4 and >= d, 1 <= k <= %d, 1 <= N < 2^24, "
              "1 <= M < 2^31 (N = %lld, M = %lld, d = %d, k = %d, ldx = %lld, ldz = %lld)", NR_MAX_D, NR_MAX_K, (long long)N,
              (long long)M, d, k, (long long)ldx, (long long)ldz);
    return G2V_ERR_UNSUPPORTED;
  }
  G2V_REQUIRE(((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Z) | reinterpret_cast<uintptr_t>(workspace)) & 15) == 0,
              "X, Z and workspace must be 16-byte aligned");
  G2V_REQUIRE((reinterpret_cast<uintptr_t>(redecided) & 7) == 0 && (reinterpret_cast<uintptr_t>(self) & 7) == 0,
              "self and redecided must be 8-byte aligned");
  if (workspace_bytes < g2v_neighbor_ranks_workspace(N, M, d, k)) {
    set_error("g2v_neighbor_ranks: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  if (!g2v_internal_lds_reserve((const void*)nr_rank_kernel, nr_lds_bytes(k))) {
    set_error("g2v_neighbor_ranks: cannot reserve LDS");
    return G2V_ERR_LAUNCH;
  }
  hipStream_t st = (hipStream_t)stream;
  double* nx = (double*)workspace;
  double* nz = (double*)((char*)workspace + nr_norm_offset(N));
  // few row blocks: the column tiles are split over workgroups, about two per CU in all
  const int64_t blocks = (M + PD_TILE - 1) / PD_TILE, tiles = (N + PD_TILE - 1) / PD_TILE;
  const int cus = g2v_internal_device_cus();
  const int64_t want = 2 * (int64_t)(cus > 0 ? cus : 256);
  int64_t slices = (want + blocks - 1) / blocks;
  slices = slices < 1 ? 1 : slices;
  slices = slices > tiles ? tiles : slices;
  slices = slices > NR_MAX_SLICES ? NR_MAX_SLICES : slices;
  (void)hipMemsetAsync(rank, 0, (size_t)M * k * sizeof(int32_t), st);
  if (redecided) (void)hipMemsetAsync(redecided, 0, sizeof(int64_t), st);
  hipLaunchKernelGGL(pd_norm_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, X, ldx, N, d, nx);
  hipLaunchKernelGGL(pd_norm_kernel, dim3(cdiv(M, 256)), dim3(256), 0, st, Z, ldz, M, d, nz);
  hipLaunchKernelGGL(nr_rank_kernel, dim3((unsigned)blocks, (unsigned)slices), dim3(256), nr_lds_bytes(k), st, X, ldx, (int)N, Z, ldz,
                     M, d, self, idx, k, (const double*)nx, (const double*)nz, rank, (unsigned long long*)redecided);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
