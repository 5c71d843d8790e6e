// dtw_tile.hpp -- what dtw.hip and softdtw.hip share: the limits, the grouping rule, the cost phase of a tile and the argmin over
// the centres.  One wave (a workgroup of 64 threads) owns one series and 64 / P centres, P the power of two >= max(S, 16): lane l
// holds column j = l % P of centre g = l / P.  dtw_cost_tile fills tile[i][l] (T x 64 float64 in LDS) with sum_f (a_if - b_jf)^2:
// the columns are walked in chunks of DTW_FC, the lane keeps its DTW_FC centre values in registers, the wave's T x DTW_FC slice of
// the series stands in LDS as fp32 and is read as a broadcast, two rows i at a time, each term fused into the running sum (one
// rounding per term, f ascending).  Both recursions read their costs from this one piece of code, so they see the same bits.
#pragma once
#include "common.hpp"

namespace g2v {
namespace {

constexpr int DTW_MAX_LEN = 64;
constexpr int DTW_MAX_F = 512;
constexpr int DTW_FC = 32;                  // columns per chunk: the lane's registers, the series slice in LDS

inline bool dtw_shape_ok(int64_t N, int64_t M, int T, int S, int F) {
  return N >= 1 && M >= 1 && N <= 0x7fffffff && M <= 0x7fffffff && T >= 1 && S >= 1 && T <= DTW_MAX_LEN && S <= DTW_MAX_LEN && F >= 1 &&
         F <= DTW_MAX_F;
}
inline int dtw_group_width(int S) { return S <= 16 ? 16 : (S <= 32 ? 32 : 64); }
// the cost tile followed by the series slice
inline size_t dtw_lds_bytes(int T) { return (size_t)T * 64 * sizeof(double) + (size_t)T * DTW_FC * sizeof(float); }

// tile[i * 64 + lane] = cost of row i of the series `a` (T x F fp32) against the centre column this lane owns (`b`: F float64, read
// only when `active`).  as: the T x DTW_FC fp32 slice.  Every lane of the wave must call it; it ends with a barrier.
__device__ __forceinline__ void dtw_cost_tile(const float* __restrict__ a, const double* __restrict__ b, bool active, int T, int F,
                                              double* tile, float* as) {
  const int lane = threadIdx.x;
  for (int i = 0; i < T; ++i) tile[i * 64 + lane] = 0.0;
  for (int f0 = 0; f0 < F; f0 += DTW_FC) {
    __syncthreads();                                         // (the slice of the chunk before is read no more)
    for (int e = lane; e < T * DTW_FC; e += 64) {
      const int i = e / DTW_FC, f = f0 + (e % DTW_FC);
      as[e] = f < F ? a[(size_t)i * F + f] : 0.f;
    }
    double bv[DTW_FC];
#pragma unroll
    for (int f = 0; f < DTW_FC; ++f) bv[f] = (active && f0 + f < F) ? b[f0 + f] : 0.0;     // past F both sides are 0: the term is +0
    __syncthreads();
    for (int i = 0; i < T; i += 2) {
      const int i1 = min(i + 1, T - 1);
      double s0 = tile[i * 64 + lane], s1 = tile[i1 * 64 + lane];
      const float4* r0 = reinterpret_cast<const float4*>(as + i * DTW_FC);
      const float4* r1 = reinterpret_cast<const float4*>(as + i1 * DTW_FC);
#pragma unroll
      for (int q = 0; q < DTW_FC / 4; ++q) {
        const float4 u = r0[q], v = r1[q];
        const double u4[4] = {u.x, u.y, u.z, u.w}, v4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const double d0 = u4[e] - bv[4 * q + e], d1 = v4[e] - bv[4 * q + e];
          s0 = fma(d0, d0, s0);
          s1 = fma(d1, d1, s1);
        }
      }
      tile[i * 64 + lane] = s0;
      if (i + 1 < T) tile[i1 * 64 + lane] = s1;
    }
  }
  __syncthreads();
}

// one wave per n over d2 (N, M): out[n][:] = d2 or sqrt(d2), labels[n], best[n]; (value, index) lexicographic, lowest index
__global__ __launch_bounds__(256) void dtw_argmin_kernel(const double* __restrict__ d2, int64_t N, int64_t M, int squared,
                                                        double* __restrict__ out, int64_t* __restrict__ labels,
                                                        double* __restrict__ best) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;                                        // (wave-uniform)
  const double* row = d2 + n * M;
  double bv = (double)__builtin_inff();
  int64_t bm = -1;
  for (int64_t m = lane; m < M; m += 64) {
    const double v = row[m];
    if (out) out[n * M + m] = squared ? v : sqrt(v);
    if (bm < 0 || v < bv) {
      bv = v;
      bm = m;
    }
  }
  if (!labels) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {                         // (value, index) in lexicographic order: ties to the lowest index
    const double ob = __shfl_xor(bv, o);
    const int64_t om = __shfl_xor(bm, o);
    if (om >= 0 && (bm < 0 || ob < bv || (ob == bv && om < bm))) {
      bv = ob;
      bm = om;
    }
  }
  if (lane == 0) {
    labels[n] = bm;
    best[n] = bv;
  }
}

}  // namespace
}  // namespace g2v
