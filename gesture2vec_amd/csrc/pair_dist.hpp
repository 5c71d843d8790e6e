// pair_dist.hpp -- what silhouette.hip and tsne.hip share when they form Euclidean distances from Gram tiles on the exact-fp32 MFMA,
// d^2 = |x_i|^2 + |x_j|^2 - 2 x_i.x_j:
//   pd_pair_sq      sum (x_i - x_j)^2 in float64 from the rows (E % 4 == 0, rows 16-byte aligned), by a whole wave: the
//                   re-evaluation of a NEAR pair, d^2 < PD_NEAR (n_i + n_j), where the Gram form has lost >= 3 bits
// Included inside one translation unit each, after km_sort.hpp (km_wave_sum).
#pragma once
#include "common.hpp"
#include "km_sort.hpp"

namespace g2v {
namespace {

constexpr float PD_NEAR = 0.125f;

// |x_ri - x_rj|^2 in float64 (64 lanes over the columns, fixed xor tree); every lane returns the same bits, and (ri, rj) gives the
// bits of (rj, ri)
__device__ __forceinline__ double pd_pair_sq(const float* __restrict__ x, int64_t ld, int E, int ri, int rj, int lane) {
  const float4* pi = reinterpret_cast<const float4*>(x + (int64_t)ri * ld);
  const float4* pj = reinterpret_cast<const float4*>(x + (int64_t)rj * ld);
  double acc = 0.0;
  for (int v = lane; v < (E >> 2); v += 64) {
    const float4 a = pi[v], b = pj[v];
    const double d0 = (double)a.x - (double)b.x, d1 = (double)a.y - (double)b.y, d2 = (double)a.z - (double)b.z,
                 d3 = (double)a.w - (double)b.w;
    acc = fma(d0, d0, acc);
    acc = fma(d1, d1, acc);
    acc = fma(d2, d2, acc);
    acc = fma(d3, d3, acc);
  }
  return km_wave_sum(acc);
}

}  // namespace
}  // namespace g2v
