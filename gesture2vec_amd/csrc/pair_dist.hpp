// pair_dist.hpp -- the one home of pairwise squared Euclidean distances between fp32 rows (tsne.hip, tsne_place.hip, silhouette.hip,
// kmeans.hip, dbscan.hip, ward.hip).  What g2v_tsne_affinities gives for two rows and what g2v_tsne_place_neighbors gives for them are the same bits
// because both call the code below.
//   pd_ld4          columns k .. k + 3 of a row of d columns, zero from column d on
//   pd_pair_sq      sum (a - b)^2 in float64 from the two rows, by a whole wave
//   pd_near_pairs   the wave-uniform loop over the NEAR pairs of a fragment: d^2 < PD_NEAR (n_i + n_j), where the Gram form
//                   d^2 = |x_i|^2 + |x_j|^2 - 2 x_i.x_j has lost >= 3 bits and the pair is evaluated again (pd_pair_sq)
//   pd_norm_kernel  |row|^2 in float64, one fma chain per row
//   pd_row_norms    a lane's four row norms for pd_tile
//   pd_stage        one k-chunk of both row sets of a tile into LDS
//   pd_tile         one 64 x 64 tile of d^2 between two row sets on the exact-fp32 MFMA, by a workgroup of 4 waves
//   pd_tile_f64     the same tile with the Gram products on the float64 MFMA and d^2 left in float64 (ward.hip)
// Included inside one translation unit each.
#pragma once
#include "common.hpp"
#include "km_sort.hpp"

namespace g2v {
namespace {

constexpr float PD_NEAR = 0.125f;
constexpr int PD_TILE = 64;
constexpr int PD_KC = 32;                   // columns per staged chunk = length of an fp32 chain
constexpr int PD_LD = PD_KC + 4;            // LDS row stride of a staged chunk (an odd number of 16-byte slots)

// columns k .. k + 3 of a row of d columns (k % 4 == 0, the row 16-byte aligned), zero from column d on and where !ok
__device__ __forceinline__ float4 pd_ld4(const float* __restrict__ row, int k, int d, bool ok) {
  // (uniform) rows of whole vectors: one load from a clamped address and a select, no divergent branch in a staging loop
  if ((d & 3) == 0) return ld4_or_zero(row + (ok && k < d ? k : 0), ok && k < d);
  if (ok && k + 3 < d) return *reinterpret_cast<const float4*>(row + k);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ok) {
    if (k < d) v.x = row[k];
    if (k + 1 < d) v.y = row[k + 1];
    if (k + 2 < d) v.z = row[k + 2];
  }
  return v;
}

// |a - b|^2 in float64 over d columns (64 lanes over the columns, four to a lane, fixed xor tree; rows 16-byte aligned); every lane
// returns the same bits, and (a, b) gives the bits of (b, a): a difference and its negative have the same square.  The d % 4 columns
// behind the last whole vector end the chain of the lane that would have held that vector.
__device__ __forceinline__ double pd_pair_sq(const float* __restrict__ a, const float* __restrict__ b, int d, int lane) {
  const float4* pa = reinterpret_cast<const float4*>(a);
  const float4* pb = reinterpret_cast<const float4*>(b);
  double acc = 0.0;
  for (int v = lane; v < (d >> 2); v += 64) {
    const float4 x = pa[v], y = pb[v];
    const double d0 = (double)x.x - (double)y.x, d1 = (double)x.y - (double)y.y, d2 = (double)x.z - (double)y.z,
                 d3 = (double)x.w - (double)y.w;
    acc = fma(d0, d0, acc);
    acc = fma(d1, d1, acc);
    acc = fma(d2, d2, acc);
    acc = fma(d3, d3, acc);
  }
  if (lane == ((d >> 2) & 63)) {
    for (int k = d & ~3; k < d; ++k) {
      const double dk = (double)a[k] - (double)b[k];
      acc = fma(dk, dk, acc);
    }
  }
  return km_wave_sum(acc);
}

// Bit r of nm: register r of this lane holds a near pair.  (wave-uniform) one lane's near pairs at a time, by the whole wave:
// eval(L, r) evaluates register r of lane L with every lane taking part, and lane L keeps the value.
template <class T, class Eval>
__device__ __forceinline__ void pd_near_pairs(unsigned nm, int lane, T (&dd)[4], Eval eval) {
  unsigned long long pend = __ballot(nm != 0);
  while (pend) {
    const int L = __ffsll((long long)pend) - 1;
    pend &= pend - 1;
    const unsigned m4 = (unsigned)__shfl((int)nm, L);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if ((m4 >> r) & 1u) {
        const T v = eval(L, r);
        if (lane == L) dd[r] = v;
      }
    }
  }
}

// one thread per row (a zero-padded row gives the bits of the unpadded one: fma(0, 0, acc) == acc)
__global__ __launch_bounds__(256) void pd_norm_kernel(const float* __restrict__ x, int64_t ld, int64_t n, int d,
                                                     double* __restrict__ norm) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const float* p = x + r * ld;
  double acc = 0.0;
  for (int k = 0; k < d; ++k) acc = fma((double)p[k], (double)p[k], acc);
  norm[r] = acc;
}

// the norms of this lane's four rows of A in pd_tile's epilogue, rows a0 + 16 wave + 4 q + r (0 past the end): a kernel that walks
// many tiles of B against the same 64 rows of A loads them once
__device__ __forceinline__ void pd_row_norms(const double* __restrict__ norm_a, int64_t na, int64_t a0, double (&nr)[4]) {
  const int64_t row0 = a0 + 16 * (threadIdx.x >> 6) + 4 * ((threadIdx.x & 63) >> 4);
#pragma unroll
  for (int r = 0; r < 4; ++r) nr[r] = row0 + r < na ? norm_a[row0 + r] : 0.0;
}

// Columns k0 .. k0 + PD_KC - 1 of rows a0 .. a0 + 63 of A into sa and of rows b0 .. b0 + 63 of B into sb, masked at the load (zero
// past the end of a set or of a row), by a workgroup of 256 threads: thread t stages rows t / 8 and t / 8 + 32, columns 4 (t % 8) ..
__device__ __forceinline__ void pd_stage(const float* __restrict__ A, int64_t lda, int64_t na, int64_t a0, const float* __restrict__ B,
                                         int64_t ldb, int nb, int b0, int d, int k0, float* __restrict__ sa, float* __restrict__ sb) {
  const int lr = threadIdx.x >> 3, lc = (threadIdx.x & 7) * 4;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int r = lr + 32 * h, k = k0 + lc;
    const int64_t ra = a0 + r;
    const int rb = b0 + r;
    *reinterpret_cast<float4*>(sa + r * PD_LD + lc) = pd_ld4(A + (ra < na ? ra : 0) * lda, k, d, ra < na);
    *reinterpret_cast<float4*>(sb + r * PD_LD + lc) = pd_ld4(B + (int64_t)(rb < nb ? rb : 0) * ldb, k, d, rb < nb);
  }
}

// The tile of d^2 between rows a0 .. a0 + 63 of A (na rows of d columns, stride lda, this lane's norms nr from pd_row_norms) and rows
// b0 .. b0 + 63 of B, by a workgroup of 256 threads; sa, sb: PD_TILE * PD_LD floats of LDS each, 16-byte aligned.  Both row sets go
// through LDS in k-chunks of PD_KC columns, masked at the load (no padded copy is needed); wave w owns tile rows 16 w .. 16 w + 15
// as the A operand of v_mfma_f32_16x16x4_f32 and the four 16-row groups of B as the B operand, so that lane (i, q) ends with
// G[row 4 q + r][col 16 j + i] in register r of accumulator j.  The fp32 chains are PD_KC columns long: after every chunk the
// accumulators are added into float64 ones and cleared, so G carries sqrt(d / 32) chunk errors of ~3e-7 |partial sum over 32
// columns| (2e-5 at d = 400 for rows of unit entries) instead of one chain through all of d.  d^2 = n_i + n_j - 2 G in float64,
// rounded to fp32 once (sklearn rounds its float64 distances to fp32 too); a near pair is evaluated again from differences, so a
// bitwise equal pair has d^2 = 0 exactly.  With same (A and B are one set) the diagonal is 0 by rule, and tile (a0, b0) holds the
// transpose of tile (b0, a0) bit for bit: the same products in the same order.
// out(row, col, dd): dd[r] = d^2(A row + r, B col), r < 4; inf where either is past the end of its set.  The first barrier of the
// call orders whatever the workgroup did before against the staging; nothing follows the last out().
template <class Out>
__device__ __forceinline__ void pd_tile(const float* __restrict__ A, int64_t lda, int64_t na, int64_t a0,
                                        const double (&nr)[4], const float* __restrict__ B, int64_t ldb, int nb, int b0,
                                        const double* __restrict__ norm_b, int d, bool same, float* __restrict__ sa,
                                        float* __restrict__ sb, Out out) {
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int E4 = (d + 3) & ~3;

  f32x4 acc[4];
  double accd[4][4];                                          // G, folded in float64 after every chunk
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) accd[j][r] = 0.0;
  }
  for (int k0 = 0; k0 < E4; k0 += PD_KC) {
    __syncthreads();                                          // the previous chunk has been multiplied
    pd_stage(A, lda, na, a0, B, ldb, nb, b0, d, k0, sa, sb);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (k0 + 16 * ks < E4) {
        const float4 a = *reinterpret_cast<const float4*>(sa + (16 * wave + i) * PD_LD + 16 * ks + 4 * q);
        float4 b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const float4*>(sb + (16 * j + i) * PD_LD + 16 * ks + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = mfma16(a.x, b[j].x, acc[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = mfma16(a.y, b[j].y, acc[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = mfma16(a.z, b[j].z, acc[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = mfma16(a.w, b[j].w, acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) accd[j][r] += (double)acc[j][r];
      acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  }

  const int64_t wrow = a0 + 16 * wave;                        // lane (i, q), register r of acc[j]: G[wrow + 4 q + r][b0 + 16 j + i]
  const int64_t row0 = wrow + 4 * q;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = b0 + 16 * j + i;
    const double nc = col < nb ? norm_b[col] : 0.0;
    float dd[4];
    unsigned nm = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double sum = nr[r] + nc;
      const double d2 = fma(-2.0, accd[j][r], sum);
      const bool in = row0 + r < na && col < nb, valid = in && !(same && row0 + r == col);
      const bool near = valid && d2 < (double)PD_NEAR * sum;
      dd[r] = in ? ((valid && !near) ? (float)d2 : 0.f) : __builtin_inff();
      nm |= near ? (1u << r) : 0u;
    }
    pd_near_pairs(nm, lane, dd, [&](int L, int r) {
      return (float)pd_pair_sq(A + (wrow + 4 * (L >> 4) + r) * lda, B + (int64_t)(b0 + 16 * j + (L & 15)) * ldb, d, lane);
    });
    out(row0, col, dd);
  }
}

// ---- the float64 tile (ward.hip) ------------------------------------------------------------------------------------------------------
// v_mfma_f64_16x16x4_f64: lane l supplies a = A[i = l & 15][k = l >> 4] and b = B[k = l >> 4][j = l & 15] as the fp32 form does, and
// receives D[i = (l >> 4) + 4 r][j = l & 15] in element r of the accumulator: NOT the fp32 form's row 4 (l >> 4) + r.
typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f64x4 mfma16_f64(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// the norms of this lane's four rows of A in pd_tile_f64's epilogue, rows a0 + 16 wave + q + 4 r (0 past the end)
__device__ __forceinline__ void pd_row_norms_f64(const double* __restrict__ norm_a, int64_t na, int64_t a0, double (&nr)[4]) {
  const int64_t row0 = a0 + 16 * (threadIdx.x >> 6) + ((threadIdx.x & 63) >> 4);
#pragma unroll
  for (int r = 0; r < 4; ++r) nr[r] = row0 + 4 * r < na ? norm_a[row0 + 4 * r] : 0.0;
}

// pd_tile with the Gram products in float64: the fp32 rows are staged as pd_tile stages them and widened at the fragment read (exact),
// every product and sum of G is a float64 fma on the MFMA, one chain through all of d, and d^2 = n_i + n_j - 2 G is not rounded to
// fp32: |d^2 - exact| <= ~d 2^-53 (n_i + n_j), so a pair that is not near carries 8 d 2^-53 relative.  A near pair is evaluated again
// from differences (pd_pair_sq) as in pd_tile.  Lane (i, q) ends with G[row q + 4 r][col 16 j + i] in register r of accumulator j:
// out(row, col, dd): dd[r] = d^2(A row + 4 r, B col), r < 4; 0 on the diagonal with same; inf where either is past the end of its set.
template <class Out>
__device__ __forceinline__ void pd_tile_f64(const float* __restrict__ A, int64_t lda, int64_t na, int64_t a0,
                                            const double (&nr)[4], const float* __restrict__ B, int64_t ldb, int nb, int b0,
                                            const double* __restrict__ norm_b, int d, bool same, float* __restrict__ sa,
                                            float* __restrict__ sb, Out out) {
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int E4 = (d + 3) & ~3;

  f64x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = (f64x4){0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < E4; k0 += PD_KC) {
    __syncthreads();                                          // the previous chunk has been multiplied
    pd_stage(A, lda, na, a0, B, ldb, nb, b0, d, k0, sa, sb);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (k0 + 16 * ks < E4) {
        const float4 a = *reinterpret_cast<const float4*>(sa + (16 * wave + i) * PD_LD + 16 * ks + 4 * q);
        float4 b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const float4*>(sb + (16 * j + i) * PD_LD + 16 * ks + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = mfma16_f64((double)a.x, (double)b[j].x, acc[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = mfma16_f64((double)a.y, (double)b[j].y, acc[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = mfma16_f64((double)a.z, (double)b[j].z, acc[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = mfma16_f64((double)a.w, (double)b[j].w, acc[j]);
      }
    }
  }

  const int64_t wrow = a0 + 16 * wave;                        // lane (i, q), register r of acc[j]: G[wrow + q + 4 r][b0 + 16 j + i]
  const int64_t row0 = wrow + q;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = b0 + 16 * j + i;
    const double nc = col < nb ? norm_b[col] : 0.0;
    double dd[4];
    unsigned nm = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double sum = nr[r] + nc;
      const double d2 = fma(-2.0, acc[j][r], sum);
      const bool in = row0 + 4 * r < na && col < nb, valid = in && !(same && row0 + 4 * r == col);
      const bool near = valid && d2 < (double)PD_NEAR * sum;
      dd[r] = in ? ((valid && !near) ? d2 : 0.0) : (double)__builtin_inff();
      nm |= near ? (1u << r) : 0u;
    }
    pd_near_pairs(nm, lane, dd, [&](int L, int r) {
      return pd_pair_sq(A + (wrow + (L >> 4) + 4 * r) * lda, B + (int64_t)(b0 + 16 * j + (L & 15)) * ldb, d, lane);
    });
    out(row0, col, dd);
  }
}

}  // namespace
}  // namespace g2v
