// frame_tile.hpp -- what the one-workgroup kernels of the frame-level models of Part a share (vq_frame.hip: VQ_Frame, vae_frame.hip:
// VAE_Network): the LDS row stride, the 16x16 output tile as one chain of fp32 MFMAs, and the two four-lane sums.
#pragma once
#include "common.hpp"

namespace g2v {

// row stride of an LDS array of n-float rows: n rounded up to 4 mod 8, so that 16 rows x 4 consecutive k of an MFMA operand hit 64
// different banks
__host__ __device__ inline int frame_ld(int n) { return ((n + 3) / 8) * 8 + 4; }

struct Side {
  float sa, saa, sbb;      // this lane's sums of a, a^2, b^2 over its k
};

// One 16x16 output tile: acc[r] = sum_k A[i = 4 q + r][k] B[k][j = lane & 15], k ascending in steps of 4.  a_at(i, k) and b_at(k, j)
// return 0 outside their matrices.
template <class FA, class FB>
__device__ __forceinline__ f32x4 tile_mma(int Kd, int lane, FA a_at, FB b_at, Side& s) {
  const int i = lane & 15, q = lane >> 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  s.sa = s.saa = s.sbb = 0.f;
  // eight k-steps' operands are fetched before the first of their MFMAs: the fetches are independent, so a wave pays one
  // memory latency per eight steps (an operand read from global memory costs an L2 round trip), and the sums keep their order
  constexpr int U = 8;
  for (int k0 = 0; k0 < Kd; k0 += 4 * U) {
    float a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + 4 * u + q;
      a[u] = k < Kd ? a_at(i, k) : 0.f;
      b[u] = k < Kd ? b_at(k, i) : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k0 + 4 * u < Kd) {      // (wave-uniform)
        s.sa += a[u];
        s.saa = fmaf(a[u], a[u], s.saa);
        s.sbb = fmaf(b[u], b[u], s.sbb);
        acc = mfma16(a[u], b[u], acc);
      }
    }
  }
  return acc;
}
// sum over the four lanes (q = 0 .. 3) that share lane & 15, in every lane
__device__ __forceinline__ float q_sum(float v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}
// sum over the four neighbouring lanes tid & 3 = 0 .. 3, in every lane
__device__ __forceinline__ float quad_sum(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  return v;
}

}  // namespace g2v
