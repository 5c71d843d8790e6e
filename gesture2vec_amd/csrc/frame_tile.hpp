// frame_tile.hpp -- what the one-workgroup kernels of the frame-level models of Part a share (vq_frame.hip: VQ_Frame, vae_frame.hip:
// VAE_Network): the LDS row stride, the 16x16 output tile as one chain of fp32 MFMAs, the two four-lane sums, the guard rule of a
// tile that hangs over its matrix (tile_guarded, tile_each) with the two stage shapes built on it (rows_tile, wgrad_tile), the
// dropped-out input, the reconstruction epilogue and the 16-lane argmin.
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

// ---- the guard rule, once: a tile at (r0, c0) of an R x Cn result reads 0 for the rows >= R and the columns >= Cn and writes nothing
// there.  Rows, columns and k are ints: every admitted shape keeps them (and the LDS offsets made of them) far below 2^31.

// tile_mma on operands that take matrix coordinates: a_at(row, k) for row < R, b_at(k, col) for col < Cn
template <class FA, class FB>
__device__ __forceinline__ f32x4 tile_guarded(int Kd, int lane, int r0, int R, int c0, int Cn, FA a_at, FB b_at, Side& s) {
  return tile_mma(
      Kd, lane, [&](int i, int k) { return r0 + i < R ? a_at(r0 + i, k) : 0.f; },
      [&](int k, int jj) { return c0 + jj < Cn ? b_at(k, c0 + jj) : 0.f; }, s);
}
// f(r, row, col) for the elements acc[r], r = 0 .. 3, of the tile that this lane holds and that lie inside the result
template <class F>
__device__ __forceinline__ void tile_each(int lane, int r0, int R, int c0, int Cn, F f) {
  const int col = c0 + (lane & 15), q = lane >> 4;
  if (col < Cn) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + 4 * q + r;
      if (row < R) f(r, row, col);
    }
  }
}
// A row product: epi(row, col, sum_k a_at(row, k) b_at(k, col)) over one tile
template <class FA, class FB, class FE>
__device__ __forceinline__ void rows_tile(int Kd, int lane, int r0, int R, int c0, int Cn, FA a_at, FB b_at, FE epi) {
  Side s;
  const f32x4 acc = tile_guarded(Kd, lane, r0, R, c0, Cn, a_at, b_at, s);
  tile_each(lane, r0, R, c0, Cn, [&](int r, int row, int col) { epi(row, col, acc[r]); });
}
// A weight gradient: gw[o][c] = sum_b s_at(b, o) t_at(b, c) over one tile of the row-major O x Cn array gw; the tiles with c0 == 0
// also write gb[o] = sum_b s_at(b, o).  gw is indexed in 64 bits at every site: O Cn is D L, which no admission rule bounds by 2^31
// (only B D is), and the one multiply per stored element costs nothing next to the chain.
template <class FS, class FT>
__device__ __forceinline__ void wgrad_tile(int B, int lane, int o0, int O, int c0, int Cn, FS s_at, FT t_at, float* gw, float* gb) {
  Side s;
  const f32x4 acc = tile_guarded(B, lane, o0, O, c0, Cn, [&](int o, int b) { return s_at(b, o); }, t_at, s);
  const float colsum = q_sum(s.sa);
  const int o = o0 + (lane & 15);
  if (c0 == 0 && (lane >> 4) == 0 && o < O) gb[o] = colsum;
  tile_each(lane, o0, O, c0, Cn, [&](int r, int oo, int c) { gw[(int64_t)oo * Cn + c] = acc[r]; });
}

// x[b][d] after Dropout with a given keep mask (nullptr: no dropout); b and d inside the (., D) array
__device__ __forceinline__ float dropped_at(const float* x, const uint8_t* keep, float scale, int D, int b, int d) {
  const int64_t e = (int64_t)b * D + d;
  const float v = x[e];
  return (keep == nullptr) ? v : (keep[e] ? v * scale : 0.f);
}
// The decoder's epilogue at element e of the (B,D) arrays: out = v + bias, g = gsc (out - t), rec += (out - t)^2
__device__ __forceinline__ void recon_epilogue(float v, float bias, int64_t e, const float* t, float gsc, float* out, float* g,
                                               float& rec) {
  const float ov = v + bias;
  if (out) out[e] = ov;
  const float df = ov - t[e];
  rec = fmaf(df, df, rec);
  g[e] = gsc * df;
}
// argmin_merge (common.hpp) over the sixteen lanes that share lane >> 4, in every one of them
__device__ __forceinline__ void argmin_merge16(float& d, int& k) {
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) {
    const float d2 = __shfl_xor(d, m);
    const int k2 = __shfl_xor(k, m);
    argmin_merge(d, k, d2, k2);
  }
}

}  // namespace g2v
