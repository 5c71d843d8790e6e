// vae_noise.hpp -- the normal deviates of the variational blocks and the finish of their KL mean, shared by vae_latent.hip (the
// chunk level) and vae_frame.hip (the frame level): the same (seed, counter) gives the same eps in every kernel that draws it.
#pragma once
#include "common.hpp"

namespace g2v {

// four normal deviates from one Philox block: two Box-Muller pairs; u in (0, 1] for the logarithm, 24-bit uniforms.  Block g of the
// stream (seed, off) is elements 4g .. 4g+3 of the row-major noise array -- g2v_keep_mask's mapping.
__device__ __forceinline__ void philox_normal4(int64_t g, uint64_t off, uint64_t seed, float (&out)[4]) {
  uint32_t c[4];
  philox4x32(g, off, seed, c);
  constexpr float S = 1.0f / 16777216.0f;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float u1 = ((float)(c[2 * p] >> 8) + 1.0f) * S;
    const float u2 = (float)(c[2 * p + 1] >> 8) * S;
    const float r = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(2.0f * u2, &sn, &cs);
    out[2 * p] = r * cs;
    out[2 * p + 1] = r * sn;
  }
}

namespace {

// kl[0] = scale * sum(partials): one workgroup, thread t sums partials t, t + 256, ... in order, then a fixed tree.
__global__ __launch_bounds__(256) void vae_kl_finish_kernel(const float* __restrict__ partial, int nblk, float scale,
                                                            float* __restrict__ kl) {
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float s = 0.f;
  for (int j = tid; j < nblk; j += 256) s += partial[j];
  s = wave_sum(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (tid == 0) kl[0] = ((red[0] + red[1]) + (red[2] + red[3])) * scale;
}

}  // namespace
}  // namespace g2v
