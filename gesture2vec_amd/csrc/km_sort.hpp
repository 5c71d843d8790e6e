// km_sort.hpp -- the stable counting sort of row ids by label (an inverted index: atomic-free scatter-add, cdna_hip_programming.md
// Appendix B) that kmeans.hip and silhouette.hip share, with the small deterministic reductions both use.  Included inside one
// translation unit each; the kernels are described at the head of kmeans.hip.
#pragma once
#include "common.hpp"

namespace g2v {
namespace {

constexpr int KM_SORT_ROWS = 2048;          // rows per workgroup of the counting sort
constexpr int KM_LDS_BINS = 8192;           // clusters whose counters fit in LDS; more: the block's row of hist in global memory

enum { ST_DONE = 0, ST_ITER, ST_CHANGED, ST_SHIFT, ST_INERTIA, ST_RELOC, ST_ACTIVE, ST_TOL };
enum { HD_CHANGED = 0, HD_EMPTY, HD_VALID, HD_CHUNKS, HD_RELOC, HD_WORDS = 8 };

inline size_t km_align(size_t v) { return (v + 255) & ~(size_t)255; }

__device__ __forceinline__ bool km_gated(const double* state) { return state && state[ST_DONE] != 0.0; }

__device__ __forceinline__ double km_wave_sum(double v) {      // fixed xor tree: every lane ends with the same bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// sum of v over the workgroup in a fixed tree (blockDim.x a power of two <= 1024); valid in thread 0
__device__ __forceinline__ double km_block_sum(double v, double* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  return sh[0];
}

__global__ __launch_bounds__(256) void km_hist_kernel(const int64_t* __restrict__ labels, const int64_t* __restrict__ prev, int64_t N,
                                                     int K, int* __restrict__ hist, unsigned long long* __restrict__ hdr, int use_lds,
                                                     const double* __restrict__ state) {
  __shared__ int bins[KM_LDS_BINS];
  if (km_gated(state)) return;
  const int tid = threadIdx.x;
  int* row = hist + (size_t)blockIdx.x * K;                 // (the global path's row was zeroed by the caller)
  if (use_lds) {
    for (int k = tid; k < K; k += 256) bins[k] = 0;
    __syncthreads();
  }
  const int64_t r0 = (int64_t)blockIdx.x * KM_SORT_ROWS;
  int changed = 0;
  for (int i = tid; i < KM_SORT_ROWS; i += 256) {
    const int64_t n = r0 + i;
    if (n >= N) break;
    const int64_t v = labels[n];
    if (prev && prev[n] != v) ++changed;
    if (v >= 0 && v < K) atomicAdd(use_lds ? &bins[v] : &row[v], 1);
  }
  if (changed) atomicAdd(&hdr[HD_CHANGED], (unsigned long long)changed);
  if (use_lds) {
    __syncthreads();
    for (int k = tid; k < K; k += 256) row[k] = bins[k];
  }
}

// hist[b][k] -> the number of rows of cluster k in the blocks before b; counts[k].  One workgroup per 64 clusters, 16 threads per
// cluster, each owning a run of consecutive blocks: sum the run, scan the 16 sums, write the run's prefixes.
__global__ __launch_bounds__(1024) void km_prefix_kernel(int* __restrict__ hist, int nb, int K, int64_t* __restrict__ counts,
                                                        const double* __restrict__ state) {
  __shared__ int segsum[16][64];
  if (km_gated(state)) return;
  const int kk = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + kk;
  const int per = (nb + 15) / 16, b0 = min(nb, seg * per), b1 = min(nb, b0 + per);
  int* p = hist + (k < K ? k : 0);
  int tot = 0;
  if (k < K) {
    int b = b0;
    for (; b + 8 <= b1; b += 8) {
      int t[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) t[j] = p[(size_t)(b + j) * K];
#pragma unroll
      for (int j = 0; j < 8; ++j) tot += t[j];
    }
    for (; b < b1; ++b) tot += p[(size_t)b * K];
  }
  segsum[seg][kk] = tot;
  __syncthreads();
  if (k >= K) return;
  int run = 0;
  for (int s2 = 0; s2 < seg; ++s2) run += segsum[s2][kk];
  int b = b0;
  for (; b + 8 <= b1; b += 8) {
    int t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = p[(size_t)(b + j) * K];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      p[(size_t)(b + j) * K] = run;
      run += t[j];
    }
  }
  for (; b < b1; ++b) {
    const int t = p[(size_t)b * K];
    p[(size_t)b * K] = run;
    run += t;
  }
  if (seg == 15) counts[k] = run;
}

// (chunk: rows of one cluster per entry of ch_first)
__global__ __launch_bounds__(1024) void km_scan_kernel(int K, int chunk, const int64_t* __restrict__ counts, int* __restrict__ cl_start,
                                                      int* __restrict__ ch_first, unsigned long long* __restrict__ hdr,
                                                      const double* __restrict__ state) {
  __shared__ int sa[1024], sb[1024], se[1024];
  __shared__ int carry[3];
  if (km_gated(state)) return;
  const int tid = threadIdx.x;
  if (tid < 3) carry[tid] = 0;
  __syncthreads();
  for (int base = 0; base < K; base += 1024) {
    const int k = base + tid;
    const int cnt = k < K ? (int)counts[k] : 0;
    const int nch = (cnt + chunk - 1) / chunk;
    sa[tid] = cnt;
    sb[tid] = nch;
    se[tid] = (k < K && cnt == 0) ? 1 : 0;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                    // inclusive scans
      const int a = tid >= o ? sa[tid - o] : 0, b = tid >= o ? sb[tid - o] : 0, e = tid >= o ? se[tid - o] : 0;
      __syncthreads();
      sa[tid] += a;
      sb[tid] += b;
      se[tid] += e;
      __syncthreads();
    }
    if (k < K) {
      cl_start[k] = carry[0] + sa[tid] - cnt;
      ch_first[k] = carry[1] + sb[tid] - nch;
    }
    __syncthreads();
    if (tid == 1023) {
      carry[0] += sa[1023];
      carry[1] += sb[1023];
      carry[2] += se[1023];
    }
    __syncthreads();
  }
  if (tid == 0) {
    cl_start[K] = carry[0];
    ch_first[K] = carry[1];
    hdr[HD_VALID] = (unsigned long long)carry[0];
    hdr[HD_CHUNKS] = (unsigned long long)carry[1];
    hdr[HD_EMPTY] = (unsigned long long)carry[2];
  }
}

// One wave per block of rows, 64 rows at a time in row order.  The lanes that share a label find each other with one ballot per label
// bit; the lowest of them reserves the group's places with one integer atomic on the block's counter of that cluster.
__global__ __launch_bounds__(64) void km_scatter_kernel(const int64_t* __restrict__ labels, int64_t N, int K, int label_bits,
                                                       int* __restrict__ hist, const int* __restrict__ cl_start,
                                                       int* __restrict__ sorted, int use_lds, const double* __restrict__ state) {
  __shared__ int bins[KM_LDS_BINS];
  if (km_gated(state)) return;
  const int lane = threadIdx.x;
  int* row = hist + (size_t)blockIdx.x * K;
  if (use_lds) {
    for (int k = lane; k < K; k += 64) bins[k] = row[k];
    __syncthreads();
  }
  int* ctr = use_lds ? bins : row;
  const int64_t r0 = (int64_t)blockIdx.x * KM_SORT_ROWS;
  int64_t v_next = r0 + lane < N ? labels[r0 + lane] : -1;   // the next 64 labels are loaded before the current ones are consumed
  for (int t = 0; t < KM_SORT_ROWS / 64; ++t) {
    if (r0 + t * 64 >= N) break;
    const int64_t n = r0 + t * 64 + lane;
    const int64_t v = v_next;
    const int64_t nn = n + 64;
    v_next = (t + 1 < KM_SORT_ROWS / 64 && nn < N) ? labels[nn] : -1;
    const int lab = (n < N && v >= 0 && v < K) ? (int)v : -1;
    const bool valid = lab >= 0;
    unsigned long long peers = __ballot(valid);
    for (int bit = 0; bit < label_bits; ++bit) {
      const bool on = valid && ((lab >> bit) & 1);
      const unsigned long long m = __ballot(on);
      peers &= on ? m : ~m;
    }
    if (valid) {                                            // (peers holds this lane: never empty)
      const int leader = __ffsll((long long)peers) - 1;
      int base = 0;
      if (lane == leader) base = atomicAdd(&ctr[lab], __popcll(peers));
      base = __shfl(base, leader);
      sorted[cl_start[lab] + base + __popcll(peers & ((1ull << lane) - 1ull))] = (int)n;
    }
  }
}

}  // namespace
}  // namespace g2v
