// ngram.hip -- clipped n-gram match counts between pairs of code-id sequences: the integer half of BLEU over code sequences
// (gesture2vec_amd/metrics.py::code_bleu; the reference scores each test case's code sequence against the ground truth's with
// torchtext's bleu_score, Clustering.py:1560-1609).
//   g2v_ngram_clipped_counts   clipped[b][n-1] = sum over the distinct n-grams g of candidate b of min(count_cand(g), count_ref(g)),
//                              n = 1 .. max_n <= 4, for B independent (candidate, reference) pairs
//
// An n-gram of ids < K <= 65536 is one 64-bit KEY: id[i + j] in bits 16 j .. 16 j + 15, j < n.  The key of the 4-gram at position i,
// cut to its low 16 n bits, is the key of the n-gram at i; position i holds an n-gram iff i + n <= len.  Keys of different orders
// never meet.  Integer arithmetic only; a pair reads nothing but its own two sequences, so its counts do not depend on the batch.
// A pair with a device length outside [0, max_len] or an id outside [0, K) is BAD: -1 in its max_n slots, bad[0] += 1 (one integer
// atomic per bad pair).  A bad length is found before anything is loaded, a bad id is replaced by 0 before it reaches LDS and no key is
// built from the pair at all: out-of-range values are neither an address nor a key.
//
// Two kernels, chosen per call from max_len (the caller's bound; the device lengths are never read back):
//
//   max_len <= 64:  ngram_wave_kernel.  One wavefront per pair, 4 pairs per 256-thread workgroup.  Lane i holds id i of both sequences
//       (0 past the length), builds its 4-gram keys from three lane shifts, and puts them into the wave's 2 x 64 keys of LDS; ONE
//       workgroup barrier (every wave reaches it, also a wave past B or with a bad pair).  Then the rank form
//           clipped_n = #{ i : rank_i < count_ref(g_i) },  rank_i = #{ j < i : g_j == g_i }
//       is evaluated for all four orders in one loop over j < max(len_c, len_r): key j of either sequence is an LDS broadcast read,
//       the four comparisons are masks of one XOR.  The sum over the lanes is __popcll(__ballot(.)).  No sort, no further barrier.
//
//   64 < max_len <= 4096:  ngram_sort_kernel.  One 256-thread workgroup per pair.  The ids go to LDS as 16-bit values (validated on
//       the way).  Per order n: both key arrays are built in LDS, sorted, and every run start of the sorted candidate array finds its
//       run's end by binary search, its run in the sorted reference array by two more, and adds min(c, r); one integer tree per order.
//       The sort is the bitonic network in its all-ascending form (a merge of 2 m keys compares i with its mirror image, then halves);
//       every comparator puts the smaller key at the lower index, so a network for the next power of two works on ANY length when
//       the comparators that reach past the length are skipped (the missing keys behave as +infinity and never move).  No sentinel
//       key exists: at K = 65536 all 2^64 keys are legal 4-grams.  Both arrays go through the same steps (one barrier per step); the
//       network is as large as this pair's longer key array needs, not as max_len.
//       LDS: 2 P keys + 2 (P + 4) ids + 4 partial sums, P = max_len rounded up to a power of two: 82 KB at 4096 (opt-in).
#include "common.hpp"

namespace g2v {
namespace {

constexpr int NG_MAX_LEN = 4096;
constexpr int NG_MAX_K = 65536;
constexpr int NG_MAX_N = 4;
constexpr int NG_WAVE_LEN = 64;             // longest sequence of the one-wave-per-pair kernel
constexpr int NG_WAVE_PAIRS = 4;            // pairs (waves) per workgroup there

__device__ __forceinline__ unsigned long long ng_mask(int n) { return n >= 4 ? ~0ull : (1ull << (16 * n)) - 1ull; }

__device__ __forceinline__ void ng_mark_bad(int64_t* __restrict__ row, int max_n, int64_t* __restrict__ bad, int t) {
  if (t < max_n) row[t] = -1;
  if (t == 0) atomicAdd(reinterpret_cast<unsigned long long*>(bad), 1ull);
}

__global__ __launch_bounds__(64 * NG_WAVE_PAIRS) void ngram_wave_kernel(
    const int64_t* __restrict__ cand, const int64_t* __restrict__ cand_start, const int64_t* __restrict__ cand_len,
    const int64_t* __restrict__ ref, const int64_t* __restrict__ ref_start, const int64_t* __restrict__ ref_len,
    int64_t* __restrict__ clipped, int64_t* __restrict__ bad, int64_t B, int K, int max_n, int max_len) {
  __shared__ unsigned long long keys[NG_WAVE_PAIRS][2][NG_WAVE_LEN];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * NG_WAVE_PAIRS + wave;
  const bool live = b < B;
  int64_t lc = 0, lr = 0;
  if (live) {
    lc = cand_len[b];
    lr = ref_len[b];
  }
  const bool bad_len = lc < 0 || lc > max_len || lr < 0 || lr > max_len;
  int64_t vc = 0, vr = 0;
  if (live && !bad_len) {
    if (lane < lc) vc = cand[cand_start[b] + lane];
    if (lane < lr) vr = ref[ref_start[b] + lane];
  }
  const bool bad_id = vc < 0 || vc >= K || vr < 0 || vr >= K;
  const bool is_bad = bad_len || __ballot(bad_id) != 0ull;
  const unsigned ic = bad_id ? 0u : (unsigned)vc, ir = bad_id ? 0u : (unsigned)vr;
  unsigned long long kc = ic, kr = ir;
#pragma unroll
  for (int j = 1; j < NG_MAX_N; ++j) {                    // (a shift past lane 63 returns the lane's own id: such a position never
    const unsigned sc = __shfl_down(ic, j), sr = __shfl_down(ir, j);      // holds a (j + 1)-gram, its upper key bits are cut off below)
    kc |= (unsigned long long)sc << (16 * j);
    kr |= (unsigned long long)sr << (16 * j);
  }
  keys[wave][0][lane] = kc;
  keys[wave][1][lane] = kr;
  __syncthreads();
  if (!live) return;
  int64_t* row = clipped + b * max_n;
  if (is_bad) {
    ng_mark_bad(row, max_n, bad, lane);
    return;
  }
  const int nc = (int)lc, nr = (int)lr, nj = nc > nr ? nc : nr;
  int rank[NG_MAX_N] = {0, 0, 0, 0}, have[NG_MAX_N] = {0, 0, 0, 0};
  for (int j = 0; j < nj; ++j) {
    const unsigned long long xc = keys[wave][0][j] ^ kc, xr = keys[wave][1][j] ^ kc;
#pragma unroll
    for (int n = 1; n <= NG_MAX_N; ++n) {
      const unsigned long long m = ng_mask(n);
      rank[n - 1] += (j < lane && j + n <= nc && (xc & m) == 0ull) ? 1 : 0;
      have[n - 1] += (j + n <= nr && (xr & m) == 0ull) ? 1 : 0;
    }
  }
  int64_t mine = 0;
#pragma unroll
  for (int n = 1; n <= NG_MAX_N; ++n) {
    const unsigned long long hit = __ballot(lane + n <= nc && rank[n - 1] < have[n - 1]);
    if (lane == n - 1) mine = (int64_t)__popcll(hit);
  }
  if (lane < max_n) row[lane] = mine;
}

__device__ __forceinline__ void ng_cmpx(unsigned long long* __restrict__ a, int i, int l) {
  const unsigned long long x = a[i], y = a[l];
  if (y < x) {
    a[i] = y;
    a[l] = x;
  }
}

// first index in a[0, n) with a[i] >= key (UPPER = false) or a[i] > key (UPPER = true)
template <bool UPPER>
__device__ __forceinline__ int ng_bound(const unsigned long long* __restrict__ a, int lo, int n, unsigned long long key) {
  int hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const unsigned long long v = a[mid];
    if (UPPER ? v <= key : v < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// LDS: keys_c[P] | keys_r[P] | ids_c[P + 4] | ids_r[P + 4] (16-bit) | red[4] (int)
__global__ __launch_bounds__(256) void ngram_sort_kernel(
    const int64_t* __restrict__ cand, const int64_t* __restrict__ cand_start, const int64_t* __restrict__ cand_len,
    const int64_t* __restrict__ ref, const int64_t* __restrict__ ref_start, const int64_t* __restrict__ ref_len,
    int64_t* __restrict__ clipped, int64_t* __restrict__ bad, int K, int max_n, int max_len, int P) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long ng_smem[];
  unsigned long long* kc = ng_smem;
  unsigned long long* kr = ng_smem + P;
  unsigned short* ic = reinterpret_cast<unsigned short*>(ng_smem + 2 * P);
  unsigned short* ir = ic + (P + 4);
  int* red = reinterpret_cast<int*>(ir + (P + 4));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const int64_t lc64 = cand_len[b], lr64 = ref_len[b];
  const bool bad_len = lc64 < 0 || lc64 > max_len || lr64 < 0 || lr64 > max_len;
  const int lc = bad_len ? 0 : (int)lc64, lr = bad_len ? 0 : (int)lr64;      // (<= max_len <= P)
  int bad_id = 0;
  if (!bad_len) {
    const int64_t* pc = cand + cand_start[b];
    const int64_t* pr = ref + ref_start[b];
    for (int i = tid; i < lc; i += 256) {
      const int64_t v = pc[i];
      const bool ok = v >= 0 && v < K;
      bad_id |= ok ? 0 : 1;
      ic[i] = ok ? (unsigned short)v : (unsigned short)0;
    }
    for (int i = tid; i < lr; i += 256) {
      const int64_t v = pr[i];
      const bool ok = v >= 0 && v < K;
      bad_id |= ok ? 0 : 1;
      ir[i] = ok ? (unsigned short)v : (unsigned short)0;
    }
  }
  int64_t* row = clipped + b * max_n;
  if (__syncthreads_or(bad_id | (bad_len ? 1 : 0))) {     // (uniform; the ids are in LDS behind this barrier)
    ng_mark_bad(row, max_n, bad, tid);
    return;
  }
  for (int n = 1; n <= max_n; ++n) {                      // (everything that steers the barriers below is uniform in the workgroup)
    const int nc = lc - n + 1, nr = lr - n + 1;
    if (nc <= 0 || nr <= 0) {
      if (tid == 0) row[n - 1] = 0;
      continue;
    }
    for (int i = tid; i < nc; i += 256) {
      unsigned long long k = ic[i];
      for (int j = 1; j < n; ++j) k |= (unsigned long long)ic[i + j] << (16 * j);
      kc[i] = k;
    }
    for (int i = tid; i < nr; i += 256) {
      unsigned long long k = ir[i];
      for (int j = 1; j < n; ++j) k |= (unsigned long long)ir[i + j] << (16 * j);
      kr[i] = k;
    }
    __syncthreads();
    const int nm = nc > nr ? nc : nr;
    for (int k = 2, lh = 0; (k >> 1) < nm; k <<= 1, ++lh) {      // merges of k keys, up to the first power of two >= nm
      const int h = 1 << lh;
      for (int t = tid; t < (P >> 1); t += 256) {         // mirror step: i <-> the same offset from the block's other end
        const int blk = t >> lh, off = t & (h - 1);
        const int i = blk * k + off, l = blk * k + (k - 1 - off);
        if (i >= nm) break;
        if (l < nc) ng_cmpx(kc, i, l);
        if (l < nr) ng_cmpx(kr, i, l);
      }
      __syncthreads();
      for (int lj = lh - 1; lj >= 0; --lj) {              // halving steps: i <-> i + j
        const int j = 1 << lj;
        for (int t = tid; t < (P >> 1); t += 256) {
          const int blk = t >> lj, off = t & (j - 1);
          const int i = blk * 2 * j + off, l = i + j;
          if (i >= nm) break;
          if (l < nc) ng_cmpx(kc, i, l);
          if (l < nr) ng_cmpx(kr, i, l);
        }
        __syncthreads();
      }
    }
    int sum = 0;
    for (int i = tid; i < nc; i += 256) {
      const unsigned long long key = kc[i];
      if (i > 0 && kc[i - 1] == key) continue;            // not a run start
      const int c = ng_bound<true>(kc, i, nc, key) - i;
      const int r0 = ng_bound<false>(kr, 0, nr, key);
      const int r = ng_bound<true>(kr, r0, nr, key) - r0;
      sum += c < r ? c : r;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) red[wave] = sum;
    __syncthreads();                                      // (also: every read of the sorted keys is done before the next order's build)
    if (tid == 0) row[n - 1] = (int64_t)((red[0] + red[1]) + (red[2] + red[3]));
    __syncthreads();                                      // (red is free again)
  }
}

inline size_t ng_sort_lds(int P) { return (size_t)2 * P * 8 + (size_t)2 * (P + 4) * 2 + 4 * sizeof(int); }

}  // namespace
}  // namespace g2v

using namespace g2v;

extern "C" int g2v_ngram_clipped_counts(const int64_t* cand, const int64_t* cand_start, const int64_t* cand_len, const int64_t* ref,
                                        const int64_t* ref_start, const int64_t* ref_len, int64_t* clipped, int64_t* bad, int64_t B,
                                        int K, int max_n, int max_len, g2v_stream_t stream) {
  G2V_REQUIRE(cand && cand_start && cand_len && ref && ref_start && ref_len && clipped && bad, "null pointer");
  G2V_REQUIRE(B > 0 && B < ((int64_t)1 << 31) - 4, "B outside [1, 2^31 - 4)");
  G2V_REQUIRE(K > 0 && max_n > 0 && max_len >= 0, "non-positive K or max_n, or a negative max_len");
  if (K > NG_MAX_K || max_n > NG_MAX_N || max_len > NG_MAX_LEN) {
    set_error("g2v_ngram_clipped_counts: K = %d, max_n = %d, max_len = %d: the kernels hold K <= %d (16-bit ids), max_n <= %d and "
              "max_len <= %d",
              K, max_n, max_len, NG_MAX_K, NG_MAX_N, NG_MAX_LEN);
    return G2V_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  if (max_len <= NG_WAVE_LEN) {
    hipLaunchKernelGGL(ngram_wave_kernel, dim3((unsigned)((B + NG_WAVE_PAIRS - 1) / NG_WAVE_PAIRS)), dim3(64 * NG_WAVE_PAIRS), 0, st, cand,
                       cand_start, cand_len, ref, ref_start, ref_len, clipped, bad, B, K, max_n, max_len);
  } else {
    int P = 128;
    while (P < max_len) P <<= 1;
    if (!g2v_internal_lds_reserve((const void*)ngram_sort_kernel, ng_sort_lds(P))) {
      set_error("g2v_ngram_clipped_counts: cannot reserve LDS");
      return G2V_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(ngram_sort_kernel, dim3((unsigned)B), dim3(256), ng_sort_lds(P), st, cand, cand_start, cand_len, ref, ref_start,
                       ref_len, clipped, bad, K, max_n, max_len, P);
  }
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
