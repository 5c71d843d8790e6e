// kmeans.hip -- Lloyd k-means over (N, E) fp32 latent rows on the device (gesture2vec_amd/kmeans.py; the reference's
// Clustering.py:705-725 sklearn.cluster.KMeans and the kmeanmodel.predict call sites).  The assignment half of an iteration is the
// exact argmin of vq.hip, unchanged; this file holds the rest:
//   g2v_kmeans_update      labels -> counts, float64 sums, new centres, inertia, centre shift, changed labels, empty-cluster relocation,
//                          and the convergence decision, kept in a device state block
//   g2v_kmeans_commit      centres / labels of the iteration become the current ones (gated on that state block)
//   g2v_kmeans_tolerance   tol * mean_e Var(x_e) from one pass of float64 column moments
//   g2v_kmeans_pp_step     one greedy k-means++ step over up to 8 candidate rows
//
// ---- update -----------------------------------------------------------------------------------------------------------------------
// x is read once, through an inverted index (atomic-free scatter-add, cdna_hip_programming.md Appendix B; the first four kernels
// live in km_sort.hpp, which silhouette.hip shares):
//   km_hist_kernel      one workgroup per KM_SORT_ROWS consecutive rows: its label histogram (LDS integer atomics) -> hist[block][k];
//                       labels that differ from the previous ones are counted (integer atomic)
//   km_prefix_kernel    hist[.][k] -> exclusive prefix over the blocks (where block b's rows of cluster k start inside the cluster's
//                       list), counts[k]
//   km_scan_kernel      one workgroup: cl_start[k] (exclusive scan of the counts), ch_first[k] (exclusive scan of
//                       ceil(count / KM_CHUNK)), the number of empty clusters
//   km_scatter_kernel   one wave per block of rows, in row order: sorted[cl_start[k] + offset++] = row.  Rows of one cluster appear in
//                       ascending row order: the index is a stable counting sort and does not depend on timing
//   km_chunk_kernel     one wave per chunk of <= KM_CHUNK rows of one cluster, four rows in flight: lane l holds columns 4l .. 4l+3 and
//                       256 + 4l .. of the running float64 sum and of sum (x - c_old)^2 -> part[chunk][E + 1]
//   km_fold_kernel      one workgroup per cluster adds its chunks' partials in chunk order -> sums[k][E], cl_inertia[k]
//   km_rowdist_kernel, km_relocate_kernel   only when a cluster is empty (they return at once otherwise): |x - c_old[label]|^2 per row in
//                       float64 (pair_dist.hpp: pd_pair_sq), then one workgroup picks the n_empty farthest rows (farthest first,
//                       lowest row on ties), takes each out of its cluster's sum / count and makes it the sum of the next empty
//                       cluster in ascending id
//   km_center_kernel    one workgroup per cluster: c_new = (float)(sum / count) (a cluster left without rows keeps c_old), its shift
//   km_finish_kernel    one workgroup: shift and inertia summed over the clusters in a fixed tree, the state block
// Every float64 sum is formed in an order fixed by (N, E, K) and the labels: no floating-point atomics, the same input gives the same
// bits, and no result depends on how many workgroups a launch happens to use.
#include "common.hpp"
#include "km_sort.hpp"
#include "pair_dist.hpp"

#include <type_traits>

namespace g2v {
namespace {

constexpr int KM_MAX_E = 512;
constexpr int KM_CHUNK = 512;               // rows of one cluster a wave sums before its partial is written
constexpr int KM_FLIGHT = 4;                // rows a wave has in flight
constexpr int KM_COL_ROWS = 1024;           // rows per workgroup of the column moments
constexpr int KM_PP_ROWS = 1024;            // rows per workgroup (and per partial sum) of the k-means++ step
constexpr int KM_PP_CAND = 8;

struct KmLayout {
  int nb;                  // sort blocks
  int64_t max_chunks;
  size_t hdr, hist, cl_start, ch_first, sorted, part, cl_inertia, cl_shift, rowdist, sel, empties, total;
};

inline KmLayout km_layout(int64_t N, int E, int K) {
  KmLayout l;
  l.nb = cdiv(N, KM_SORT_ROWS);
  l.max_chunks = N / KM_CHUNK + K;
  size_t o = 0;
  l.hdr = o;        o = km_align(o + HD_WORDS * sizeof(unsigned long long));
  l.hist = o;       o = km_align(o + (size_t)l.nb * K * sizeof(int));
  l.cl_start = o;   o = km_align(o + (size_t)(K + 1) * sizeof(int));
  l.ch_first = o;   o = km_align(o + (size_t)(K + 1) * sizeof(int));
  l.sorted = o;     o = km_align(o + (size_t)N * sizeof(int));
  l.part = o;       o = km_align(o + (size_t)l.max_chunks * (E + 1) * sizeof(double));
  l.cl_inertia = o; o = km_align(o + (size_t)K * sizeof(double));
  l.cl_shift = o;   o = km_align(o + (size_t)K * sizeof(double));
  l.rowdist = o;    o = km_align(o + (size_t)N * sizeof(double));
  l.sel = o;        o = km_align(o + (size_t)K * sizeof(int));
  l.empties = o;    o = km_align(o + (size_t)K * sizeof(int));
  l.total = o;
  return l;
}

__global__ __launch_bounds__(256) void km_chunk_kernel(const float* __restrict__ x, const float* __restrict__ centers,
                                                      const int* __restrict__ sorted, const int* __restrict__ cl_start,
                                                      const int* __restrict__ ch_first, const unsigned long long* __restrict__ hdr,
                                                      double* __restrict__ part, int E, int K, const double* __restrict__ state) {
  if (km_gated(state)) return;
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= (int64_t)hdr[HD_CHUNKS]) return;
  int lo = 0, hi = K;                                       // the cluster k with ch_first[k] <= c < ch_first[k + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ch_first[mid] <= (int)c) lo = mid; else hi = mid;
  }
  const int k = lo;
  const int start = cl_start[k] + ((int)c - ch_first[k]) * KM_CHUNK;
  const int len = min(KM_CHUNK, cl_start[k + 1] - start);
  const int nv = E >> 2;
  const bool has0 = lane < nv, has1 = lane + 64 < nv;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4* cp = reinterpret_cast<const float4*>(centers + (size_t)k * E);
  const int i0 = has0 ? lane : 0, i1 = has1 ? lane + 64 : 0;
  const float4 c0r = cp[i0], c1r = cp[i1];
  const float4 c0 = has0 ? c0r : zero, c1 = has1 ? c1r : zero;
  const double cd[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double dist = 0.0;
  for (int base = 0; base < len; base += 64) {
    const int cnt = min(64, len - base);
    const int myrow = lane < cnt ? sorted[start + base + lane] : 0;
    // R rows in flight: all their loads are issued before the first is consumed; the sums still grow in row order
    auto rows = [&](int u, auto rc) {
      constexpr int R = decltype(rc)::value;
      float4 a[R][2];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const int r = __shfl(myrow, u + j);
        const float4* p = reinterpret_cast<const float4*>(x + (int64_t)r * E);
        a[j][0] = p[i0];                                    // unconditional 16-byte loads (a lane without a column re-reads
        a[j][1] = p[i1];                                    // column group 0 and drops it below): no branch, no wait between them
      }
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const float4 a0 = has0 ? a[j][0] : zero, a1 = has1 ? a[j][1] : zero;
        const double v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          s[q] += v[q];
          const double d = v[q] - cd[q];
          dist = fma(d, d, dist);
        }
      }
    };
    int u = 0;
    for (; u + KM_FLIGHT <= cnt; u += KM_FLIGHT) rows(u, std::integral_constant<int, KM_FLIGHT>{});
    for (; u < cnt; ++u) rows(u, std::integral_constant<int, 1>{});
  }
  double* out = part + (size_t)c * (E + 1);
  if (has0) {
    out[4 * lane + 0] = s[0];
    out[4 * lane + 1] = s[1];
    out[4 * lane + 2] = s[2];
    out[4 * lane + 3] = s[3];
  }
  if (has1) {
    out[256 + 4 * lane + 0] = s[4];
    out[256 + 4 * lane + 1] = s[5];
    out[256 + 4 * lane + 2] = s[6];
    out[256 + 4 * lane + 3] = s[7];
  }
  dist = km_wave_sum(dist);
  if (lane == 0) out[E] = dist;
}

__global__ __launch_bounds__(256) void km_fold_kernel(const double* __restrict__ part, const int* __restrict__ ch_first,
                                                     double* __restrict__ sums, double* __restrict__ cl_inertia, int E,
                                                     const double* __restrict__ state) {
  if (km_gated(state)) return;
  const int k = blockIdx.x;
  const int first = ch_first[k], nch = ch_first[k + 1] - first;
  for (int e = threadIdx.x; e <= E; e += 256) {
    const double* p = part + (size_t)first * (E + 1) + e;
    double acc = 0.0;
    int j = 0;
    for (; j + 4 <= nch; j += 4) {
      const double v0 = p[(size_t)j * (E + 1)], v1 = p[(size_t)(j + 1) * (E + 1)], v2 = p[(size_t)(j + 2) * (E + 1)],
                   v3 = p[(size_t)(j + 3) * (E + 1)];
      acc += v0;
      acc += v1;
      acc += v2;
      acc += v3;
    }
    for (; j < nch; ++j) acc += p[(size_t)j * (E + 1)];
    if (e < E) sums[(size_t)k * E + e] = acc;
    else cl_inertia[k] = acc;
  }
}

// rowdist[n] = |x_n - c_old[label_n]|^2 in float64, -1 for a row whose label is out of range.  One wave per row, grid-stride.
__global__ __launch_bounds__(256) void km_rowdist_kernel(const float* __restrict__ x, const int64_t* __restrict__ labels,
                                                        const float* __restrict__ centers, int64_t N, int E, int K,
                                                        const unsigned long long* __restrict__ hdr, double* __restrict__ rowdist,
                                                        const double* __restrict__ state) {
  if (km_gated(state) || hdr[HD_EMPTY] == 0) return;
  __builtin_assume((E & 3) == 0);                             // (whole vectors only: pd_pair_sq has no tail here)
  const int lane = threadIdx.x & 63;
  for (int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); n < N; n += (int64_t)gridDim.x * 4) {
    const int64_t lab = labels[n];
    if (lab < 0 || lab >= K) {
      if (lane == 0) rowdist[n] = -1.0;
      continue;
    }
    const double dist = pd_pair_sq(x + n * E, centers + (size_t)lab * E, E, lane);
    if (lane == 0) rowdist[n] = dist;
  }
}

__global__ __launch_bounds__(1024) void km_relocate_kernel(const float* __restrict__ x, const int64_t* __restrict__ labels, int64_t N,
                                                          int E, int K, unsigned long long* __restrict__ hdr,
                                                          double* __restrict__ rowdist, int* __restrict__ sel, int* __restrict__ empties,
                                                          int64_t* __restrict__ counts, double* __restrict__ sums,
                                                          int64_t* __restrict__ relocated_rows, const double* __restrict__ state) {
  __shared__ double sd[1024];
  __shared__ int64_t sn[1024];
  if (km_gated(state) || hdr[HD_EMPTY] == 0) return;
  const int tid = threadIdx.x;
  const unsigned long long n_empty = hdr[HD_EMPTY], n_valid = hdr[HD_VALID];
  const int n_reloc = (int)(n_empty < n_valid ? n_empty : n_valid);
  if (tid == 0) {                                           // the empty clusters in ascending id
    int e = 0;
    for (int k = 0; k < K && e < n_reloc; ++k)
      if (counts[k] == 0) empties[e++] = k;
  }
  for (int r = 0; r < n_reloc; ++r) {                       // the farthest row still unchosen; the lowest row among equals
    double bd = -1.0;
    int64_t bn = -1;
    for (int64_t n = tid; n < N; n += 1024) {
      const double d = rowdist[n];
      if (d > bd) {
        bd = d;
        bn = n;
      }
    }
    sd[tid] = bd;
    sn[tid] = bn;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
      if (tid < s) {
        const double d = sd[tid + s];
        const int64_t n = sn[tid + s];
        if (n >= 0 && (sn[tid] < 0 || d > sd[tid] || (d == sd[tid] && n < sn[tid]))) {
          sd[tid] = d;
          sn[tid] = n;
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      sel[r] = (int)sn[0];
      if (sn[0] >= 0) rowdist[sn[0]] = -2.0;
    }
    __syncthreads();
  }
  __threadfence_block();
  int moved = 0;                                            // (uniform over the workgroup)
  for (int r = 0; r < n_reloc; ++r) {
    const int row = sel[r];
    if (row < 0) continue;                                  // nothing left to choose (the remaining distances are NaN)
    const int old_k = (int)labels[row], new_k = empties[moved];
    for (int e = tid; e < E; e += 1024) {
      const double v = (double)x[(int64_t)row * E + e];
      sums[(size_t)old_k * E + e] -= v;
      sums[(size_t)new_k * E + e] = v;
    }
    if (tid == 0) {
      counts[old_k] -= 1;
      counts[new_k] = 1;
      if (relocated_rows) relocated_rows[moved] = row;
    }
    ++moved;
    __syncthreads();
  }
  if (tid == 0) hdr[HD_RELOC] = (unsigned long long)moved;
}

__global__ __launch_bounds__(128) void km_center_kernel(const int64_t* __restrict__ counts, const double* __restrict__ sums,
                                                       const float* __restrict__ c_old, float* __restrict__ c_new,
                                                       double* __restrict__ cl_shift, int E, const double* __restrict__ state) {
  __shared__ double sh[128];
  if (km_gated(state)) return;
  const int k = blockIdx.x;
  const int64_t cnt = counts[k];
  double acc = 0.0;
  for (int e = threadIdx.x; e < E; e += 128) {
    const float o = c_old[(size_t)k * E + e];
    const float c = cnt > 0 ? (float)(sums[(size_t)k * E + e] / (double)cnt) : o;
    c_new[(size_t)k * E + e] = c;
    const double d = (double)c - (double)o;
    acc = fma(d, d, acc);
  }
  acc = km_block_sum(acc, sh);
  if (threadIdx.x == 0) cl_shift[k] = acc;
}

__global__ __launch_bounds__(1024) void km_finish_kernel(const double* __restrict__ cl_shift, const double* __restrict__ cl_inertia,
                                                        int K, int64_t N, int have_prev, const unsigned long long* __restrict__ hdr,
                                                        double* __restrict__ stats, double* __restrict__ state) {
  __shared__ double sh[1024];
  const int tid = threadIdx.x;
  if (km_gated(state)) {
    if (tid == 0) state[ST_ACTIVE] = 0.0;
    return;
  }
  double a = 0.0, b = 0.0;
  for (int k = tid; k < K; k += 1024) {
    a += cl_shift[k];
    b += cl_inertia[k];
  }
  const double shift = km_block_sum(a, sh);
  __syncthreads();
  const double inertia = km_block_sum(b, sh);
  if (tid != 0) return;
  const double changed = have_prev ? (double)hdr[HD_CHANGED] : (double)N;
  const double reloc = (double)hdr[HD_RELOC];
  stats[0] = inertia;
  stats[1] = shift;
  stats[2] = changed;
  stats[3] = reloc;
  if (state) {
    state[ST_ITER] += 1.0;
    state[ST_CHANGED] = changed;
    state[ST_SHIFT] = shift;
    state[ST_INERTIA] = inertia;
    state[ST_RELOC] = reloc;
    state[ST_ACTIVE] = 1.0;
    if ((have_prev && changed == 0.0) || shift <= state[ST_TOL]) state[ST_DONE] = 1.0;
  }
}

__global__ __launch_bounds__(256) void km_commit_kernel(const double* __restrict__ state, const float* __restrict__ c_new,
                                                       float* __restrict__ c, int64_t ke, const int64_t* __restrict__ l_new,
                                                       int64_t* __restrict__ l, int64_t N) {
  if (state[ST_ACTIVE] == 0.0) return;
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  for (int64_t i = i0; i < ke; i += step) c[i] = c_new[i];
  if (l_new && l)
    for (int64_t i = i0; i < N; i += step) l[i] = l_new[i];
}

// ---- tolerance --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void km_colmom_kernel(const float* __restrict__ x, int64_t N, int E, double* __restrict__ part) {
  const int e = threadIdx.x;
  if (e >= E) return;
  const int64_t r0 = (int64_t)blockIdx.x * KM_COL_ROWS;
  const int rows = (int)min((int64_t)KM_COL_ROWS, N - r0);
  const float* p = x + r0 * E + e;
  double s1 = 0.0, s2 = 0.0;
  int r = 0;
  for (; r + 4 <= rows; r += 4) {
    const double v0 = p[(int64_t)r * E], v1 = p[(int64_t)(r + 1) * E], v2 = p[(int64_t)(r + 2) * E], v3 = p[(int64_t)(r + 3) * E];
    s1 += v0; s2 = fma(v0, v0, s2);
    s1 += v1; s2 = fma(v1, v1, s2);
    s1 += v2; s2 = fma(v2, v2, s2);
    s1 += v3; s2 = fma(v3, v3, s2);
  }
  for (; r < rows; ++r) {
    const double v = p[(int64_t)r * E];
    s1 += v;
    s2 = fma(v, v, s2);
  }
  part[((size_t)blockIdx.x * 2 + 0) * E + e] = s1;
  part[((size_t)blockIdx.x * 2 + 1) * E + e] = s2;
}

__global__ __launch_bounds__(512) void km_colvar_kernel(const double* __restrict__ part, int nslab, int64_t N, int E, double scale,
                                                       double* __restrict__ out) {
  __shared__ double sh[512];
  const int e = threadIdx.x;
  double var = 0.0;
  if (e < E) {
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < nslab; ++b) {
      s1 += part[((size_t)b * 2 + 0) * E + e];
      s2 += part[((size_t)b * 2 + 1) * E + e];
    }
    const double mean = s1 / (double)N;
    var = s2 / (double)N - mean * mean;
    var = var > 0.0 ? var : 0.0;
  }
  const double tot = km_block_sum(var, sh);
  if (e == 0) out[0] = scale * (tot / (double)E);
}

// ---- k-means++ --------------------------------------------------------------------------------------------------------------------
struct PpPick {
  int64_t block[KM_PP_CAND];
  double resid[KM_PP_CAND];
};

// candidate t: direct -> the given row; else the first row i of block[t] whose running sum of closest[] over the block reaches resid[t]
__global__ __launch_bounds__(64 * KM_PP_CAND) void pp_pick_kernel(const double* __restrict__ closest, int64_t N, PpPick pick, int ncand,
                                                                 int direct, int64_t* __restrict__ cand) {
  const int lane = threadIdx.x & 63, t = threadIdx.x >> 6;
  if (t >= ncand) return;
  if (direct) {
    if (lane == 0) cand[t] = min(max(pick.block[t], (int64_t)0), N - 1);
    return;
  }
  const int64_t r0 = pick.block[t] * KM_PP_ROWS;
  const int rows = (int)min((int64_t)KM_PP_ROWS, N - r0);
  constexpr int PER = KM_PP_ROWS / 64;
  double v[PER], loc = 0.0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int r = lane * PER + i;
    v[i] = r < rows ? closest[r0 + r] : 0.0;
    loc += v[i];
  }
  double incl = loc;                                         // inclusive scan over the lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_up(incl, o);
    if (lane >= o) incl += u;
  }
  double run = incl - loc;
  int found = KM_PP_ROWS;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    run += v[i];
    if (found == KM_PP_ROWS && run >= pick.resid[t]) found = lane * PER + i;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) found = min(found, __shfl_xor(found, o));
  if (lane == 0) cand[t] = r0 + min(found, rows - 1);
}

// newd[t][n] = min(closest[n], |x_n - x_cand[t]|^2) in float64; ppart[block][t] = sum over the block's rows, in row order per wave
__global__ __launch_bounds__(256) void pp_dist_kernel(const float* __restrict__ x, int64_t N, int E, const double* __restrict__ closest,
                                                     const int64_t* __restrict__ cand, int ncand, double* __restrict__ newd,
                                                     double* __restrict__ ppart) {
  __shared__ double wpot[4][KM_PP_CAND];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nv = E >> 2;
  const bool has0 = lane < nv, has1 = lane + 64 < nv;
  const int i0 = has0 ? lane : 0, i1 = has1 ? lane + 64 : 0;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 c[KM_PP_CAND][2];
#pragma unroll
  for (int t = 0; t < KM_PP_CAND; ++t) {
    c[t][0] = zero;
    c[t][1] = zero;
    if (t < ncand) {
      const float4* p = reinterpret_cast<const float4*>(x + cand[t] * E);
      const float4 r0 = p[i0], r1 = p[i1];
      c[t][0] = has0 ? r0 : zero;
      c[t][1] = has1 ? r1 : zero;
    }
  }
  double pot[KM_PP_CAND];
#pragma unroll
  for (int t = 0; t < KM_PP_CAND; ++t) pot[t] = 0.0;
  constexpr int WROWS = KM_PP_ROWS / 4;
  const int64_t r0 = (int64_t)blockIdx.x * KM_PP_ROWS + w * WROWS;
  for (int i = 0; i < WROWS; ++i) {
    const int64_t n = r0 + i;
    if (n >= N) break;
    const float4* p = reinterpret_cast<const float4*>(x + n * E);
    const float4 l0 = p[i0], l1 = p[i1];                     // unconditional 16-byte loads; lanes without a column drop theirs
    const float4 a0 = has0 ? l0 : zero, a1 = has1 ? l1 : zero;
    const double v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    const double cl = closest[n];
#pragma unroll
    for (int t = 0; t < KM_PP_CAND; ++t) {
      if (t < ncand) {
        const double cv[8] = {c[t][0].x, c[t][0].y, c[t][0].z, c[t][0].w, c[t][1].x, c[t][1].y, c[t][1].z, c[t][1].w};
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const double d = v[q] - cv[q];
          acc = fma(d, d, acc);
        }
        acc = km_wave_sum(acc);
        const double m = acc < cl ? acc : cl;
        if (lane == 0) newd[(size_t)t * N + n] = m;
        pot[t] += m;
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < KM_PP_CAND; ++t) wpot[w][t] = pot[t];
  }
  __syncthreads();
  if (threadIdx.x < KM_PP_CAND)
    ppart[(size_t)blockIdx.x * KM_PP_CAND + threadIdx.x] =
        ((wpot[0][threadIdx.x] + wpot[1][threadIdx.x]) + wpot[2][threadIdx.x]) + wpot[3][threadIdx.x];
}

// potentials per candidate (blocks in a fixed order per lane, then the xor tree), the best candidate (lowest index among equals)
__global__ __launch_bounds__(64 * KM_PP_CAND) void pp_reduce_kernel(const double* __restrict__ ppart, int nblk, int ncand,
                                                                   const int64_t* __restrict__ cand, int* __restrict__ best,
                                                                   double* __restrict__ tail) {
  __shared__ double pots[KM_PP_CAND];
  const int lane = threadIdx.x & 63, t = threadIdx.x >> 6;
  double acc = 0.0;
  if (t < ncand)
    for (int b = lane; b < nblk; b += 64) acc += ppart[(size_t)b * KM_PP_CAND + t];
  acc = km_wave_sum(acc);
  if (lane == 0) pots[t] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    int bt = 0;
    for (int u = 1; u < ncand; ++u)
      if (pots[u] < pots[bt]) bt = u;
    best[0] = bt;
    for (int u = 0; u < KM_PP_CAND; ++u) tail[u] = u < ncand ? pots[u] : 0.0;
    tail[KM_PP_CAND] = (double)bt;
    tail[KM_PP_CAND + 1] = (double)cand[bt];
    tail[KM_PP_CAND + 2] = pots[bt];
  }
}

__global__ __launch_bounds__(256) void pp_commit_kernel(const float* __restrict__ x, int64_t N, int E, const double* __restrict__ newd,
                                                       const int* __restrict__ best, const int64_t* __restrict__ cand,
                                                       double* __restrict__ closest, double* __restrict__ block_sums,
                                                       float* __restrict__ center_out) {
  __shared__ double sh[256];
  const int bt = best[0];
  const int64_t r0 = (int64_t)blockIdx.x * KM_PP_ROWS;
  double acc = 0.0;
  for (int i = threadIdx.x; i < KM_PP_ROWS; i += 256) {
    const int64_t n = r0 + i;
    if (n < N) {
      const double v = newd[(size_t)bt * N + n];
      closest[n] = v;
      acc += v;
    }
  }
  acc = km_block_sum(acc, sh);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = acc;
  if (blockIdx.x == 0 && center_out) {
    const float* p = x + cand[bt] * E;
    for (int e = threadIdx.x; e < E; e += 256) center_out[e] = p[e];
  }
}

inline bool km_shape_ok(int64_t N, int E, int K) { return N > 0 && N < ((int64_t)1 << 31) - KM_SORT_ROWS && E > 0 && K > 0; }

}  // namespace
}  // namespace g2v

using namespace g2v;

extern "C" size_t g2v_kmeans_update_workspace(int64_t N, int E, int K) {
  if (!km_shape_ok(N, E, K) || E > KM_MAX_E) return 0;
  return km_layout(N, E, K).total;
}

extern "C" int g2v_kmeans_update(const float* x, const int64_t* labels, const int64_t* prev_labels, const float* centers_old,
                                 int64_t N, int E, int K, int relocate, int64_t* counts, double* sums, float* centers_new,
                                 double* stats, int64_t* relocated_rows, double* state, void* workspace, size_t workspace_bytes,
                                 g2v_stream_t stream) {
  G2V_REQUIRE(x && labels && centers_old && counts && sums && centers_new && stats && workspace, "null pointer");
  G2V_REQUIRE(km_shape_ok(N, E, K), "sizes: 1 <= N < 2^31 - 2048, E >= 1, K >= 1");
  if ((E & 3) != 0 || E > KM_MAX_E) {
    set_error("g2v_kmeans_update: needs E %% 4 == 0 and E <= %d (E = %d)", KM_MAX_E, E);
    return G2V_ERR_UNSUPPORTED;
  }
  G2V_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(centers_old) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "x, centers_old and workspace must be 16-byte aligned");
  const KmLayout l = km_layout(N, E, K);
  if (workspace_bytes < l.total) {
    set_error("g2v_kmeans_update: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  unsigned long long* hdr = (unsigned long long*)(ws + l.hdr);
  int* hist = (int*)(ws + l.hist);
  int* cl_start = (int*)(ws + l.cl_start);
  int* ch_first = (int*)(ws + l.ch_first);
  int* sorted = (int*)(ws + l.sorted);
  double* part = (double*)(ws + l.part);
  double* cl_inertia = (double*)(ws + l.cl_inertia);
  double* cl_shift = (double*)(ws + l.cl_shift);
  double* rowdist = (double*)(ws + l.rowdist);
  int* sel = (int*)(ws + l.sel);
  int* empties = (int*)(ws + l.empties);
  const int use_lds = K <= KM_LDS_BINS ? 1 : 0;
  const double* gate = state;

  (void)hipMemsetAsync(hdr, 0, HD_WORDS * sizeof(unsigned long long), st);
  if (!use_lds) (void)hipMemsetAsync(hist, 0, (size_t)l.nb * K * sizeof(int), st);
  hipLaunchKernelGGL(km_hist_kernel, dim3(l.nb), dim3(256), 0, st, labels, prev_labels, N, K, hist, hdr, use_lds, gate);
  hipLaunchKernelGGL(km_prefix_kernel, dim3(cdiv(K, 64)), dim3(1024), 0, st, hist, l.nb, K, counts, gate);
  hipLaunchKernelGGL(km_scan_kernel, dim3(1), dim3(1024), 0, st, K, KM_CHUNK, (const int64_t*)counts, cl_start, ch_first, hdr, gate);
  int label_bits = 0;
  while (label_bits < 31 && ((int64_t)1 << label_bits) < K) ++label_bits;
  hipLaunchKernelGGL(km_scatter_kernel, dim3(l.nb), dim3(64), 0, st, labels, N, K, label_bits, hist, (const int*)cl_start, sorted,
                     use_lds, gate);
  hipLaunchKernelGGL(km_chunk_kernel, dim3(cdiv(l.max_chunks, 4)), dim3(256), 0, st, x, centers_old, (const int*)sorted,
                     (const int*)cl_start, (const int*)ch_first, (const unsigned long long*)hdr, part, E, K, gate);
  hipLaunchKernelGGL(km_fold_kernel, dim3(K), dim3(256), 0, st, (const double*)part, (const int*)ch_first, sums, cl_inertia, E, gate);
  if (relocate) {
    const int64_t rb = (N + 3) / 4;
    hipLaunchKernelGGL(km_rowdist_kernel, dim3((int)(rb < 4096 ? rb : 4096)), dim3(256), 0, st, x, labels, centers_old, N, E, K,
                       (const unsigned long long*)hdr, rowdist, gate);
    hipLaunchKernelGGL(km_relocate_kernel, dim3(1), dim3(1024), 0, st, x, labels, N, E, K, hdr, rowdist, sel, empties, counts, sums,
                       relocated_rows, gate);
  }
  hipLaunchKernelGGL(km_center_kernel, dim3(K), dim3(128), 0, st, (const int64_t*)counts, (const double*)sums, centers_old,
                     centers_new, cl_shift, E, gate);
  hipLaunchKernelGGL(km_finish_kernel, dim3(1), dim3(1024), 0, st, (const double*)cl_shift, (const double*)cl_inertia, K, N,
                     prev_labels ? 1 : 0, (const unsigned long long*)hdr, stats, state);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int g2v_kmeans_commit(const double* state, const float* centers_new, float* centers, int64_t n_center_elems,
                                 const int64_t* labels_new, int64_t* labels, int64_t N, g2v_stream_t stream) {
  G2V_REQUIRE(state && centers_new && centers, "null pointer");
  G2V_REQUIRE(n_center_elems > 0 && N >= 0, "negative size");
  const int64_t n = n_center_elems > N ? n_center_elems : N;
  const int64_t blocks = (n + 1023) / 1024;
  hipLaunchKernelGGL(km_commit_kernel, dim3((int)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream, state,
                     centers_new, centers, n_center_elems, labels_new, labels, N);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" size_t g2v_kmeans_tolerance_workspace(int64_t N, int E) {
  if (N <= 0 || E <= 0 || E > KM_MAX_E) return 0;
  return (size_t)cdiv(N, KM_COL_ROWS) * 2 * E * sizeof(double);
}

extern "C" int g2v_kmeans_tolerance(const float* x, int64_t N, int E, double tol, double* out, void* workspace,
                                    size_t workspace_bytes, g2v_stream_t stream) {
  G2V_REQUIRE(x && out && workspace, "null pointer");
  G2V_REQUIRE(N > 0 && E > 0, "non-positive size");
  if (E > KM_MAX_E) {
    set_error("g2v_kmeans_tolerance: E = %d is wider than %d columns", E, KM_MAX_E);
    return G2V_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < g2v_kmeans_tolerance_workspace(N, E)) {
    set_error("g2v_kmeans_tolerance: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int nslab = cdiv(N, KM_COL_ROWS);
  hipLaunchKernelGGL(km_colmom_kernel, dim3(nslab), dim3(512), 0, st, x, N, E, (double*)workspace);
  hipLaunchKernelGGL(km_colvar_kernel, dim3(1), dim3(512), 0, st, (const double*)workspace, nslab, N, E, tol, out);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int g2v_kmeans_pp_blocks(int64_t N) { return N > 0 ? cdiv(N, KM_PP_ROWS) : 0; }

extern "C" size_t g2v_kmeans_pp_workspace(int64_t N, int E) {
  if (N <= 0 || E <= 0 || E > KM_MAX_E) return 0;
  return km_align(256) + km_align((size_t)KM_PP_CAND * N * sizeof(double)) +
         km_align((size_t)cdiv(N, KM_PP_ROWS) * KM_PP_CAND * sizeof(double));
}

extern "C" int g2v_kmeans_pp_step(const float* x, int64_t N, int E, double* closest, const int64_t* pick_block,
                                  const double* pick_resid, int ncand, double* out, float* center_out, void* workspace,
                                  size_t workspace_bytes, g2v_stream_t stream) {
  G2V_REQUIRE(x && closest && pick_block && out && workspace, "null pointer");
  G2V_REQUIRE(N > 0 && E > 0 && ncand >= 1 && ncand <= KM_PP_CAND, "sizes: N >= 1, 1 <= ncand <= 8");
  if ((E & 3) != 0 || E > KM_MAX_E) {
    set_error("g2v_kmeans_pp_step: needs E %% 4 == 0 and E <= %d (E = %d)", KM_MAX_E, E);
    return G2V_ERR_UNSUPPORTED;
  }
  G2V_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
              "x and workspace must be 16-byte aligned");
  if (workspace_bytes < g2v_kmeans_pp_workspace(N, E)) {
    set_error("g2v_kmeans_pp_step: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  const int nblk = cdiv(N, KM_PP_ROWS);
  PpPick pick;
  for (int t = 0; t < KM_PP_CAND; ++t) {
    pick.block[t] = t < ncand ? pick_block[t] : 0;
    pick.resid[t] = (t < ncand && pick_resid) ? pick_resid[t] : 0.0;
    if (pick_resid) G2V_REQUIRE(pick.block[t] >= 0 && pick.block[t] < nblk, "pick_block outside the row blocks");
  }
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int64_t* cand = (int64_t*)ws;
  int* best = (int*)(ws + 128);
  double* newd = (double*)(ws + km_align(256));
  double* ppart = (double*)(ws + km_align(256) + km_align((size_t)KM_PP_CAND * N * sizeof(double)));
  hipLaunchKernelGGL(pp_pick_kernel, dim3(1), dim3(64 * KM_PP_CAND), 0, st, (const double*)closest, N, pick, ncand,
                     pick_resid ? 0 : 1, cand);
  hipLaunchKernelGGL(pp_dist_kernel, dim3(nblk), dim3(256), 0, st, x, N, E, (const double*)closest, (const int64_t*)cand, ncand, newd,
                     ppart);
  hipLaunchKernelGGL(pp_reduce_kernel, dim3(1), dim3(64 * KM_PP_CAND), 0, st, (const double*)ppart, nblk, ncand, (const int64_t*)cand,
                     best, out + nblk);
  hipLaunchKernelGGL(pp_commit_kernel, dim3(nblk), dim3(256), 0, st, x, N, E, (const double*)newd, (const int*)best,
                     (const int64_t*)cand, closest, out, center_out);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
