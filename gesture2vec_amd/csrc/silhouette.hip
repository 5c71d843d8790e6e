// silhouette.hip -- silhouette coefficient of a clustering of (N, E) fp32 latent rows (gesture2vec_amd/silhouette.py; the reference's
// Clustering.py:608-624 sklearn.metrics.silhouette_score over the k scan).  With c = labels[i], n_c rows in c and d the Euclidean distance:
//   a(i) = sum_{j in c, j != i} d(i, j) / (n_c - 1)        b(i) = min_{c' != c, n_c' > 0} sum_{j in c'} d(i, j) / n_c'
//   s(i) = (b - a) / max(a, b),  0 where n_c = 1 or a = b = 0
// The N x N distances are never stored; nor is an N x K table of cluster sums.
//
//   km_hist / km_prefix / km_scan / km_scatter (km_sort.hpp)   the stable counting sort of the row ids by label that g2v_kmeans_update
//                       uses, with lists cut into SUBTILES of 16 rows: a subtile never holds rows of two clusters
//   sil_slots_kernel    lays the subtiles out as SLOTS, 16 per subtile: slot_row[s] = the row in slot s (-1 where a subtile's tail is
//                       empty), slot_norm[s] = |x_row|^2, meta[subtile] = (cluster, rows, n_cluster).  The norm is the fp32 fma chain
//                       over k in the order the MFMAs below contract it, so two bitwise equal rows have d^2 = n + n - 2 G = 0 exactly
//   sil_tile_kernel     one workgroup (4 waves) per OWNER tile of 64 slots, whose rows stay in LDS for the whole kernel.  It sweeps all
//                       slots in order, 64 at a time, in k-chunks of 32 columns through a double-buffered LDS image (the loads of chunk
//                       g + 2 are in registers while chunk g is multiplied).  Wave w owns owner slots 16 w .. 16 w + 15 and keeps one
//                       16 x 16 fp32 accumulator per swept subtile: v_mfma_f32_16x16x4_f32 with the SWEPT rows as the A operand and the
//                       owner rows as B, so that lane (i, q) ends with G[swept 4 q + r][owner i] in register r: an owner row lives on
//                       one lane column and its distances are summed along registers.  Epilogue per subtile: d^2 = n_i + n_j - 2 G,
//                       sqrt, masked (tail slots, the pair i = j: exactly 0, never from arithmetic), added in float64 to the lane's
//                       running sum.  Where the next subtile belongs to another cluster the four lanes of an owner row add their
//                       running sums in a fixed tree and the (row, cluster) sum goes into a(i) or min -> b(i): every such sum has one
//                       owner, the wave, and is complete when it is used.
//   near pairs          d^2 < 1/8 (n_i + n_j): the Gram form has lost >= 3 bits there (its absolute error is ~3e-7 (n_i + n_j)); the
//                       wave re-evaluates such a pair as sum (x_i - x_j)^2 in float64 from the rows (pair_dist.hpp: pd_pair_sq;
//                       the loop is pd_near_pairs written out), as vq_fused_bx_kernel screens and then decides exactly.  Everywhere
//                       else d carries <= 1.2e-6 d.
//   sil_finish_kernel   out[0] = sum_i s(i) (one workgroup, rows dealt to threads by index, fixed tree), out[1] = non-empty clusters,
//                       counts[K] = rows whose label is outside [0, K) (they are in no list: never used as an address)
// Every sum is formed in an order fixed by (N, E, K, ld), the data and the labels: no floating-point atomics, and no result depends on
// how many workgroups a launch happens to use.  d(i, j) = d(j, i) is not exploited (each product is formed twice): it would need sums
// along the lane direction as well.
#include "common.hpp"
#include "km_sort.hpp"
#include "pair_dist.hpp"

namespace g2v {
namespace {

constexpr int SIL_MAX_E = 512;
constexpr int SIL_SUB = 16;                 // slots per subtile (= one MFMA tile edge)
constexpr int SIL_TILE = 64;                // slots per owner tile and per swept tile
constexpr int SIL_KC = 32;                  // columns per staged chunk of the swept tile
constexpr int SIL_SWLD = SIL_KC + 4;        // its LDS row stride (an odd number of 16-byte slots)
constexpr float SIL_NEAR = PD_NEAR;

struct SilLayout {
  int nb;                  // sort blocks
  int64_t slots;           // 16 per subtile, rounded up to whole tiles
  size_t hdr, hist, cl_start, sub_first, sorted, slot_row, slot_norm, meta, total;
};

inline SilLayout sil_layout(int64_t N, int K) {
  SilLayout l;
  l.nb = cdiv(N, KM_SORT_ROWS);
  const int64_t max_sub = N / SIL_SUB + K;                   // sum_k ceil(n_k / 16) <= N / 16 + K
  l.slots = (max_sub * SIL_SUB + SIL_TILE - 1) / SIL_TILE * SIL_TILE;
  size_t o = 0;
  l.hdr = o;        o = km_align(o + HD_WORDS * sizeof(unsigned long long));
  l.hist = o;       o = km_align(o + (size_t)l.nb * K * sizeof(int));
  l.cl_start = o;   o = km_align(o + (size_t)(K + 1) * sizeof(int));
  l.sub_first = o;  o = km_align(o + (size_t)(K + 1) * sizeof(int));
  l.sorted = o;     o = km_align(o + (size_t)N * sizeof(int));
  l.slot_row = o;   o = km_align(o + (size_t)l.slots * sizeof(int));
  l.slot_norm = o;  o = km_align(o + (size_t)l.slots * sizeof(float));
  l.meta = o;       o = km_align(o + (size_t)(l.slots / SIL_SUB) * sizeof(int4));
  l.total = o;
  return l;
}

inline bool sil_shape_ok(int64_t N, int E, int K) {
  return N >= 2 && N < ((int64_t)1 << 31) - KM_SORT_ROWS && E > 0 && K > 0 && N + (int64_t)SIL_SUB * K + SIL_TILE < ((int64_t)1 << 31);
}

inline size_t sil_lds_bytes(int E) {
  const int E16 = (E + 15) & ~15;
  return ((size_t)SIL_TILE * (E16 + 4) + 2 * SIL_TILE * SIL_SWLD) * sizeof(float);
}

__global__ __launch_bounds__(256) void sil_slots_kernel(const float* __restrict__ x, int64_t ld, int E, int K, int slots,
                                                       const int* __restrict__ sorted, const int* __restrict__ cl_start,
                                                       const int* __restrict__ sub_first, const unsigned long long* __restrict__ hdr,
                                                       int* __restrict__ slot_row, float* __restrict__ slot_norm,
                                                       int4* __restrict__ meta) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= slots) return;
  const int st = s >> 4, w = s & 15;
  int row = -1;
  int4 m = make_int4(-1, 0, 0, 0);
  if (st < (int)hdr[HD_CHUNKS]) {
    int lo = 0, hi = K;                                     // the cluster k with sub_first[k] <= st < sub_first[k + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (sub_first[mid] <= st) lo = mid; else hi = mid;
    }
    const int start = cl_start[lo] + (st - sub_first[lo]) * SIL_SUB;
    const int cnt = min(SIL_SUB, cl_start[lo + 1] - start);
    m = make_int4(lo, cnt, cl_start[lo + 1] - cl_start[lo], 0);
    if (w < cnt) row = sorted[start + w];
  }
  float acc = 0.f;
  if (row >= 0) {                                           // k in the order of the MFMA chain: 16 k0 + 4 q + e, q fastest, then e
    const float* p = x + (int64_t)row * ld;
    for (int k0 = 0; k0 < E; k0 += 16) {
      float4 v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        v[q] = ld4_or_zero(p + k0 + 4 * q, k0 + 4 * q < E);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = fmaf(v[q].x, v[q].x, acc);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = fmaf(v[q].y, v[q].y, acc);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = fmaf(v[q].z, v[q].z, acc);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = fmaf(v[q].w, v[q].w, acc);
    }
  }
  slot_row[s] = row;
  slot_norm[s] = acc;
  if (w == 0) meta[st] = m;
}

// (element-wise: a ternary over the float4 structs themselves becomes a select between two stack copies)
__device__ __forceinline__ float4 sil_keep(bool ok, const float4& v) {
  return make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
}

// |x_ri - x_rj| in float64 from the rows, by the whole wave; every lane returns the same bits
__device__ __forceinline__ double sil_pair(const float* __restrict__ x, int64_t ld, int E, int ri, int rj, int lane) {
  return sqrt(pd_pair_sq(x + (int64_t)ri * ld, x + (int64_t)rj * ld, E, lane));
}

// LDS: own[64][E16 + 4] | swept[2][64][SIL_SWLD]
__global__ __launch_bounds__(256) void sil_tile_kernel(const float* __restrict__ x, int64_t ld, int E,
                                                      const unsigned long long* __restrict__ hdr, const int* __restrict__ slot_row,
                                                      const float* __restrict__ slot_norm, const int4* __restrict__ meta,
                                                      double* __restrict__ a_out, double* __restrict__ b_out,
                                                      double* __restrict__ s_out) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __builtin_assume((E & 3) == 0);                           // (whole vectors only: pd_pair_sq has no tail here)
  const int n_sub = (int)hdr[HD_CHUNKS];
  const int n_mt = (n_sub + 3) >> 2;                        // tiles that hold a row
  if ((int)blockIdx.x >= n_mt) return;
  const int E16 = (E + 15) & ~15, ldo = E16 + 4;
  float* own = smem;
  float* swp = smem + SIL_TILE * ldo;
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nkc = (E16 + SIL_KC - 1) / SIL_KC;
  const int own0 = blockIdx.x * SIL_TILE;

  {                                                         // the owner tile: four threads per row
    const int r = tid >> 2;
    const int row = slot_row[own0 + r];
    const float* p = x + (int64_t)max(row, 0) * ld;
    for (int k = (tid & 3) * 4; k < E16; k += 16) {
      const bool ok = row >= 0 && k < E;
      const float4 v = *reinterpret_cast<const float4*>(p + (ok ? k : 0));
      *reinterpret_cast<float4*>(own + r * ldo + k) = sil_keep(ok, v);
    }
  }
  // this lane's owner row
  const int os = own0 + 16 * wave + i;
  const int own_row = slot_row[os];
  const float own_norm = slot_norm[os];
  const int4 own_meta = meta[os >> 4];
  const int own_c = own_meta.x, own_n = own_meta.z;
  const bool own_ok = own_row >= 0;

  // staging of the swept tile: thread -> rows lr and lr + 32 of the tile, columns lc .. lc + 3 of the chunk
  const int lr = tid >> 3, lc = (tid & 7) * 4;
  auto rows_of = [&](int mt, int (&rid)[2]) __attribute__((always_inline)) {
    const int m = min(mt, n_mt - 1);
    rid[0] = slot_row[m * SIL_TILE + lr];
    rid[1] = slot_row[m * SIL_TILE + 32 + lr];
  };
  auto issue = [&](int kc, const int (&rid)[2], float4 (&R)[2]) __attribute__((always_inline)) {   // unconditional loads from clamped addresses, then a select
    const int k = kc * SIL_KC + lc;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bool ok = rid[h] >= 0 && k < E;
      const float4 v = *reinterpret_cast<const float4*>(x + (int64_t)(ok ? rid[h] : 0) * ld + (ok ? k : 0));
      R[h] = sil_keep(ok, v);
    }
  };
  auto commit = [&](int buf, const float4 (&R)[2]) __attribute__((always_inline)) {
    float* b = swp + buf * (SIL_TILE * SIL_SWLD);
    *reinterpret_cast<float4*>(b + lr * SIL_SWLD + lc) = R[0];
    *reinterpret_cast<float4*>(b + (32 + lr) * SIL_SWLD + lc) = R[1];
  };

  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  double run = 0.0, a = 0.0, b = __builtin_inf();
  int cur_c = -1, cur_n = 1;                                // the cluster `run` belongs to (wave-uniform)
  auto flush = [&]() __attribute__((always_inline)) {
    double t = run + __shfl_xor(run, 16);
    t = t + __shfl_xor(t, 32);
    run = 0.0;
    if (cur_c == own_c) {
      a = own_n > 1 ? t / (double)(own_n - 1) : 0.0;
    } else {
      const double v = t / (double)cur_n;
      b = v < b ? v : b;
    }
  };

  int4 tmeta[4];                                            // of the swept tile being multiplied
  float4 tnorm[4];
  auto epilogue = [&](int mt) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = __builtin_amdgcn_readfirstlane(tmeta[j].x);
      if (c >= 0) {
        if (c != cur_c) {
          if (cur_c >= 0) flush();
          cur_c = c;
          cur_n = __builtin_amdgcn_readfirstlane(tmeta[j].z);
        }
        const int cnt = tmeta[j].y;
        const int ss0 = mt * SIL_TILE + 16 * j + 4 * q;     // this lane's four swept slots
        const float nj[4] = {tnorm[j].x, tnorm[j].y, tnorm[j].z, tnorm[j].w};
        double dd[4];
        unsigned nm = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float sum = own_norm + nj[r];
          const float d2 = fmaf(-2.f, acc[j][r], sum);
          const bool valid = own_ok && 4 * q + r < cnt && ss0 + r != os;
          const bool near = valid && d2 < SIL_NEAR * sum;
          dd[r] = (valid && !near) ? (double)sqrtf(fmaxf(d2, 0.f)) : 0.0;
          nm |= near ? (1u << r) : 0u;
        }
        // (pd_near_pairs written out: through the helper this kernel took 0.3 % longer at 65536 rows, outside its own spread)
        unsigned long long pend = __ballot(nm != 0);
        while (pend) {                                      // (wave-uniform) one lane's near pairs at a time, by the whole wave
          const int L = __ffsll((long long)pend) - 1;
          pend &= pend - 1;
          const unsigned m4 = (unsigned)__shfl((int)nm, L);
          const int ri = __shfl(own_row, L), sb = __shfl(ss0, L);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if ((m4 >> r) & 1u) {
              const double v = sil_pair(x, ld, E, ri, slot_row[sb + r], lane);
              if (lane == L) dd[r] = v;
            }
          }
        }
        run += dd[0];
        run += dd[1];
        run += dd[2];
        run += dd[3];
      }
      acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  };

  // Stage = (swept tile mt, chunk kc); a tile has nkc2 chunks, nkc rounded up to even (the odd one out is empty), so that the two
  // register sets and the two LDS buffers alternate statically inside a pair.  Entering body(kc): LDS buffer kc & 1 holds the
  // stage, Rn holds the next stage, Rf is free, rid_pend holds the rows of the stage after that, and (bo0, av0) hold the operand
  // fragments of the stage's first k-step.  The second k-step's fragments are read while the first is multiplied; then the next
  // stage is committed, and ITS first fragments are read while the second k-step is multiplied.
  const int nkc2 = (nkc + 1) & ~1;
  int mt2 = 0, kc2 = 0, mt3 = 0, kc3 = 0;                   // the stages two and three ahead
  auto advance = [&](int& m, int& k) __attribute__((always_inline)) {
    if (++k == nkc2) {
      k = 0;
      ++m;
    }
  };
  auto frag = [&](int buf, int kc, int ks, float4& bo, float4 (&av)[4]) __attribute__((always_inline)) {
    const int kk = min(kc * SIL_KC + ks * 16, E16 - 16);    // (an empty k-step reads a valid place and multiplies nothing)
    const float* sb = swp + buf * (SIL_TILE * SIL_SWLD);
    bo = *reinterpret_cast<const float4*>(own + (16 * wave + i) * ldo + kk + 4 * q);
#pragma unroll
    for (int j = 0; j < 4; ++j) av[j] = *reinterpret_cast<const float4*>(sb + (16 * j + i) * SIL_SWLD + ks * 16 + 4 * q);
  };
  auto mma = [&](const float4& bo, const float4 (&av)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = mfma16(av[j].x, bo.x, acc[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = mfma16(av[j].y, bo.y, acc[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = mfma16(av[j].z, bo.z, acc[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = mfma16(av[j].w, bo.w, acc[j]);
  };
  float4 R0[2], R1[2];
  int rid_pend[2];
  {
    int rid[2];
    rows_of(0, rid);
    issue(0, rid, R0);
    advance(mt2, kc2);                                      // -> stage 1
    rows_of(mt2, rid);
    issue(kc2, rid, R1);
    advance(mt2, kc2);                                      // -> stage 2
    rows_of(mt2, rid_pend);
    mt3 = mt2;
    kc3 = kc2;
    advance(mt3, kc3);                                      // -> stage 3
    commit(0, R0);
  }
  __syncthreads();
  float4 bo0, av0[4];
  frag(0, 0, 0, bo0, av0);

  auto body = [&](int kc, float4 (&Rf)[2], const float4 (&Rn)[2]) __attribute__((always_inline)) {
    const int rid_cur[2] = {rid_pend[0], rid_pend[1]};
    rows_of(mt3, rid_pend);
    issue(kc2, rid_cur, Rf);                                // two stages ahead (past the end: valid addresses, never used)
    float4 bo1, av1[4];
    frag(kc & 1, kc, 1, bo1, av1);
    if (kc * SIL_KC < E16) mma(bo0, av0);
    commit((kc + 1) & 1, Rn);
    lds_barrier();
    frag((kc + 1) & 1, kc + 1 == nkc2 ? 0 : kc + 1, 0, bo0, av0);
    if (kc * SIL_KC + 16 < E16) mma(bo1, av1);
    advance(mt2, kc2);
    advance(mt3, kc3);
  };
  for (int mt = 0; mt < n_mt; ++mt) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      tmeta[j] = meta[mt * 4 + j];
      tnorm[j] = *reinterpret_cast<const float4*>(slot_norm + mt * SIL_TILE + 16 * j + 4 * q);
    }
    for (int kc = 0; kc < nkc2; kc += 2) {
      body(kc, R0, R1);
      body(kc + 1, R1, R0);
    }
    epilogue(mt);
  }
  if (cur_c >= 0) flush();

  if (q == 0 && own_ok) {
    double s = 0.0;
    if (own_n > 1 && b < __builtin_inf()) {
      const double m = a > b ? a : b;
      s = m > 0.0 ? (b - a) / m : 0.0;
    }
    a_out[own_row] = a;
    b_out[own_row] = b;
    s_out[own_row] = s;
  }
}

__global__ __launch_bounds__(1024) void sil_finish_kernel(const double* __restrict__ s, int64_t N, int K,
                                                         const unsigned long long* __restrict__ hdr, int64_t* __restrict__ counts,
                                                         double* __restrict__ out) {
  __shared__ double sh[1024];
  double acc = 0.0;
  for (int64_t n = threadIdx.x; n < N; n += 1024) acc += s[n];
  const double tot = km_block_sum(acc, sh);
  if (threadIdx.x != 0) return;
  out[0] = tot;
  out[1] = (double)(K - (int)hdr[HD_EMPTY]);
  counts[K] = N - (int64_t)hdr[HD_VALID];
}

}  // namespace
}  // namespace g2v

using namespace g2v;

extern "C" size_t g2v_silhouette_workspace(int64_t N, int E, int K) {
  if (!sil_shape_ok(N, E, K) || E > SIL_MAX_E) return 0;
  return sil_layout(N, K).total;
}

extern "C" int g2v_silhouette_samples(const float* x, int64_t ld, const int64_t* labels, int64_t N, int E, int K, double* a, double* b,
                                      double* s, int64_t* counts, double* out, void* workspace, size_t workspace_bytes,
                                      g2v_stream_t stream) {
  G2V_REQUIRE(x && labels && a && b && s && counts && out && workspace, "null pointer");
  G2V_REQUIRE(N >= 2 && E > 0 && K > 0, "sizes: N >= 2, E >= 1, K >= 1");
  if ((E & 3) != 0 || E > SIL_MAX_E) {
    set_error("g2v_silhouette_samples: needs E %% 4 == 0 and E <= %d (E = %d)", SIL_MAX_E, E);
    return G2V_ERR_UNSUPPORTED;
  }
  if (!sil_shape_ok(N, E, K)) {
    set_error("g2v_silhouette_samples: needs N < 2^31 - 2048 and N + 16 K + 64 < 2^31");
    return G2V_ERR_UNSUPPORTED;
  }
  G2V_REQUIRE(ld >= E && (ld & 3) == 0, "row stride smaller than E or not a multiple of 4");
  G2V_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
              "x and workspace must be 16-byte aligned");
  const SilLayout l = sil_layout(N, K);
  if (workspace_bytes < l.total) {
    set_error("g2v_silhouette_samples: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  if (!g2v_internal_lds_reserve((const void*)sil_tile_kernel, sil_lds_bytes(E))) {
    set_error("g2v_silhouette_samples: cannot reserve LDS");
    return G2V_ERR_LAUNCH;
  }
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  unsigned long long* hdr = (unsigned long long*)(ws + l.hdr);
  int* hist = (int*)(ws + l.hist);
  int* cl_start = (int*)(ws + l.cl_start);
  int* sub_first = (int*)(ws + l.sub_first);
  int* sorted = (int*)(ws + l.sorted);
  int* slot_row = (int*)(ws + l.slot_row);
  float* slot_norm = (float*)(ws + l.slot_norm);
  int4* meta = (int4*)(ws + l.meta);
  const int use_lds = K <= KM_LDS_BINS ? 1 : 0;
  const double* gate = nullptr;

  (void)hipMemsetAsync(hdr, 0, HD_WORDS * sizeof(unsigned long long), st);
  if (!use_lds) (void)hipMemsetAsync(hist, 0, (size_t)l.nb * K * sizeof(int), st);
  (void)hipMemsetAsync(a, 0, (size_t)N * sizeof(double), st);          // rows with a label outside [0, K) keep zeros
  (void)hipMemsetAsync(b, 0, (size_t)N * sizeof(double), st);
  (void)hipMemsetAsync(s, 0, (size_t)N * sizeof(double), st);
  hipLaunchKernelGGL(km_hist_kernel, dim3(l.nb), dim3(256), 0, st, labels, (const int64_t*)nullptr, N, K, hist, hdr, use_lds, gate);
  hipLaunchKernelGGL(km_prefix_kernel, dim3(cdiv(K, 64)), dim3(1024), 0, st, hist, l.nb, K, counts, gate);
  hipLaunchKernelGGL(km_scan_kernel, dim3(1), dim3(1024), 0, st, K, SIL_SUB, (const int64_t*)counts, cl_start, sub_first, hdr, gate);
  int label_bits = 0;
  while (label_bits < 31 && ((int64_t)1 << label_bits) < K) ++label_bits;
  hipLaunchKernelGGL(km_scatter_kernel, dim3(l.nb), dim3(64), 0, st, labels, N, K, label_bits, hist, (const int*)cl_start, sorted,
                     use_lds, gate);
  hipLaunchKernelGGL(sil_slots_kernel, dim3(cdiv(l.slots, 256)), dim3(256), 0, st, x, ld, E, K, (int)l.slots, (const int*)sorted,
                     (const int*)cl_start, (const int*)sub_first, (const unsigned long long*)hdr, slot_row, slot_norm, meta);
  hipLaunchKernelGGL(sil_tile_kernel, dim3((int)(l.slots / SIL_TILE)), dim3(256), sil_lds_bytes(E), st, x, ld, E,
                     (const unsigned long long*)hdr, (const int*)slot_row, (const float*)slot_norm, (const int4*)meta, a, b, s);
  hipLaunchKernelGGL(sil_finish_kernel, dim3(1), dim3(1024), 0, st, (const double*)s, N, K, (const unsigned long long*)hdr, counts,
                     out);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
