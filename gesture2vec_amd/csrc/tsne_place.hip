// tsne_place.hip -- new rows into a fitted t-SNE map (gesture2vec_amd/embedding.py: TSNE.transform, LatentMap; the reference's
// make_unity_scatter(latents, labels, file, pca, MyTSNE) = MyTSNE.transform(pca.transform(latents)), Clustering.py:1318-1350).
// openTSNE's structure and transform defaults, stated exactly: X (N, d) the rows the map was fitted on, Y (N, 2)
// their map, Z (M, d) the new rows.  Every new row is its own problem and Y does not move.
//
// g2v_tsne_place_neighbors
//   pd_norm_kernel      |row|^2 in float64 over the d columns (pair_dist.hpp)
//   place_knn_kernel    one workgroup (4 waves) per 64 new rows, streaming over the 64-column tiles of the reference rows.  A tile of
//                       squared distances is formed by pd_tile (pair_dist.hpp), which tsne_dist_kernel calls too: the same bits as
//                       g2v_tsne_affinities gives for the same two rows.  The tile goes to LDS and never to memory.  Selection:
//                       wave w owns tile rows 16 w .. 16 w + 15 and their sorted lists of the kk best (d^2, index) in LDS.  Per row
//                       the 64 candidates of the tile sit one per lane; a ballot against the running kk-th best finds the few that
//                       enter, and each is inserted with the list in registers (slot s in lane s & 63): its place is a popcount,
//                       the shift one __shfl_up.  Tiles and lanes ascend, so a candidate's index is above every kept one and a tie
//                       goes to the lower index by construction.
//   place_refine_kernel the kk kept distances of a row once more, from differences in float64 (one wave per row), and the list
//                       sorted again.  The Gram form is good enough to SELECT (its error, ~3e-7 (|z|^2 + |x|^2), is far below the
//                       tolerance of the selection) but not to weigh: on rows centred like PCA scores it is ~20 fp32 roundings of
//                       the distance itself and moved the conditionals by 1.6e-5 of a row's largest (measured).
// g2v_tsne_place_conditionals
//   place_cond_kernel   one lane per row, 64 rows per workgroup, the first k_aff distances of each row in LDS: sklearn's bisection of
//                       the precision (tsne_cells.hpp, as tsne_search_kernel), without a term to leave out; the sums run over
//                       j ascending.
// g2v_tsne_place_init
//   place_init_kernel   one lane per row.  median: the k_use gathered coordinates in LDS, rank of each by counting (ties by
//                       position), numpy's rule for an even count; weighted: sum p Y in float64 over j ascending.
// g2v_tsne_place_descent
//   ALL n_iter iterations and the closing sweep run in one launch; y, velocity and gains live in registers.  dy and
//   w = 1 / (1 + |dy|^2) are fp32 (ts_q, tsne_cells.hpp); sum w and sum w^2 dy are float64, formed per BLOCK of 128
//   reference points over j ascending and the block sums added in ascending block order; the attraction over the row's k_aff
//   neighbours (gathered) is float64 over j ascending.  That order is fixed by N alone and both layouts keep it, so a row's bits
//   depend on that row, Y and the parameters only: not on M, the layout, the grid or the row's place in the batch.
//   place_descent_kernel      one lane per row, 64 rows per workgroup: Y goes through LDS 2048 points at a time and every lane reads
//                       the same point (a broadcast); no cross-lane reduction.  Its time is that of one row's N points x n_iter
//                       however few rows there are.
//   place_descent_row_kernel  one workgroup per row, for M <= 16384 rows (and 8 .. 512 blocks): thread t takes blocks t, t + 256, ..,
//                       three threads add the block sums in order while a fourth walks the neighbours, every thread takes the step.
// No floating-point atomics; the same input gives the same bits.  No environment variable is read.
#include <float.h>
#include <limits.h>

#include "common.hpp"
#include "km_sort.hpp"
#include "pair_dist.hpp"
#include "tsne_cells.hpp"

namespace g2v {
namespace {

constexpr int PL_MAX_D = 512;
constexpr int PL_MAX_KK = 128;
constexpr int64_t PL_MAX_N = (1 << 24) - 1;
constexpr int64_t PL_MAX_M = 2147483647LL;
constexpr int PL_YCH = 2048;                // points of Y per LDS stage of the descent
constexpr int PL_GRID = 1024;               // workgroups of the descent (4 per CU); row groups beyond are taken in turn
constexpr int PL_BLK = 128;                 // reference points per block: block sums are formed j ascending, then added b ascending
constexpr int PL_ROW_MAX_BLOCKS = 512;      // workgroup-per-row layout: block sums in LDS (N <= 65536) ..
constexpr int PL_ROW_MIN_BLOCKS = 8;        // .. enough blocks to occupy a few lanes ..
constexpr int64_t PL_ROW_MAX_M = 16384;     // .. and rows up to here: measured, DESIGN 3.5e (the lane layout takes the time of a full
                                            // grid however few rows there are: 86 ms per 50 iterations at N = 32768, where the row
                                            // layout takes 0.7 ms for 256 rows and 29 ms for 16384; 10.9 against 9.5 ms at N = 4096)
static_assert(PL_YCH % PL_BLK == 0, "a stage of Y holds whole blocks");

inline size_t place_norm_offset(int64_t N) { return km_align((size_t)N * sizeof(double)); }

// dynamic LDS: best_d[64][kk] float | best_i[64][kk] int.  waves_per_eu(4): the LDS lets four workgroups share a CU up to kk = 11,
// and the register allocator left alone lands a few registers either side of the 128 that allow them.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void place_knn_kernel(
    const float* __restrict__ X, int64_t ldx, int N, const float* __restrict__ Z, int64_t ldz, int64_t M, int d, int kk,
    const double* __restrict__ nx, const double* __restrict__ nz, int* __restrict__ idx_out, float* __restrict__ d2_out) {
  __shared__ __attribute__((aligned(16))) float sa[PD_TILE * PD_LD];
  __shared__ __attribute__((aligned(16))) float sb[PD_TILE * PD_LD];
  __shared__ float dt[PD_TILE][PD_TILE + 1];
  extern __shared__ __attribute__((aligned(16))) float best[];
  float* best_d = best;
  int* best_i = reinterpret_cast<int*>(best + PD_TILE * kk);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t i0 = (int64_t)blockIdx.x * PD_TILE;
  const float inf = __builtin_inff();

  for (int e = tid; e < PD_TILE * kk; e += 256) {
    best_d[e] = inf;
    best_i[e] = INT_MAX;
  }
  double nr[4];
  pd_row_norms(nz, M, i0, nr);
  for (int j0 = 0; j0 < N; j0 += PD_TILE) {
    // (pd_tile's first barrier: the lists are set, the previous tile has been selected from)
    pd_tile(Z, ldz, M, i0, nr, X, ldx, N, j0, nx, d, false, sa, sb, [&](int64_t row, int col, const float (&dd)[4]) {
#pragma unroll
      for (int r = 0; r < 4; ++r) dt[(int)(row - i0) + r][col - j0] = dd[r];
    });
    __syncthreads();

    // selection: this wave's 16 rows, the tile's 64 candidates one per lane
    for (int r = 0; r < 16; ++r) {
      const int row = 16 * wave + r;
      const float c = dt[row][lane];
      float* ld_ = best_d + row * kk;
      int* li_ = best_i + row * kk;
      float thr = ld_[kk - 1];
      unsigned long long cand = __ballot(c < thr);
      if (!cand) continue;
      float e0 = lane < kk ? ld_[lane] : inf, e1 = lane + 64 < kk ? ld_[lane + 64] : inf;
      int n0 = lane < kk ? li_[lane] : INT_MAX, n1 = lane + 64 < kk ? li_[lane + 64] : INT_MAX;
      while (cand) {
        const int L = __ffsll((long long)cand) - 1;
        cand &= cand - 1;
        const float cd = __shfl(c, L);
        if (!(cd < thr)) continue;                            // (uniform) the threshold has fallen since the ballot
        const int ci = j0 + L;
        // every kept index is below ci: the candidate goes behind the entries with d^2 <= its own
        const int pos = __popcll(__ballot(e0 <= cd)) + __popcll(__ballot(e1 <= cd));
        const float u0 = __shfl_up(e0, 1), u1 = __shfl_up(e1, 1), w0 = __shfl(e0, 63);
        const int v0 = __shfl_up(n0, 1), v1 = __shfl_up(n1, 1), x0 = __shfl(n0, 63);
        const int s0 = lane, s1 = lane + 64;
        e0 = s0 < pos ? e0 : (s0 == pos ? cd : u0);
        n0 = s0 < pos ? n0 : (s0 == pos ? ci : v0);
        e1 = s1 < pos ? e1 : (s1 == pos ? cd : (lane == 0 ? w0 : u1));
        n1 = s1 < pos ? n1 : (s1 == pos ? ci : (lane == 0 ? x0 : v1));
        thr = __shfl(kk - 1 < 64 ? e0 : e1, (kk - 1) & 63);
      }
      if (lane < kk) {
        ld_[lane] = e0;
        li_[lane] = n0;
      }
      if (lane + 64 < kk) {
        ld_[lane + 64] = e1;
        li_[lane + 64] = n1;
      }
    }
  }

  for (int r = 0; r < 16; ++r) {                              // (the wave's own lists: no barrier)
    const int row = 16 * wave + r;
    if (i0 + row >= M) break;
    for (int s = lane; s < kk; s += 64) {
      const int id = best_i[row * kk + s];                    // (a list is short of kk entries only where distances are NaN)
      idx_out[(i0 + row) * kk + s] = id == INT_MAX ? 0 : id;
      d2_out[(i0 + row) * kk + s] = best_d[row * kk + s];
    }
  }
}

// One wave per new row: the kk kept distances again, as sum (z - x)^2 in float64 rounded to fp32 once, then the list in ascending
// (d^2, index) order again (rank by counting; slot s in lane s & 63).  In place: every read of the row precedes its writes.
__global__ __launch_bounds__(256) void place_refine_kernel(const float* __restrict__ X, int64_t ldx, int N, const float* __restrict__ Z,
                                                          int64_t ldz, int64_t M, int d, int kk, int* __restrict__ idx,
                                                          float* __restrict__ d2) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;                                       // (wave-uniform; no barrier follows)
  int* ir = idx + row * kk;
  float* dr = d2 + row * kk;
  const float* zr = Z + row * ldz;
  const int n0 = lane < kk ? ir[lane] : INT_MAX, n1 = lane + 64 < kk ? ir[lane + 64] : INT_MAX;
  float e0 = __builtin_inff(), e1 = __builtin_inff();
  for (int s = 0; s < kk; ++s) {
    const int id = __shfl(s < 64 ? n0 : n1, s & 63);
    const float v = (float)pd_pair_sq(zr, X + (int64_t)id * ldx, d, lane);
    if (s == lane) e0 = v;
    if (s == lane + 64) e1 = v;
  }
  int r0 = 0, r1 = 0;
  for (int s = 0; s < kk; ++s) {
    const float es = __shfl(s < 64 ? e0 : e1, s & 63);
    const int ns = __shfl(s < 64 ? n0 : n1, s & 63);
    r0 += (es < e0 || (es == e0 && ns < n0)) ? 1 : 0;
    r1 += (es < e1 || (es == e1 && ns < n1)) ? 1 : 0;
  }
  if (lane < kk) {
    ir[r0] = n0;
    dr[r0] = e0;
  }
  if (lane + 64 < kk) {
    ir[r1] = n1;
    dr[r1] = e1;
  }
}

// LDS: the first k_aff distances of 64 rows, [j][lane]
__global__ __launch_bounds__(64) void place_cond_kernel(const float* __restrict__ d2, int64_t M, int kk, int k_aff, double log_perp,
                                                       float* __restrict__ p) {
  __shared__ float ds[PL_MAX_KK][64];
  const int lane = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  for (int e = lane; e < 64 * kk; e += 64) {                  // 64 rows of kk floats are one run of memory
    const int r = e / kk, j = e - r * kk;
    if (j < k_aff) ds[j][r] = r0 + r < M ? d2[r0 * kk + e] : 0.f;
  }
  __syncthreads();
  const int64_t row = r0 + lane;
  if (row >= M) return;
  TsBisect bs;
  for (int step = 0; step < TS_BISECT_STEPS; ++step) {
    double s0 = 0.0, s1 = 0.0;
    for (int j = 0; j < k_aff; ++j) {
      const double dj = (double)ds[j][lane];
      const double e = exp(-dj * bs.beta);
      s0 += e;
      s1 = fma(dj, e, s1);
    }
    if (ts_bisect_next(bs, s0, s1, log_perp)) break;
  }
  for (int j = 0; j < k_aff; ++j) p[row * k_aff + j] = (float)(exp(-(double)ds[j][lane] * bs.beta_eval) / bs.sum_p);
}

__device__ __forceinline__ int pl_ref_index(int id, int N) { return (unsigned)id < (unsigned)N ? id : 0; }

// LDS: one coordinate of the k_use neighbours of 64 rows, [j][lane]
__global__ __launch_bounds__(64) void place_init_kernel(const float* __restrict__ Y, int N, const int* __restrict__ idx,
                                                       const float* __restrict__ p, int64_t M, int kk, int k_aff, int mode, int k_use,
                                                       float* __restrict__ y) {
  __shared__ float vs[PL_MAX_KK][64];
  const int lane = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x * 64 + lane;
  if (row >= M) return;
  const int* ir = idx + row * kk;
  if (mode == 1) {
    double ax = 0.0, ay = 0.0;
    for (int j = 0; j < k_use; ++j) {
      const int id = pl_ref_index(ir[j], N);
      const double pj = (double)p[row * k_aff + j];
      ax = fma(pj, (double)Y[2 * id], ax);
      ay = fma(pj, (double)Y[2 * id + 1], ay);
    }
    y[2 * row] = (float)ax;
    y[2 * row + 1] = (float)ay;
    return;
  }
  const int lo = (k_use - 1) >> 1, hi = k_use >> 1;           // the two middle ranks (the same for an odd count)
  for (int c = 0; c < 2; ++c) {
    for (int j = 0; j < k_use; ++j) vs[j][lane] = Y[2 * pl_ref_index(ir[j], N) + c];
    float a = 0.f, b = 0.f;
    for (int j = 0; j < k_use; ++j) {
      const float v = vs[j][lane];
      int rank = 0;
      for (int l = 0; l < k_use; ++l) {
        const float u = vs[l][lane];
        rank += (u < v || (u == v && l < j)) ? 1 : 0;
      }
      if (rank == lo) a = v;
      if (rank == hi) b = v;
    }
    y[2 * row + c] = lo == hi ? a : __fmul_rn(__fadd_rn(a, b), 0.5f);
  }
}

// ---- the descent.  Both layouts call the same pieces, with every product-and-sum written as an explicit fma, so that a row ends
// with the same bits whichever of them ran it.
// one reference point: sum w^2 (y - Y_j) and sum w of a block, in float64
__device__ __forceinline__ void pl_pair(const float2 yi, const float2 yj, double& bx, double& by, double& bz) {
  const float dx = yi.x - yj.x, dy = yi.y - yj.y;
  const float w = ts_q(dx, dy);
  const double wd = (double)w, wr = wd * wd;
  bx = fma(wr, (double)dx, bx);
  by = fma(wr, (double)dy, by);
  bz += wd;
}

// the row's k_aff neighbours, j ascending: a = { sum p w (y - Y_j) (x, y), sum p (log p - log w), sum p }, the last two with want_kl
__device__ __forceinline__ void pl_attract(const float2* __restrict__ Y, int N, const int* __restrict__ ir, const float* __restrict__ pr,
                                           int k_aff, const float2 yi, bool want_kl, double (&a)[4]) {
  a[0] = a[1] = a[2] = a[3] = 0.0;
  for (int j = 0; j < k_aff; ++j) {
    const float2 yj = Y[pl_ref_index(ir[j], N)];
    const float dx = yi.x - yj.x, dy = yi.y - yj.y;
    const float w = ts_q(dx, dy);
    const double pd = (double)pr[j], wd = (double)w, pw = pd * wd;
    a[0] = fma(pw, (double)dx, a[0]);
    a[1] = fma(pw, (double)dy, a[1]);
    if (want_kl && pd > 0.0) {
      a[2] = fma(pd, log(pd) - log(wd), a[2]);
      a[3] += pd;
    }
  }
}

__device__ __forceinline__ float2 pl_gradient(double ex, const double (&a)[4], double rx, double ry, double z) {
  return make_float2((float)(2.0 * fma(ex, a[0], -(rx / z))), (float)(2.0 * fma(ex, a[1], -(ry / z))));
}

__device__ __forceinline__ double pl_kl(const double (&a)[4], double z) { return fma(log(z), a[3], a[2]); }

// one step, fp32, no contraction: clip by the norm, then ts_step per component
__device__ __forceinline__ void pl_step(float2 g, float momentum, float lr, float max_gnorm, float2& yi, float2& v, float2& gn) {
  const float n = __fsqrt_rn(__fadd_rn(__fmul_rn(g.x, g.x), __fmul_rn(g.y, g.y)));
  if (max_gnorm > 0.f && n > max_gnorm) {
    const float s = __fdiv_rn(max_gnorm, n);
    g.x = __fmul_rn(g.x, s);
    g.y = __fmul_rn(g.y, s);
  }
  ts_step(g.x, momentum, lr, yi.x, v.x, gn.x);
  ts_step(g.y, momentum, lr, yi.y, v.y, gn.y);
}

// one lane per row
__global__ __launch_bounds__(64) void place_descent_kernel(const float2* __restrict__ Y, int N, const int* __restrict__ idx,
                                                          const float* __restrict__ p, int64_t M, int kk, int k_aff,
                                                          float2* __restrict__ y, float2* __restrict__ vel, float2* __restrict__ gains,
                                                          int n_iter, double exag, float momentum, float lr, float max_gnorm,
                                                          double* __restrict__ kl, double* __restrict__ zsum,
                                                          float2* __restrict__ grad) {
  __shared__ __attribute__((aligned(16))) float2 ys[PL_YCH];
  const int lane = threadIdx.x;
  const int64_t groups = (M + 63) >> 6;
  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t row = g * 64 + lane;
    const bool live = row < M;
    const int64_t rc = live ? row : M - 1;                    // (a lane past the end walks row M - 1 and writes nothing)
    float2 yi = y[rc], v = make_float2(0.f, 0.f), gn = make_float2(1.f, 1.f);
    if (n_iter > 0) {
      v = vel[rc];
      gn = gains[rc];
    }
    for (int it = 0; it <= n_iter; ++it) {
      const bool last = it == n_iter;                         // the closing sweep: outputs only
      double rx = 0.0, ry = 0.0, z = 0.0;
      for (int c0 = 0; c0 < N; c0 += PL_YCH) {
        __syncthreads();
        for (int c = lane; c < PL_YCH; c += 64)
          if (c0 + c < N) ys[c] = Y[c0 + c];
        __syncthreads();
        const int cend = min(PL_YCH, N - c0);
        for (int b0 = 0; b0 < cend; b0 += PL_BLK) {           // (PL_YCH % PL_BLK == 0: these are the blocks of the other layout)
          double bx = 0.0, by = 0.0, bz = 0.0;
          const int be = min(cend, b0 + PL_BLK);
#pragma unroll 8
          for (int c = b0; c < be; ++c) pl_pair(yi, ys[c], bx, by, bz);
          rx += bx;
          ry += by;
          z += bz;
        }
      }
      double a[4];
      pl_attract(Y, N, idx + rc * kk, p + rc * k_aff, k_aff, yi, last, a);
      const float2 gr = pl_gradient((last && n_iter > 0) ? 1.0 : exag, a, rx, ry, z);   // (n_iter == 0: the gradient asked for)
      if (last) {
        if (live) {
          if (kl) kl[row] = pl_kl(a, z);
          if (zsum) zsum[row] = z;
          if (grad) grad[row] = gr;
        }
        break;
      }
      pl_step(gr, momentum, lr, max_gnorm, yi, v, gn);
    }
    if (live && n_iter > 0) {
      y[row] = yi;
      vel[row] = v;
      gains[row] = gn;
    }
  }
}

// one workgroup per row, for few rows against many points: thread t takes the blocks t, t + 256, .. of PL_BLK points (read from
// memory: Y stays in L2), three threads add the block sums in ascending block order while a fourth walks the neighbours, and every
// thread then takes the same step on its own copy of the state.
__global__ __launch_bounds__(256) void place_descent_row_kernel(const float2* __restrict__ Y, int N, const int* __restrict__ idx,
                                                               const float* __restrict__ p, int kk, int k_aff, float2* __restrict__ y,
                                                               float2* __restrict__ vel, float2* __restrict__ gains, int n_iter,
                                                               double exag, float momentum, float lr, float max_gnorm,
                                                               double* __restrict__ kl, double* __restrict__ zsum,
                                                               float2* __restrict__ grad) {
  __shared__ double ps[3][PL_ROW_MAX_BLOCKS];
  __shared__ double tot[8];                                   // sum w^2 dy (x, y), sum w, then pl_attract's four
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int nb = (N + PL_BLK - 1) / PL_BLK;
  float2 yi = y[row], v = make_float2(0.f, 0.f), gn = make_float2(1.f, 1.f);
  if (n_iter > 0) {
    v = vel[row];
    gn = gains[row];
  }
  for (int it = 0; it <= n_iter; ++it) {
    const bool last = it == n_iter;
    for (int b = tid; b < nb; b += 256) {
      double bx = 0.0, by = 0.0, bz = 0.0;
      const int be = min(N, (b + 1) * PL_BLK);
#pragma unroll 8
      for (int c = b * PL_BLK; c < be; ++c) pl_pair(yi, Y[c], bx, by, bz);
      ps[0][b] = bx;
      ps[1][b] = by;
      ps[2][b] = bz;
    }
    __syncthreads();
    if (tid == 0 || tid == 64 || tid == 128) {                // (one lane of three waves)
      const double* q = ps[tid >> 6];
      double acc = 0.0;
      for (int b = 0; b < nb; ++b) acc += q[b];
      tot[tid >> 6] = acc;
    } else if (tid == 192) {
      double a[4];
      pl_attract(Y, N, idx + row * kk, p + row * k_aff, k_aff, yi, last, a);
#pragma unroll
      for (int k = 0; k < 4; ++k) tot[3 + k] = a[k];
    }
    __syncthreads();                                          // (tot is written again only behind the next barrier)
    const double a[4] = {tot[3], tot[4], tot[5], tot[6]};
    const double z = tot[2];
    const float2 gr = pl_gradient((last && n_iter > 0) ? 1.0 : exag, a, tot[0], tot[1], z);
    if (last) {
      if (tid == 0) {
        if (kl) kl[row] = pl_kl(a, z);
        if (zsum) zsum[row] = z;
        if (grad) grad[row] = gr;
      }
      break;
    }
    pl_step(gr, momentum, lr, max_gnorm, yi, v, gn);
  }
  if (tid == 0 && n_iter > 0) {
    y[row] = yi;
    vel[row] = v;
    gains[row] = gn;
  }
}

inline bool place_shape_ok(int64_t N, int64_t M, int kk) {
  return N >= 1 && N <= PL_MAX_N && M >= 1 && M <= PL_MAX_M && kk >= 1 && kk <= PL_MAX_KK && kk <= N;
}

}  // namespace
}  // namespace g2v

using namespace g2v;

extern "C" size_t g2v_tsne_place_neighbors_workspace(int64_t N, int64_t M, int d, int kk) {
  if (!place_shape_ok(N, M, kk) || d < 1 || d > PL_MAX_D) return 0;
  return place_norm_offset(N) + km_align((size_t)M * sizeof(double));
}

extern "C" int g2v_tsne_place_neighbors(const float* X, int64_t ldx, int64_t N, const float* Z, int64_t ldz, int64_t M, int d, int kk,
                                        int32_t* idx, float* d2, void* workspace, size_t workspace_bytes, g2v_stream_t stream) {
  G2V_REQUIRE(X && Z && idx && d2 && workspace, "null pointer");
  if (!place_shape_ok(N, M, kk) || d < 1 || d > PL_MAX_D || (ldx & 3) || (ldz & 3)) {
    set_error("g2v_tsne_place_neighbors: needs 1 <= d <= %d, ldx %% 4 == ldz %% 4 == 0, 1 <= kk <= min(N, %d), N < 2^24, "
              "M < 2^31 (N = %lld, M = %lld, d = %d, kk = %d)", PL_MAX_D, PL_MAX_KK, (long long)N, (long long)M, d, kk);
    return G2V_ERR_UNSUPPORTED;
  }
  G2V_REQUIRE(ldx >= d && ldz >= d, "row stride smaller than d");
  G2V_REQUIRE(((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Z) | reinterpret_cast<uintptr_t>(workspace)) & 15) == 0,
              "X, Z and workspace must be 16-byte aligned");
  if (workspace_bytes < g2v_tsne_place_neighbors_workspace(N, M, d, kk)) {
    set_error("g2v_tsne_place_neighbors: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  if (!g2v_internal_lds_reserve((const void*)place_knn_kernel, (size_t)PD_TILE * kk * 8)) {
    set_error("g2v_tsne_place_neighbors: cannot reserve LDS");
    return G2V_ERR_LAUNCH;
  }
  hipStream_t st = (hipStream_t)stream;
  double* nx = (double*)workspace;
  double* nz = (double*)((char*)workspace + place_norm_offset(N));
  hipLaunchKernelGGL(pd_norm_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, X, ldx, N, d, nx);
  hipLaunchKernelGGL(pd_norm_kernel, dim3(cdiv(M, 256)), dim3(256), 0, st, Z, ldz, M, d, nz);
  hipLaunchKernelGGL(place_knn_kernel, dim3(cdiv(M, PD_TILE)), dim3(256), (size_t)PD_TILE * kk * 8, st, X, ldx, (int)N, Z, ldz, M, d,
                     kk, (const double*)nx, (const double*)nz, idx, d2);
  hipLaunchKernelGGL(place_refine_kernel, dim3(cdiv(M, 4)), dim3(256), 0, st, X, ldx, (int)N, Z, ldz, M, d, kk, idx, d2);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int g2v_tsne_place_conditionals(const float* d2, int64_t M, int kk, int k_aff, double perplexity, float* p,
                                           g2v_stream_t stream) {
  G2V_REQUIRE(d2 && p, "null pointer");
  G2V_REQUIRE(M >= 1 && M <= PL_MAX_M && kk >= 1 && kk <= PL_MAX_KK && k_aff >= 1 && k_aff <= kk,
              "sizes: 1 <= M < 2^31, 1 <= k_aff <= kk <= 128");
  G2V_REQUIRE(perplexity > 0.0 && perplexity < (double)k_aff, "perplexity must be in (0, k_aff)");
  hipLaunchKernelGGL(place_cond_kernel, dim3(cdiv(M, 64)), dim3(64), 0, (hipStream_t)stream, d2, M, kk, k_aff, log(perplexity), p);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int g2v_tsne_place_init(const float* Y, int64_t N, const int32_t* idx, const float* p, int64_t M, int kk, int k_aff,
                                   int mode, int k_use, float* y, g2v_stream_t stream) {
  G2V_REQUIRE(Y && idx && y, "null pointer");
  G2V_REQUIRE(mode == 0 || mode == 1, "mode: 0 (median) or 1 (weighted)");
  G2V_REQUIRE(N >= 1 && N <= PL_MAX_N && M >= 1 && M <= PL_MAX_M && kk >= 1 && kk <= PL_MAX_KK,
              "sizes: 1 <= N < 2^24, 1 <= M < 2^31, 1 <= kk <= 128");
  if (mode == 1)
    G2V_REQUIRE(p && k_aff >= 1 && k_aff <= kk && k_use >= 1 && k_use <= k_aff, "weighted start: p and 1 <= k_use <= k_aff <= kk");
  else
    G2V_REQUIRE(k_use >= 1 && k_use <= kk, "median start: 1 <= k_use <= kk");
  hipLaunchKernelGGL(place_init_kernel, dim3(cdiv(M, 64)), dim3(64), 0, (hipStream_t)stream, Y, (int)N, idx, p, M, kk, k_aff, mode,
                     k_use, y);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int g2v_tsne_place_descent(const float* Y, int64_t N, const int32_t* idx, const float* p, int64_t M, int kk, int k_aff,
                                      float* y, float* velocity, float* gains, int n_iter, double exaggeration, float momentum,
                                      float learning_rate, float max_grad_norm, double* kl, double* zsum, float* grad,
                                      g2v_stream_t stream) {
  G2V_REQUIRE(Y && idx && p && y, "null pointer");
  G2V_REQUIRE(n_iter >= 0 && (n_iter == 0 || (velocity && gains)), "n_iter >= 0; velocity and gains are needed when it is positive");
  G2V_REQUIRE(N >= 1 && N <= PL_MAX_N && M >= 1 && M <= PL_MAX_M && kk >= 1 && kk <= PL_MAX_KK && k_aff >= 1 && k_aff <= kk,
              "sizes: 1 <= N < 2^24, 1 <= M < 2^31, 1 <= k_aff <= kk <= 128");
  G2V_REQUIRE(exaggeration > 0.0, "exaggeration must be positive");
  G2V_REQUIRE(((reinterpret_cast<uintptr_t>(Y) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(velocity) |
                reinterpret_cast<uintptr_t>(gains) | reinterpret_cast<uintptr_t>(grad)) & 7) == 0,
              "Y, y, velocity, gains and grad must be 8-byte aligned");
  const int64_t groups = (M + 63) / 64, nb = (N + PL_BLK - 1) / PL_BLK;
  if (M <= PL_ROW_MAX_M && nb >= PL_ROW_MIN_BLOCKS && nb <= PL_ROW_MAX_BLOCKS) {
    hipLaunchKernelGGL(place_descent_row_kernel, dim3((int)M), dim3(256), 0, (hipStream_t)stream, (const float2*)Y, (int)N, idx, p,
                       kk, k_aff, (float2*)y, (float2*)velocity, (float2*)gains, n_iter, exaggeration, momentum, learning_rate,
                       max_grad_norm, kl, zsum, (float2*)grad);
    G2V_CHECK_LAUNCH();
    return G2V_OK;
  }
  hipLaunchKernelGGL(place_descent_kernel, dim3((int)(groups < PL_GRID ? groups : PL_GRID)), dim3(64), 0, (hipStream_t)stream,
                     (const float2*)Y, (int)N, idx, p, M, kk, k_aff, (float2*)y, (float2*)velocity, (float2*)gains, n_iter,
                     exaggeration, momentum, learning_rate, max_grad_norm, kl, zsum, (float2*)grad);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
