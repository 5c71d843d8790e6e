// metrics.hip -- device-side evaluation statistics (gesture2vec_amd/metrics.py; the reference's Clustering.Metrics_analysis):
//   g2v_moments_accumulate   shifted first and second moments of an (N, E) latent matrix, added to float64 accumulators
//   g2v_code_histogram       exact int64 histogram of code ids
//
// ---- moments ----------------------------------------------------------------------------------------------------------------------
//   S1 += sum_n (x_n - shift),   S2 += sum_n (x_n - shift)(x_n - shift)^T      (S2 is stored FULL: the upper triangle is computed
//   and mirrored into the lower, so s2[i][j] == s2[j][i] bit for bit)
//
//   moments_slab_kernel   one workgroup (4 waves, one per SIMD) per SLAB of R consecutive rows.  The columns are cut into
//                         ET = ceil(E / 16) tiles; the ET (ET + 1) / 2 unordered tile pairs are enumerated by wrapped diagonals,
//                         p = d ET + ti  <->  (ti, tj = (ti + d) mod ET), d = 0 .. ET / 2, and dealt to the four waves in contiguous
//                         runs.  A wave keeps one 16 x 16 fp32 accumulator per pair in registers (82 pairs = 328 registers at
//                         E = 400) and feeds v_mfma_f32_16x16x4_f32 from a 32-row tile of x - shift in LDS, double-buffered:
//                         the next tile's global loads are issued before the products of the current one and written to the other
//                         buffer after them.  x is read ONCE for E <= 400; 401 <= E <= 512 has 351 .. 528 pairs, more than four
//                         waves hold, and runs two workgroups per slab (each half of the pairs, each reading the slab).
//                         LDS image: 8 planes of 4 rows, [plane][column][4 rows] (16 B per column, no padding): lane (i, q) of a
//                         pair takes rows 4q .. 4q+3 and 16+4q .. 16+4q+3 of columns 16 ti + i and 16 tj + i with four
//                         ds_read_b128 (the 16 lanes of a bank group read 16 consecutive 16-byte slots: conflict-free) and
//                         contracts them in 8 MFMAs: which rows meet in which k-step is free as long as both operands agree.
//                         Column sums come from the same image.  Everything a workgroup accumulated is written, fp32, to its own
//                         slice of the workspace: no atomics.
//   moments_fold_kernel   sums the slabs' partials in slab order in float64 and adds them to s1 / s2 (both triangles).
// The fp32 chains are R rows long (one fma per row and output).  R = ceil(rows / 256) rounded up to 32 and clamped to [64, 1024]:
// enough slabs to fill the chip as soon as there are rows for it, never more than 1024 rows between two float64 folds; calls with
// more than 256 x 1024 rows are processed in pieces of that many rows (one launch pair each), which bounds the workspace.
// The result depends on (N, E, ld) and the data only: two runs give the same bits.
#include "common.hpp"

#include <type_traits>

namespace g2v {
namespace {

constexpr int MO_MAX_E = 512;
constexpr int MO_TILE_ROWS = 32;            // rows per LDS tile: 8 planes of 4
constexpr int MO_MAX_SLABS = 256;           // slabs per launch
constexpr int MO_MAX_R = 1024;              // rows per slab: the longest fp32 chain
constexpr int MO_MIN_R = 64;
constexpr int64_t MO_PIECE = (int64_t)MO_MAX_SLABS * MO_MAX_R;

struct MoGeom {
  int ET, Ep, P, groups, per_group, tpw;    // column tiles, padded width, tile pairs, workgroups per slab, pairs per group, template
};

inline MoGeom mo_geom(int E) {
  MoGeom g;
  g.ET = (E + 15) / 16;
  g.Ep = 16 * g.ET;
  g.P = g.ET * (g.ET + 1) / 2;
  g.groups = g.P > 4 * 82 ? 2 : 1;
  g.per_group = (g.P + g.groups - 1) / g.groups;
  const int per_wave = (g.per_group + 3) / 4;
  g.tpw = 82;
  for (int t : {66, 40, 20, 10, 4})
    if (per_wave <= t) g.tpw = t;
  return g;
}

inline int mo_slab_rows(int64_t n) {
  int64_t r = (n + MO_MAX_SLABS - 1) / MO_MAX_SLABS;
  r = (r + MO_TILE_ROWS - 1) / MO_TILE_ROWS * MO_TILE_ROWS;
  return (int)(r < MO_MIN_R ? MO_MIN_R : r > MO_MAX_R ? MO_MAX_R : r);
}

inline size_t mo_slab_floats(const MoGeom& g) { return (size_t)g.P * 256 + g.Ep; }

// f(integral_constant<int, U>) for U = BEGIN, BEGIN + STEP, ... < END, expanded at compile time: the accumulators are indexed by U and
// must stay in registers (a loop the optimizer declines to unroll would put them in scratch memory)
template <int U, int END, int STEP, class F>
__device__ __forceinline__ void mo_static_for(F&& f) {
  if constexpr (U < END) {
    f(std::integral_constant<int, U>{});
    mo_static_for<U + STEP, END, STEP>(f);
  }
}

// LDS: [2 buffers][8 planes][Ep columns][4 rows] | shift[Ep]
template <int TPW, bool VEC>
__global__ __launch_bounds__(256, 1) void moments_slab_kernel(const float* __restrict__ x, int64_t ld, const float* __restrict__ shift,
                                                             float* __restrict__ part, int64_t n_rows, int R, int E, int ET, int P,
                                                             int per_group) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Ep = 16 * ET, E4 = Ep / 4;
  const int plane = Ep * 4;                               // floats per plane
  const int buf_floats = 8 * plane;
  float* sh = smem + 2 * buf_floats;
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ngroups = gridDim.y, group = blockIdx.y, slab = blockIdx.x;
  const int64_t row0 = (int64_t)slab * R;
  const int rows = (int)min((int64_t)R, n_rows - row0);
  const int ntiles = (rows + MO_TILE_ROWS - 1) / MO_TILE_ROWS;
  (void)ngroups;

  // this wave's run of pairs [p0, p0 + np)
  const int g0 = group * per_group, gcnt = min(per_group, P - g0);
  const int per_wave = (gcnt + 3) / 4;
  const int p0 = g0 + wave * per_wave;
  const int np = max(0, min(per_wave, g0 + gcnt - p0));
  const int pc = min(p0, P - 1);                          // (a wave without pairs multiplies the last one, and stores nothing)
  const int d0 = pc / ET, ti0 = pc - d0 * ET, tj0 = ti0 + d0 - (ti0 + d0 >= ET ? ET : 0);

  for (int c = tid; c < Ep; c += 256) sh[c] = c < E ? shift[c] : 0.f;

  // staging items: (plane, 4 columns) pairs, 8 * E4 of them, item f = 256 n + tid; an item is 4 rows x 4 columns
  const int nitems = 8 * E4;
  int it_row[4], it_col[4];                               // first row inside the tile, first column; -1: no item
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int f = 256 * n + tid;
    if (f < nitems) {
      const int pl = f / E4;
      it_row[n] = 4 * pl;
      it_col[n] = 4 * (f - pl * E4);
    } else {
      it_row[n] = -1;
      it_col[n] = 0;
    }
  }
  float4 pre[2][4];                                       // [item of the half in flight][row]: raw x values
  // The next tile is staged in two halves (items 0, 1 / items 2, 3): 32 registers in flight instead of 64.  The loads are
  // unconditional: a row past the slab reads the slab's last row, a thread without an item reads item 0's place, a column group
  // past E reads column 0 -- commit() writes zeros for those.
  auto issue = [&](int t, int h) {
    const int64_t tr0 = row0 + (int64_t)t * MO_TILE_ROWS;
    const float* tb = x + tr0 * ld;                       // (wave-uniform)
    const int last = (int)(row0 + rows - tr0) - 1;        // last row of the slab, counted from this tile's first
#pragma unroll
    for (int nn = 0; nn < 2; ++nn) {
      const int n = 2 * h + nn;
      const int rr = max(it_row[n], 0);
      const int c = VEC ? (it_col[n] < E ? it_col[n] : 0) : it_col[n];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* p = tb + (min(rr + r, last) * (int)ld + c);
        if (VEC) {
          pre[nn][r] = *reinterpret_cast<const float4*>(p);
        } else {                                          // any E, any alignment: element loads, the row's tail clamped
          const int e1 = E - 1 - c;                       // (>= 0 for an item that has a column inside E; others are discarded)
          pre[nn][r] = make_float4(p[min(0, e1)], p[min(1, e1)], p[min(2, e1)], p[min(3, e1)]);
        }
      }
    }
  };
  // rows past the slab and columns past E become exact zeros (x - shift is not formed there)
  auto commit = [&](int t, float* buf, int h) {
    const int left = rows - t * MO_TILE_ROWS;
#pragma unroll
    for (int nn = 0; nn < 2; ++nn) {
      const int n = 2 * h + nn;
      if (it_row[n] < 0) continue;
      const int c = it_col[n];
      const float4 s = *reinterpret_cast<const float4*>(sh + c);
      bool m[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) m[r] = it_row[n] + r < left;
      float* dst = buf + (it_row[n] >> 2) * plane + c * 4;
      const float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {                       // column c + j: its four rows, 16 bytes
        const float v[4] = {j == 0 ? pre[nn][0].x : j == 1 ? pre[nn][0].y : j == 2 ? pre[nn][0].z : pre[nn][0].w,
                            j == 0 ? pre[nn][1].x : j == 1 ? pre[nn][1].y : j == 2 ? pre[nn][1].z : pre[nn][1].w,
                            j == 0 ? pre[nn][2].x : j == 1 ? pre[nn][2].y : j == 2 ? pre[nn][2].z : pre[nn][2].w,
                            j == 0 ? pre[nn][3].x : j == 1 ? pre[nn][3].y : j == 2 ? pre[nn][3].z : pre[nn][3].w};
        const bool cok = c + j < E;
        *reinterpret_cast<float4*>(dst + 4 * j) =
            make_float4(cok && m[0] ? v[0] - sv[j] : 0.f, cok && m[1] ? v[1] - sv[j] : 0.f, cok && m[2] ? v[2] - sv[j] : 0.f,
                        cok && m[3] ? v[3] - sv[j] : 0.f);
      }
    }
  };

  f32x4 acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float s1a[2] = {0.f, 0.f};                              // column sums of columns tid and tid + 256 (group 0 only)

  __syncthreads();                                        // shift staged
  issue(0, 0);
  commit(0, smem, 0);
  issue(0, 1);
  commit(0, smem, 1);
  __syncthreads();

  const int lane_off = q * plane + i * 4;                 // lane (i, q): plane q (and 4 + q), column i of a tile
  constexpr int UH = (TPW / 4) * 2;
  for (int t = 0; t < ntiles; ++t) {
    const float* buf = smem + (t & 1) * buf_floats;
    const bool more = t + 1 < ntiles;
    float* nbuf = smem + ((t + 1) & 1) * buf_floats;
    if (more) issue(t + 1, 0);
    if (group == 0) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int c = tid + 256 * k;
        if (c < Ep) {
          float s = 0.f;
#pragma unroll
          for (int pl = 0; pl < 8; ++pl) {
            const float4 v = *reinterpret_cast<const float4*>(buf + pl * plane + c * 4);
            s += (v.x + v.y) + (v.z + v.w);
          }
          s1a[k] += s;
        }
      }
    }
    int ti = ti0, tj = tj0;                               // the next pair to LOAD
    asm volatile("" : "+s"(ti), "+s"(tj));                // recompute the pairs' addresses per tile (scalar, cheap): hoisted, they spill
    // Operands of a block of two pairs: {a, a', b, b'} x 2 (' = rows 16 ..), two sets: the block after the one being multiplied
    // is read while it runs.  Every wave multiplies TPW pairs with NO branch around the MFMAs (branches make the compiler
    // shuttle the accumulators between register files and spill): past its run a wave walks on through (valid) pairs into
    // accumulators that are never stored.  sched_barrier keeps the compiler from pulling later blocks' reads further up.
    // Along a diagonal both tile indices step by one (tj wraps at ET); a new diagonal starts at ti = 0 with tj one further.
    float4 op[2][8];
    auto load_block = [&](float4* o) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const float* pa = buf + lane_off + ti * 64;
        const float* pb = buf + lane_off + tj * 64;
        o[4 * k + 0] = *reinterpret_cast<const float4*>(pa);
        o[4 * k + 1] = *reinterpret_cast<const float4*>(pa + 4 * plane);
        o[4 * k + 2] = *reinterpret_cast<const float4*>(pb);
        o[4 * k + 3] = *reinterpret_cast<const float4*>(pb + 4 * plane);
        const bool wrap = ti + 1 == ET;                   // (scalar selects, no control flow)
        ti = wrap ? 0 : ti + 1;
        tj = wrap ? tj + 2 : tj + 1;
        tj = tj >= ET ? tj - ET : tj;
      }
    };
    load_block(op[0]);
    mo_static_for<0, TPW, 2>([&](auto uc) {
      constexpr int u = decltype(uc)::value;
      constexpr int cur = (u / 2) & 1;
      if (u == UH && more) {                              // half-way: first half lands, second half leaves
        commit(t + 1, nbuf, 0);
        issue(t + 1, 1);
      }
      if (u + 2 < TPW) load_block(op[cur ^ 1]);
      const float4* o = op[cur];
#define G2V_MO_STEP(h_, c_)                                         \
  acc[u] = mfma16(o[h_].c_, o[2 + h_].c_, acc[u]);                  \
  acc[u + 1] = mfma16(o[4 + h_].c_, o[6 + h_].c_, acc[u + 1]);
      G2V_MO_STEP(0, x)
      G2V_MO_STEP(0, y)
      G2V_MO_STEP(0, z)
      G2V_MO_STEP(0, w)
      G2V_MO_STEP(1, x)
      G2V_MO_STEP(1, y)
      G2V_MO_STEP(1, z)
      G2V_MO_STEP(1, w)
#undef G2V_MO_STEP
      __builtin_amdgcn_sched_barrier(0);
    });
    if (more) commit(t + 1, nbuf, 1);
    __syncthreads();
  }

  // partials of this slab: [pair][4 registers][64 lanes] | column sums[Ep]
  float* out = part + (size_t)slab * ((size_t)P * 256 + Ep);
  mo_static_for<0, TPW, 1>([&](auto uc) {
    constexpr int u = decltype(uc)::value;
    if (u < np) {
      float* o = out + (size_t)(p0 + u) * 256 + lane;
      o[0] = acc[u][0];
      o[64] = acc[u][1];
      o[128] = acc[u][2];
      o[192] = acc[u][3];
    }
  });
  if (group == 0) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = tid + 256 * k;
      if (c < Ep) out[(size_t)P * 256 + c] = s1a[k];
    }
  }
}

// element e < P * 256: accumulator register r of lane l of pair p = S2[16 ti + 4 (l >> 4) + r][16 tj + (l & 15)]; the rest: S1.
// A workgroup folds 64 elements: wave w sums its quarter of the slabs in slab order, the four partial sums are added in wave order.
__global__ __launch_bounds__(256) void moments_fold_kernel(const float* __restrict__ part, int nslabs, double* __restrict__ s1,
                                                          double* __restrict__ s2, int E, int ET, int P) {
  __shared__ double quarter[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t e = (int64_t)blockIdx.x * 64 + lane;
  const int64_t stride = (int64_t)P * 256 + 16 * ET;
  const int per = (nslabs + 3) / 4, s_end = min(nslabs, (w + 1) * per);
  double sum = 0.0;
  if (e < stride) {
    const float* p = part + e;
    int s = w * per;
    for (; s + 4 <= s_end; s += 4) {
      const float v0 = p[(int64_t)s * stride], v1 = p[(int64_t)(s + 1) * stride], v2 = p[(int64_t)(s + 2) * stride],
                  v3 = p[(int64_t)(s + 3) * stride];
      sum += (double)v0;
      sum += (double)v1;
      sum += (double)v2;
      sum += (double)v3;
    }
    for (; s < s_end; ++s) sum += (double)p[(int64_t)s * stride];
  }
  quarter[w][lane] = sum;
  __syncthreads();
  if (w != 0 || e >= stride) return;
  sum = ((quarter[0][lane] + quarter[1][lane]) + quarter[2][lane]) + quarter[3][lane];
  if (e >= (int64_t)P * 256) {
    const int c = (int)(e - (int64_t)P * 256);
    if (c < E) s1[c] += sum;
    return;
  }
  const int pr = (int)(e >> 8), r = (int)(e >> 6) & 3, l = (int)e & 63;
  const int d = pr / ET, ti = pr - d * ET;
  int tj = ti + d;
  tj -= tj >= ET ? ET : 0;
  const int row = 16 * ti + 4 * (l >> 4) + r, col = 16 * tj + (l & 15);
  if (row >= E || col >= E) return;
  s2[(int64_t)row * E + col] += sum;
  if (ti != tj) s2[(int64_t)col * E + row] += sum;       // (a diagonal tile holds both of its triangles itself)
}

// ---- histogram --------------------------------------------------------------------------------------------------------------------
constexpr int HI_LDS_BINS = 8192;

__global__ __launch_bounds__(256) void code_histogram_kernel(const int64_t* __restrict__ idx, int64_t N, int K,
                                                            unsigned long long* __restrict__ counts, int use_lds) {
  __shared__ unsigned int bins[HI_LDS_BINS];
  const int tid = threadIdx.x;
  const int64_t start = (int64_t)blockIdx.x * 256 + tid, step = (int64_t)gridDim.x * 256;
  if (use_lds) {
    for (int k = tid; k <= K; k += 256) bins[k] = 0u;
    __syncthreads();
    for (int64_t n = start; n < N; n += step) {            // (a workgroup sees fewer than 2^32 ids: N / gridDim.x)
      const int64_t v = idx[n];
      atomicAdd(&bins[(v >= 0 && v < K) ? (int)v : K], 1u);
    }
    __syncthreads();
    for (int k = tid; k <= K; k += 256)
      if (bins[k]) atomicAdd(&counts[k], (unsigned long long)bins[k]);
  } else {
    for (int64_t n = start; n < N; n += step) {
      const int64_t v = idx[n];
      atomicAdd(&counts[(v >= 0 && v < K) ? v : (int64_t)K], 1ull);
    }
  }
}

}  // namespace
}  // namespace g2v

using namespace g2v;

extern "C" size_t g2v_moments_workspace(int64_t N, int E) {
  if (N <= 0 || E <= 0 || E > MO_MAX_E) return 0;
  const MoGeom g = mo_geom(E);
  const int64_t n = N < MO_PIECE ? N : MO_PIECE;
  const int R = mo_slab_rows(n);
  const size_t slabs = (size_t)((n + R - 1) / R);
  return slabs * mo_slab_floats(g) * sizeof(float);
}

extern "C" int g2v_moments_accumulate(const float* x, int64_t ld, const float* shift, double* s1, double* s2, int64_t N, int E,
                                      void* workspace, size_t workspace_bytes, g2v_stream_t stream) {
  G2V_REQUIRE(x && shift && s1 && s2 && workspace, "null pointer");
  G2V_REQUIRE(N > 0 && E > 0, "non-positive size");
  G2V_REQUIRE(ld >= E && ld < (1 << 24), "row stride smaller than E (or 2^24 elements and more)");
  if (E > MO_MAX_E) {
    set_error("g2v_moments_accumulate: E = %d is wider than the %d columns the kernel holds", E, MO_MAX_E);
    return G2V_ERR_UNSUPPORTED;
  }
  G2V_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(x) & 3) == 0, "misaligned pointer");
  if (workspace_bytes < g2v_moments_workspace(N, E)) {
    set_error("g2v_moments_accumulate: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const MoGeom g = mo_geom(E);
  const size_t lds = ((size_t)2 * 8 * g.Ep * 4 + g.Ep) * sizeof(float);
  const bool vec = ptr_vec_ok(x, ld) && (E & 3) == 0;       // 16-byte loads: aligned rows that end on a 4-column group
  float* part = (float*)workspace;
  for (int64_t off = 0; off < N; off += MO_PIECE) {
    const int64_t n = N - off < MO_PIECE ? N - off : MO_PIECE;
    const int R = mo_slab_rows(n);
    const int slabs = (int)((n + R - 1) / R);
    const float* xp = x + off * ld;
#define G2V_MO_LAUNCH(TPW_, VEC_)                                                                                                 \
  do {                                                                                                                            \
    if (!g2v_internal_lds_reserve((const void*)moments_slab_kernel<TPW_, VEC_>, lds)) {                                           \
      set_error("g2v_moments_accumulate: cannot reserve LDS");                                                                    \
      return G2V_ERR_LAUNCH;                                                                                                      \
    }                                                                                                                             \
    hipLaunchKernelGGL((moments_slab_kernel<TPW_, VEC_>), dim3(slabs, g.groups), dim3(256), lds, st, xp, ld, shift, part, n, R,   \
                       E, g.ET, g.P, g.per_group);                                                                                \
  } while (0)
#define G2V_MO_CASE(TPW_)                     \
  case TPW_:                                  \
    if (vec) G2V_MO_LAUNCH(TPW_, true);       \
    else G2V_MO_LAUNCH(TPW_, false);          \
    break;
    switch (g.tpw) {
      G2V_MO_CASE(4)
      G2V_MO_CASE(10)
      G2V_MO_CASE(20)
      G2V_MO_CASE(40)
      G2V_MO_CASE(66)
      default:
        if (vec) G2V_MO_LAUNCH(82, true);
        else G2V_MO_LAUNCH(82, false);
    }
#undef G2V_MO_CASE
#undef G2V_MO_LAUNCH
    hipLaunchKernelGGL(moments_fold_kernel, dim3(cdiv((int64_t)mo_slab_floats(g), 64)), dim3(256), 0, st, (const float*)part, slabs,
                       s1, s2, E, g.ET, g.P);
  }
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int g2v_code_histogram(const int64_t* idx, int64_t N, int K, int64_t* counts, g2v_stream_t stream) {
  G2V_REQUIRE(idx && counts, "null pointer");
  G2V_REQUIRE(N > 0 && K > 0, "non-positive size");
  const int blocks = (int)(N / 4096 < 1 ? 1 : N / 4096 > 1024 ? 1024 : N / 4096);
  hipLaunchKernelGGL(code_histogram_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, idx, N, K, (unsigned long long*)counts,
                     K + 1 <= HI_LDS_BINS ? 1 : 0);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
