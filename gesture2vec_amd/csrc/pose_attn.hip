// pose_attn.hip -- the text -> pose seq2seq baseline (Seq2SeqNet): a decoder with Bahdanau attention AND continuous feedback that
// carries its gradient, as fused per-step kernels (g2v_pose_attn_rollout_fwd / _bwd).
//
// Per decode step t = 0 .. S1-1:
//   x_t = target[t] while t < max(1, n_pre), else y_{t-1} (the OUTPUT, not detached)                         (D)
//   w_t = softmax_tw( v . tanh(h1_t W_attn[:, :H]^T + b_attn + enc_proj[tw]) ) over ALL Tw positions,  c_t = sum_tw w_t[tw] enc[tw]
//   u_t = [x_t | c_t] W_pre^T + b_pre;  a_t = ReLU(BatchNorm1d(u_t)) on batch statistics
//   h0_{t+1}, h1_{t+1} = GRU(a_t; h0_t, h1_t) (inter-layer dropout p on h0);  y_t = h1_{t+1} W_out^T + b_out
// The tiling and launch structure are t2e_latent.hip's (16 batch rows per 512-thread workgroup, weights packed once per call as MFMA
// A operands, a kernel boundary as the only grid-wide seam); everything the three step-kernel files share lives in t2e_cells.hpp.
//
// Forward, S1 + 1 launches of one kernel; launch j:
//   [tail of step j-1]  finish BN(u_{j-1}) from the per-workgroup partials -> ReLU -> both GRU cells -> y_{j-1} -> outputs[j]
//   [head of step j]    x_j = this tile's own y_{j-1} (still in LDS) or target_j;  hp = h1_j W_attn[:, :H]^T + b_attn from the h1 tile
//                       the tail left in LDS -> energies, softmax, context over this tile's rows (enc / enc_proj streamed from global
//                       memory) -> u_j = [x_j | c_j] W_pre^T (two column blocks of one product) + the BatchNorm partial sums (where one
//                       row tile holds the whole batch, B <= 16, the second sum is taken about the tile's own mean: t2e_cells.hpp).
// The saved input row is [x | c], D + H floats at the row stride ldec = round_up(D + H, 4) in s->ec; at D % 4 != 0 (D = 135 is the
// width the model is trained at) the rows of target, y and d_out and the context half of an ec row are not 16-byte aligned: those
// move element-wise, nothing is staged at a stride of its own.
//
// Backward, S1 + 1 launches of one kernel, descending; launch t:
//   Part A (t < S1-1)   finish the BN backward of step s = t+1 -> du_s;  du_s W_pre splits into the pose part (the feedback into d y_t
//                       where step s was fed back) and the context part d c_s -> attention backward of step s, row-local: d hp_s, this
//                       workgroup's d v partial, d enc / d enc_proj rows accumulated in place by the owning workgroup (no atomics),
//                       carry1 += d hp_s W_attn[:, :H]
//   Part B (t >= 0)     d y_t = g_t + feedback -> the cells of step t (code_bwd_cells<true>) -> BN-backward partial sums of step t.
// The carries travel between the launches in d_hidden0.  Every weight and bias gradient is batched over the S1 x B rows behind the
// loop.  No kernel here waits on another workgroup; no float atomics: the same input gives the same bits.
#include "t2e_cells.hpp"

namespace g2v {

static __host__ __device__ inline int pa_ldec(int H, int D) { return (D + H + 3) & ~3; }

// LDS carve of the backward kernel: the cells' carve (CtBwdLds, so that code_bwd_cells runs on it) with the regions Part A borrows
// grown to what it puts there -- Gi: du | d ctx, then d hp over du; Gh: BatchNorm sums + reduction scratch, then the d v rows;
// Dd: d_w / ds and the attention weights [2][16][Tw].  At H = 200 nothing grows: 146 KB.
struct PaBwdLds {
  CtBwdLds l;
  int scratch;
};
static __host__ __device__ inline PaBwdLds pa_bwd_lds(int H, int D, int Tw) {
  const int Hp = (H + 15) & ~15, ldh = Hp + 4, Gp = (3 * H + 15) & ~15, ldg = Gp + 4, Kp = (D + 15) & ~15, ldk = Kp + 4;
  auto mx = [](int a, int b) { return a > b ? a : b; };
  PaBwdLds r;
  const int gh = mx(16 * ldg, 2 * Hp + 1024);
  r.scratch = (2 * Hp + 2048 <= gh) ? 2048 : 1024;
  int o = 0;
  r.l.xdl = o; o += 16 * mx(ldk, 2 * ldh);
  r.l.gi = o; o += mx(16 * ldg, 2 * 16 * ldh);
  r.l.gh = o; o += gh;
  r.l.dd = o; o += mx(16 * ldh, 2 * 16 * Tw);
  r.l.c0 = o; o += 16 * ldh;
  r.l.c1 = o; o += 16 * ldh;
  r.l.total = o;
  return r;
}

// =====================================================================================================================
// forward: launch j of S1 + 1       (dm.K = D, dm.Hin = D + H, dm.Tw = Tw)
// =====================================================================================================================
__global__ __launch_bounds__(CT_NTHR) void pose_attn_step_fwd_kernel(const float* __restrict__ target, const float* __restrict__ h_init,
                                                                     const float* __restrict__ enc, const float* __restrict__ ep,
                                                                     g2v_code_dec_weights w, CodePackF pk, const float* __restrict__ pre_c,
                                                                     g2v_code_dec_saved sv, const uint8_t* __restrict__ keep_l0,
                                                                     CodeDims dm, int j) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NTHR = CT_NTHR;
  const int S1 = dm.S1, B = dm.B, H = dm.H, D = dm.K;
  const int Hp = (H + 15) & ~15, ldh = Hp + 4, Dp = (D + 15) & ~15, ldx = Dp + Hp + 4, ldec = pa_ldec(H, D);
  const CtFwdLds L = ct_fwd_lds(H, Dp + H, dm.Tw, dm.scratch);
  float* Xa = smem + L.xa;          // a_t                [16][ldh]   (head: hp)
  float* Xh0 = smem + L.xh0;        // h0_t
  float* Xh1 = smem + L.xh1;        // h1_t
  float* Xx1 = smem + L.xx1;        // dropped h0_{t+1}
  float* Xh1n = smem + L.xh1n;      // h1_{t+1}
  float* Xe = smem + L.xe;          // [x_j (Dp) | c_j (Hp)] [16][ldx]
  float* st = smem + L.st;          // mean[Hp], invstd[Hp]
  float* red = smem + L.red;
  float* red_scratch = smem + L.scratch;
  float* sc = smem + L.sc;          // attention scores / weights [16][Tw]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b0 = blockIdx.x * 16;
  const int nrows = min(16, B - b0);
  const bool has_tail = j > 0, has_head = j < S1;
  const int t = j - 1;                                   // the step whose tail this launch runs
  const int npre = max(1, min(dm.n_pre, S1));            // steps fed from `target` (teacher forcing; step 0 always)
  const bool feed = has_tail && has_head && j >= npre;   // step j reads this tile's own y_{j-1}

  CtRowPf pf;
  ct_fwd_prefetch(pf, sv, h_init, t, has_tail, B, H, b0, nrows, tid);
  // zero what the MFMA contractions must see as zero: padding columns, rows >= nrows
  if (nrows < 16 || Hp != H || Dp != D) {
    for (int e = tid; e < 5 * 16 * ldh + 16 * ldx; e += NTHR) smem[e] = 0.f;
  }
  lds_barrier();

  if (!has_tail) {
    ct_fwd_init_state(pf, sv, B, H, b0, Xh1n, ldh);      // (the attention of step 0 scores h1_0)
  } else {
    ct_bn_finish_fwd<true, true>(w, sv, dm, t, st, red, red_scratch, tid);
    lds_barrier();
    ct_bn_relu_stage(pf, w, sv, st, Xa, Xh0, Xh1, ldh, t, B, H, b0);
    lds_barrier();
    const bool drop = keep_l0 && dm.p_drop > 0.f;
    ct_cells_fwd(pk, w, sv, keep_l0, drop, dm, t, b0, nrows, Xa, Xh0, Xh1, Xx1, Xh1n, lane, wave);
    ct_out_feed_fwd(pk.out, w.b_out, Xh1n, ldh, Hp, D, sv.logits + ((int64_t)t * B + b0) * D, feed, Xe, ldx,
                    sv.ec + ((int64_t)j * B + b0) * ldec, ldec, nrows, lane, wave);
  }
  if (!has_head) return;
  // ---- head of step j: x_j = target_j while teacher-forced (else the tile the out layer just left in LDS) ------------------
  if (!feed) {
    if ((D & 3) == 0) {
      const int D4 = D >> 2;
      for (int e = tid; e < 16 * D4; e += NTHR) {
        const int r = e / D4, c = (e - r * D4) * 4;
        if (r >= nrows) continue;
        const float4 v = *reinterpret_cast<const float4*>(target + ((int64_t)j * B + b0 + r) * D + c);
        *reinterpret_cast<float4*>(Xe + r * ldx + c) = v;
        *reinterpret_cast<float4*>(sv.ec + ((int64_t)j * B + b0 + r) * ldec + c) = v;
      }
    } else {
      for (int e = tid; e < 16 * D; e += NTHR) {
        const int r = e / D, c = e - r * D;
        if (r >= nrows) continue;
        const float v = target[((int64_t)j * B + b0 + r) * D + c];
        Xe[r * ldx + c] = v;
        sv.ec[((int64_t)j * B + b0 + r) * ldec + c] = v;
      }
    }
  }
  // ---- attention on h1_j (the Xh1n tile: the tail's, or h_init's at launch 0); a_t is dead: hp takes its tile --------------
  ct_attn_head_fwd(pk.attn_h, w, sv, enc, ep, Xh1n, Xa, sc, Xe + Dp, ldx, sv.ec + ((int64_t)j * B + b0) * ldec + D, ldec, (D & 3) == 0, pf,
                   dm, j, b0, nrows, tid);
  lds_barrier();
  // ---- u_j = [x_j | c_j] W_pre^T + b_pre and the per-workgroup BatchNorm partial sums -----------------------------------------
  ct_pre_linear_partials<true>(pk.pre, Dp >> 4, Xe, pre_c, Hp >> 4, Xe + Dp, ldx, w, sv, dm, j, b0, nrows, lane, wave);
}

// =====================================================================================================================
// backward: launch for step t = S1-1 .. 0, and a last launch t = -1 that only finishes step 0 (BatchNorm and attention backward) and
// writes d_hidden0.     (a.d_logits = g (S1,B,D); dm.K = D; a.tw.pre_ctx_t = W_pre[:, D:]^T; pre_x_t = W_pre[:, :D]^T)
// =====================================================================================================================
__global__ __launch_bounds__(CT_NTHR) void pose_attn_step_bwd_kernel(CodeBwdArgs a, CodeDims dm, int t, const float* __restrict__ pre_x_t,
                                                                     float* __restrict__ dy) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NTHR = CT_NTHR, NW = CT_NW;
  const CtBwdLds L = pa_bwd_lds(dm.H, dm.K, dm.Tw).l;
  const int S1 = dm.S1, B = dm.B, H = dm.H, D = dm.K, Tw = dm.Tw;
  const int Hp = (H + 15) & ~15, ldh = Hp + 4, Dp = (D + 15) & ~15, ldk = Dp + 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int b0 = blockIdx.x * 16, nrows = min(16, B - b0);
  const int npre = max(1, min(dm.n_pre, S1));
  float* C0 = smem + L.c0;
  float* C1 = smem + L.c1;
  float* Xdy = smem + L.xdl;               // [16][ldk]   the feedback term, then d y_t (code_bwd_cells' d-logits tile)
  float* Xdu = smem + L.gi;                // [16][ldh]   du_{t+1}; dead behind the two products: d hp takes its place
  float* Xdc = Xdu + 16 * ldh;             // [16][ldh]   d ctx
  float* red = smem + L.gh;                // [2H] BatchNorm backward sums; dead before the d v rows land
  float* red_scratch = red + 2 * Hp;       // [dm.scratch]
  float* dsc = smem + L.dd;                // [16][Tw] d_w -> ds
  float* wsc = dsc + 16 * Tw;              // [16][Tw] attention weights of step t+1
  const bool last = (t == S1 - 1);
  const bool fed = !last && t >= 0 && (t + 1) >= npre;      // step t+1 read y_t
  for (int e = tid; e < L.total; e += NTHR) smem[e] = 0.f;
  lds_barrier();
  if (!last) {
    ct_bwd_load_carries(a, dm, C0, C1, b0, nrows, tid);
    // ================= Part A: BatchNorm backward of step s = t+1, attention backward of step s ==========================
    const int s = t + 1;
    ct_bn_bwd_finish<true>(a, dm, s, red, red_scratch, Xdu, b0, nrows, tid);
    lds_barrier();
    // du_s W_pre: the pose columns = the feedback term of d y_t (where step s was fed back), the context columns = d ctx_s
    if (fed) {
      const int nte = Dp >> 4;
      for (int et = wave; et < nte; et += NW) {
        f32x4 acc[1] = {(f32x4){0.f, 0.f, 0.f, 0.f}};
        wave_gemm_p<1, 0>(acc, pre_x_t, Hp >> 4, et, 0, Xdu, ldh, lane);
        *reinterpret_cast<float4*>(Xdy + i * ldk + 16 * et + 4 * q) = make_float4(acc[0][0], acc[0][1], acc[0][2], acc[0][3]);
      }
    }
    const int nth = Hp >> 4;
    for (int ft = wave; ft < nth; ft += NW) {
      const int f0 = 16 * ft + 4 * q;
      f32x4 acc[1] = {(f32x4){0.f, 0.f, 0.f, 0.f}};
      wave_gemm_p<1, 0>(acc, a.tw.pre_ctx_t, Hp >> 4, ft, 0, Xdu, ldh, lane);
      if (f0 + 3 < H) *reinterpret_cast<float4*>(Xdc + i * ldh + f0) = make_float4(acc[0][0], acc[0][1], acc[0][2], acc[0][3]);
    }
    lds_barrier();
    ct_attn_bwd_step(a, dm, s, Xdc, Xdu, dsc, wsc, smem + L.gh, C1, b0, nrows, tid);
    // Gi / Gh / Dd were borrowed: padding back to zero for the cells (the d y tile keeps the feedback term)
    for (int e = tid + L.gi; e < L.c0; e += NTHR) smem[e] = 0.f;
    lds_barrier();
  }
  if (t >= 0) code_bwd_cells<true>(a, dm, L, smem, t, b0, nrows, tid, last, fed, dy);
  code_bwd_write_hidden0(a, dm, L, smem, b0, nrows, tid);
}

// d attn.attn.weight (H,2H) = [dW_h | 0]: the encoder half belongs to the caller's enc_proj product
__global__ void pose_attn_join_kernel(const float* __restrict__ dwh, float* __restrict__ out, int H) {
  for (int e = blockIdx.x * 256 + threadIdx.x; e < H * H; e += gridDim.x * 256) {
    const int r = e / H, c = e - r * H;
    out[(int64_t)r * 2 * H + c] = dwh[e];
    out[(int64_t)r * 2 * H + H + c] = 0.f;
  }
}

}  // namespace g2v

// ---------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------
using namespace g2v;

static size_t pa_fwd_lds_floats(int H, int D, int Tw, int scratch) {
  return (size_t)ct_fwd_lds(H, ((D + 15) & ~15) + H, Tw, scratch).total;
}

extern "C" int g2v_pose_attn_rollout_ok(int S1, int B, int H, int D, int Tw) {
  if (S1 < 1 || B < 2 || H < 16 || (H & 3) || H > 256 || D < 1 || D > 256 || Tw < 1 || Tw > CT_MAX_TW) return 0;
  const size_t lf = pa_fwd_lds_floats(H, D, Tw, 1024) * 4;
  const size_t lb = (size_t)pa_bwd_lds(H, D, Tw).l.total * 4;
  return lf <= 160 * 1024 && lb <= 160 * 1024;
}

extern "C" int g2v_pose_attn_rollout_plan(int S1, int B, int H, int D, int Tw, int fused_min_rows) {
  return (g2v_pose_attn_rollout_ok(S1, B, H, D, Tw) && B >= fused_min_rows) ? 1 : 0;
}

static size_t pa_fwd_pack_floats(int H, int D) {
  return pack_floats(H, 1, D) + 2 * pack_floats(H, 1, H) + 4 * pack_floats(H, 3, H) + (size_t)ct_ktiles_alloc(D) * pack_ks(H) * 256;
}
extern "C" size_t g2v_pose_attn_rollout_fwd_workspace(int H, int D) {
  if (H < 1 || D < 1) return 0;
  return al256(pa_fwd_pack_floats(H, D) * sizeof(float));
}

extern "C" int g2v_pose_attn_rollout_fwd(const float* target, const float* h_init, const float* enc, const float* enc_proj,
                                         const g2v_code_dec_weights* w, const g2v_code_dec_saved* s, const uint8_t* keep_l0,
                                         float p_drop, int n_pre, int S1, int B, int H, int D, int Tw, void* workspace,
                                         size_t workspace_bytes, g2v_stream_t stream) {
  G2V_REQUIRE(target && h_init && enc && enc_proj && w && s && workspace, "null pointer");
  G2V_REQUIRE(w->w_attn && w->b_attn && w->v_attn, "attention: missing array");
  G2V_REQUIRE((w->bn_running_mean == nullptr) == (w->bn_running_var == nullptr), "BatchNorm running statistics: both or neither");
  G2V_REQUIRE(w->w_pre && w->b_pre && w->bn_w && w->bn_b && w->w_ih0 && w->w_hh0 && w->b_ih0 && w->b_hh0 && w->w_ih1 && w->w_hh1 &&
              w->b_ih1 && w->b_hh1 && w->w_out && w->b_out, "missing weight");
  G2V_REQUIRE(s->ec && s->u && s->a && s->bn_stats && s->h0 && s->h1 && s->gates0 && s->gates1 && s->logits && s->bn_partial &&
              s->hp && s->attw, "missing state buffer");
  G2V_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "bad dropout probability");
  const bool drop = keep_l0 && p_drop > 0.f;
  G2V_REQUIRE(!drop || s->x1, "inter-layer dropout: no x1 buffer");
  if (!g2v_pose_attn_rollout_ok(S1, B, H, D, Tw)) {
    set_error("g2v_pose_attn_rollout_fwd: shape not served (g2v_pose_attn_rollout_ok)");
    return G2V_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < g2v_pose_attn_rollout_fwd_workspace(H, D)) {
    set_error("g2v_pose_attn_rollout_fwd: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  const bool dvec = (D & 3) == 0;
  const void* al[] = {h_init, enc, enc_proj, w->b_pre, w->bn_w, w->bn_b, w->b_ih0, w->b_hh0, w->b_ih1, w->b_hh1, w->b_attn, w->v_attn,
                      dvec ? w->b_out : nullptr, dvec ? target : nullptr, dvec ? s->logits : nullptr, s->ec, s->u, s->a, s->h0, s->h1,
                      s->x1, s->gates0, s->gates1, s->bn_partial, s->hp, keep_l0, workspace};
  for (const void* p : al) G2V_REQUIRE(ct_al16(p), "16-byte alignment");
  hipStream_t st = (hipStream_t)stream;
  // ---- pack the weights into MFMA fragment order (one launch) ----
  float* p = (float*)workspace;
  PackBatch pb;
  CodePackF pk{};
  const int Hin = D + H;
  pb.n = 0;
  pb.d[pb.n++] = PackDesc{w->w_pre, p, H, 1, 0, D, Hin, 0, 0}; pk.pre = p; p += pack_floats(H, 1, D);              // W_pre[:, :D]
  const float* pre_c = p;
  pb.d[pb.n++] = PackDesc{w->w_pre + D, p, H, 1, 0, H, Hin, 0, 0}; p += pack_floats(H, 1, H);                      // W_pre[:, D:]
  pb.d[pb.n++] = PackDesc{w->w_attn, p, H, 1, 0, H, 2 * H, 0, 0}; pk.attn_h = p; p += pack_floats(H, 1, H);        // W_attn[:, :H]
  pb.d[pb.n++] = PackDesc{w->w_ih0, p, H, 3, H, H, H, 0, 0}; pk.ih0 = p; p += pack_floats(H, 3, H);
  pb.d[pb.n++] = PackDesc{w->w_hh0, p, H, 3, H, H, H, 0, 0}; pk.hh0 = p; p += pack_floats(H, 3, H);
  pb.d[pb.n++] = PackDesc{w->w_ih1, p, H, 3, H, H, H, 0, 0}; pk.ih1 = p; p += pack_floats(H, 3, H);
  pb.d[pb.n++] = PackDesc{w->w_hh1, p, H, 3, H, H, H, 0, 0}; pk.hh1 = p; p += pack_floats(H, 3, H);
  pb.d[pb.n++] = PackDesc{w->w_out, p, D, 1, 0, H, H, 0, ct_ktiles_alloc(D)}; pk.out = p;
  launch_pack(pb, st);
  G2V_CHECK_LAUNCH();
  const int scratch = ct_scratch(pa_fwd_lds_floats(H, D, Tw, 0));
  CodeDims dm{S1, B, H, D, Hin, Tw, drop ? p_drop : 0.f, n_pre, 1, cdiv(B, 16), 1, scratch};
  const size_t lds = pa_fwd_lds_floats(H, D, Tw, scratch) * sizeof(float);
  if (!g2v_internal_lds_reserve((const void*)pose_attn_step_fwd_kernel, lds)) return G2V_ERR_LAUNCH;
  for (int j = 0; j <= S1; ++j)
    hipLaunchKernelGGL(pose_attn_step_fwd_kernel, dim3(dm.nblk), dim3(CT_NTHR), lds, st, target, h_init, enc, enc_proj, *w, pk, pre_c, *s,
                       drop ? keep_l0 : nullptr, dm, j);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

// ---- backward workspace layout (bytes, every region 256-byte aligned) ----------------------------------------------------
struct PaBwdWs {
  size_t pack, dgi0, dgh0, dgi1, dgh1, dbn, du, dy, dhp, dvp, dwh, bn_part, bn_sums, wg, total;
};
static PaBwdWs pa_bwd_ws(int S1, int B, int H, int D) {
  const size_t M = (size_t)S1 * B, G = 3 * (size_t)H, nblk = cdiv(B, 16);
  PaBwdWs l;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += al256(bytes); return at; };
  l.pack = take((pack_floats(H, 1, D) + 4 * pack_floats(H, 1, 3 * H) + pack_floats(D, 1, H) + 2 * pack_floats(H, 1, H)) * 4);
  l.dgi0 = take(M * G * 4); l.dgh0 = take(M * G * 4); l.dgi1 = take(M * G * 4); l.dgh1 = take(M * G * 4);
  l.dbn = take(M * H * 4);
  l.du = take(M * H * 4);
  l.dy = take(M * D * 4);
  l.dhp = take(M * H * 4);
  l.dvp = take(nblk * H * 4);
  l.dwh = take((size_t)H * H * 4);
  l.bn_part = take((size_t)S1 * nblk * 2 * H * 4);
  l.bn_sums = take((size_t)S1 * 2 * H * 4);
  size_t wg = 4 * g2v_linear_bwd_weight_workspace((int)M, H, 3 * H);
  auto up = [&](size_t v) { wg = wg > v ? wg : v; };
  up(g2v_linear_bwd_weight_workspace((int)M, H, D));
  up(g2v_linear_bwd_weight_workspace((int)M, D + H, H));
  up(g2v_linear_bwd_weight_workspace((int)M, H, H));
  l.wg = take(wg);
  l.total = o;
  return l;
}
extern "C" size_t g2v_pose_attn_rollout_bwd_workspace(int S1, int B, int H, int D, int Tw) {
  (void)Tw;
  if (S1 < 1 || B < 1 || H < 1 || D < 1) return 0;
  return pa_bwd_ws(S1, B, H, D).total;
}

extern "C" int g2v_pose_attn_rollout_bwd(const float* d_out, const float* enc, const float* enc_proj, const g2v_code_dec_weights* w,
                                         const g2v_code_dec_saved* s, const g2v_code_dec_grads* g, const uint8_t* keep_l0, float p_drop,
                                         int n_pre, int S1, int B, int H, int D, int Tw, void* workspace, size_t workspace_bytes,
                                         g2v_stream_t stream) {
  G2V_REQUIRE(d_out && enc && enc_proj && w && s && g && workspace, "null pointer");
  G2V_REQUIRE(w->w_attn && w->v_attn, "attention: missing array");
  G2V_REQUIRE(w->w_pre && w->bn_w && w->w_ih0 && w->w_hh0 && w->w_ih1 && w->w_hh1 && w->w_out, "missing weight");
  G2V_REQUIRE(s->ec && s->u && s->a && s->bn_stats && s->h0 && s->h1 && s->gates0 && s->gates1 && s->hp && s->attw, "missing saved buffer");
  G2V_REQUIRE(g->d_hidden0 && g->d_w_pre && g->d_b_pre && g->d_bn_w && g->d_bn_b && g->d_w_ih0 && g->d_w_hh0 && g->d_b_ih0 &&
              g->d_b_hh0 && g->d_w_ih1 && g->d_w_hh1 && g->d_b_ih1 && g->d_b_hh1 && g->d_w_out && g->d_b_out && g->d_w_attn &&
              g->d_b_attn && g->d_v_attn && g->d_enc && g->d_emb, "missing gradient buffer");
  G2V_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "bad dropout probability");
  const bool drop = keep_l0 && p_drop > 0.f;
  G2V_REQUIRE(!drop || s->x1, "inter-layer dropout: x1 was not saved");
  if (!g2v_pose_attn_rollout_ok(S1, B, H, D, Tw)) {
    set_error("g2v_pose_attn_rollout_bwd: shape not served (g2v_pose_attn_rollout_ok)");
    return G2V_ERR_UNSUPPORTED;
  }
  const PaBwdWs L = pa_bwd_ws(S1, B, H, D);
  if (workspace_bytes < L.total) {
    set_error("g2v_pose_attn_rollout_bwd: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  const bool dvec = (D & 3) == 0;
  const void* al[] = {workspace, dvec ? d_out : nullptr, enc, enc_proj, g->d_hidden0, g->d_enc, g->d_emb, w->bn_w, w->v_attn, s->ec, s->u,
                      s->a, s->bn_stats, s->h0, s->h1, drop ? s->x1 : nullptr, s->gates0, s->gates1, s->hp, keep_l0};
  for (const void* p : al) G2V_REQUIRE(ct_al16(p), "16-byte alignment");
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)workspace;
  const int G = 3 * H, M = S1 * B, Hin = D + H, ldec = pa_ldec(H, D);
  // ---- transposed packs ----
  float* p = (float*)(base + L.pack);
  PackBatch pb;
  CodeBwdArgs a{};
  pb.n = 0;
  pb.d[pb.n++] = PackDesc{w->w_out, p, H, 1, 0, D, H, 1, 0}; a.tw.out_t = p; p += pack_floats(H, 1, D);      // rows f, k = e: W_out[e][f]
  pb.d[pb.n++] = PackDesc{w->w_ih0, p, H, 1, 0, G, H, 1, 0}; a.tw.ih0_t = p; p += pack_floats(H, 1, G);
  pb.d[pb.n++] = PackDesc{w->w_hh0, p, H, 1, 0, G, H, 1, 0}; a.tw.hh0_t = p; p += pack_floats(H, 1, G);
  pb.d[pb.n++] = PackDesc{w->w_ih1, p, H, 1, 0, G, H, 1, 0}; a.tw.ih1_t = p; p += pack_floats(H, 1, G);
  pb.d[pb.n++] = PackDesc{w->w_hh1, p, H, 1, 0, G, H, 1, 0}; a.tw.hh1_t = p; p += pack_floats(H, 1, G);
  const float* pre_x_t = p;                                                                                   // rows e, k = f: W_pre[f][e]
  pb.d[pb.n++] = PackDesc{w->w_pre, p, D, 1, 0, H, Hin, 1, 0}; p += pack_floats(D, 1, H);
  pb.d[pb.n++] = PackDesc{w->w_pre + D, p, H, 1, 0, H, Hin, 1, 0}; a.tw.pre_ctx_t = p; p += pack_floats(H, 1, H);   // rows c, k = f: W_pre[f][D + c]
  pb.d[pb.n++] = PackDesc{w->w_attn, p, H, 1, 0, H, 2 * H, 1, 0}; a.tw.attn_h_t = p;                          // rows c, k = f: W_attn[f][c]
  launch_pack(pb, st);
  G2V_CHECK_LAUNCH();
  a.d_logits = d_out; a.enc = enc; a.ep = enc_proj; a.w = *w; a.sv = *s; a.keep_l0 = drop ? keep_l0 : nullptr;
  a.dgi0 = (float*)(base + L.dgi0); a.dgh0 = (float*)(base + L.dgh0); a.dgi1 = (float*)(base + L.dgi1); a.dgh1 = (float*)(base + L.dgh1);
  a.dbn = (float*)(base + L.dbn); a.du = (float*)(base + L.du);
  a.dhp = (float*)(base + L.dhp); a.d_ep = g->d_emb; a.d_enc = g->d_enc; a.dv_partial = (float*)(base + L.dvp);
  a.bn_part = (float*)(base + L.bn_part); a.bn_sums = (float*)(base + L.bn_sums); a.d_hidden0 = g->d_hidden0;
  float* dy = (float*)(base + L.dy);
  float* dwh = (float*)(base + L.dwh);
  const PaBwdLds bl = pa_bwd_lds(H, D, Tw);
  CodeDims dm{S1, B, H, D, Hin, Tw, drop ? p_drop : 0.f, n_pre, 1, cdiv(B, 16), 1, bl.scratch};
  const size_t lds = (size_t)bl.l.total * sizeof(float);
  if (!g2v_internal_lds_reserve((const void*)pose_attn_step_bwd_kernel, lds)) return G2V_ERR_LAUNCH;
  for (int t = S1 - 1; t >= -1; --t)
    hipLaunchKernelGGL(pose_attn_step_bwd_kernel, dim3(dm.nblk), dim3(CT_NTHR), lds, st, a, dm, t, pre_x_t, dy);
  hipLaunchKernelGGL(code_small_sums_kernel, dim3(1), dim3(256), 0, st, a.bn_sums, S1, H, g->d_bn_w, g->d_bn_b,
                     (const float*)a.dv_partial, dm.nblk, g->d_v_attn);
  G2V_CHECK_LAUNCH();
  // ---- every weight gradient: one launch over the S1 x B rows each ---------------------------------------------------------
  void* wgws = base + L.wg;
  const size_t wgn = L.total - L.wg;
  int rc;
  if ((rc = g2v_linear_bwd_weight(dy, D, s->h1 + (size_t)B * H, H, 0, 0, 0, nullptr, 1.0f, g->d_w_out, g->d_b_out, M, H, D, 0, wgws, wgn,
                                  stream)) != G2V_OK)
    return rc;
  if ((rc = g2v_linear_bwd_weight(a.du, H, s->ec, ldec, 0, 0, 0, nullptr, 1.0f, g->d_w_pre, g->d_b_pre, M, Hin, H, 0, wgws, wgn,
                                  stream)) != G2V_OK)
    return rc;
  g2v_wgrad_item it[4];
  const float* x1 = drop ? s->x1 : s->h0 + (size_t)B * H;     // layer 1's input: dropped h0_{t+1}
  it[0] = g2v_wgrad_item{a.dgi0, s->a, g->d_w_ih0, g->d_b_ih0};
  it[1] = g2v_wgrad_item{a.dgh0, s->h0, g->d_w_hh0, g->d_b_hh0};
  it[2] = g2v_wgrad_item{a.dgi1, x1, g->d_w_ih1, g->d_b_ih1};
  it[3] = g2v_wgrad_item{a.dgh1, s->h1, g->d_w_hh1, g->d_b_hh1};
  if ((rc = g2v_linear_bwd_weight_batch(it, 4, G, H, M, H, G, 0, wgws, wgn, stream)) != G2V_OK) return rc;
  // attn.attn.weight[:, :H]: d W_h = dhp^T h1_t (the state in front of each step); bias from dhp.  The encoder half [:, H:] and the
  // enc_proj -> enc path belong to the caller (g2v_linear_bwd_weight / g2v_linear_bwd_data on g->d_emb = d loss / d enc_proj)
  if ((rc = g2v_linear_bwd_weight(a.dhp, H, s->h1, H, 0, 0, 0, nullptr, 1.0f, dwh, g->d_b_attn, M, H, H, 0, wgws, wgn, stream)) != G2V_OK)
    return rc;
  hipLaunchKernelGGL(pose_attn_join_kernel, dim3(cdiv(H * H, 256)), dim3(256), 0, st, dwh, g->d_w_attn, H);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
