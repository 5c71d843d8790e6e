// t2e_latent.hip -- Part d on continuous latents (text2_embedding_discrete: False): the attention-free decoder of
// text2embedding_model that regresses each chunk's latent vector, as fused per-step kernels (g2v_latent_rollout_fwd / _bwd).
//
// Replaces the loop model/text2embedding_model.py:701-744 over BahdanauAttnDecoderRNN.forward (:338-395) in its continuous form and
// its autograd: per decode step  x_t (E) -> Linear(E -> H) + BatchNorm1d + ReLU -> GRU (2 layers) -> y_t = Linear(H -> E), where
// x_t is the target's slot t while teacher-forced and y_{t-1} afterwards -- the output itself, NOT detached (:741).  There is no
// embedding, no Dropout(0.5) and no argmax.
//
// Forward (the tiling of t2e_rollout.hip: 16 batch rows per 512-thread workgroup, weights packed once per call as MFMA A operands,
// a kernel boundary as the only grid-wide seam): S1 + 1 launches of one kernel,
//   launch j:  [tail of step j-1]  finish BN(u_{j-1}) from the per-workgroup partials -> ReLU -> GRU cell 0 -> inter-layer dropout
//                                  -> GRU cell 1 -> y_{j-1} = out(h1) -> outputs[j]
//              [head of step j]    x_j = this tile's own y_{j-1} (still in LDS) or target_j -> u_j = pre_linear(x_j) + partial sums.
//
// Backward: because y_t feeds step t+1 with its gradient, d loss / d y_t = g_t + du_{t+1} W_pre, and du_{t+1} comes out of
// BatchNorm's backward of step t+1, which sums over ALL batch rows.  The one-launch BPTT of the discrete decoder does not apply:
// S1 + 1 launches of one kernel, descending,
//   launch t:  [finish BN backward of step t+1 from the partials -> du_{t+1} -> (step t+1 fed back) the feedback term du W_pre]
//              + [dy_t = g_t + feedback -> dh1 += dy_t W_out -> both cells (t2e_cells.hpp) -> BN backward partial sums of step t],
// the state-gradient carries travelling between the launches in d_hidden0; launch t = -1 only finishes step 0.  Every weight and
// bias gradient is batched over the S1 x B rows behind the loop (g2v_linear_bwd_weight / _batch).  No kernel here waits on another
// workgroup.
#include "t2e_cells.hpp"

namespace g2v {

// =====================================================================================================================
// forward: launch j of S1 + 1       (dm.K = dm.Hin = E, dm.Tw = 0)
// =====================================================================================================================
__global__ __launch_bounds__(CT_NTHR) void latent_step_fwd_kernel(const float* __restrict__ target, const float* __restrict__ h_init,
                                                                  g2v_code_dec_weights w, CodePackF pk, g2v_code_dec_saved sv,
                                                                  const uint8_t* __restrict__ keep_l0, CodeDims dm, int j) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NTHR = CT_NTHR;
  const int S1 = dm.S1, B = dm.B, H = dm.H, E = dm.K;
  const int Hp = (H + 15) & ~15, ldh = Hp + 4, Ep = (E + 15) & ~15, ldx = Ep + 4;
  const CtFwdLds L = ct_fwd_lds(H, E, 0, dm.scratch);
  float* Xa = smem + L.xa;          // a_t                [16][ldh]
  float* Xh0 = smem + L.xh0;        // h0_t
  float* Xh1 = smem + L.xh1;        // h1_t
  float* Xx1 = smem + L.xx1;        // dropped h0_{t+1}
  float* Xh1n = smem + L.xh1n;      // h1_{t+1}
  float* Xe = smem + L.xe;          // x_j                [16][ldx]
  float* st = smem + L.st;          // mean[Hp], invstd[Hp]
  float* red = smem + L.red;
  float* red_scratch = smem + L.scratch;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b0 = blockIdx.x * 16;
  const int nrows = min(16, B - b0);
  const bool has_tail = j > 0, has_head = j < S1;
  const int t = j - 1;                                   // the step whose tail this launch runs
  const int npre = max(1, min(dm.n_pre, S1));            // steps fed from `target` (teacher forcing :734-737; step 0 always)
  const bool feed = has_tail && has_head && j >= npre;   // step j reads this tile's own y_{j-1}

  // ---- prefetch this block's rows of u_t, h0_t, h1_t (written by the previous launch on some other CU) -------------------
  CtRowPf pf;
  ct_fwd_prefetch(pf, sv, h_init, t, has_tail, B, H, b0, nrows, tid);
  // zero what the MFMA contractions must see as zero: padding columns, rows >= nrows
  if (nrows < 16 || Hp != H || Ep != E) {
    for (int e = tid; e < 5 * 16 * ldh + 16 * ldx; e += NTHR) smem[e] = 0.f;
  }
  lds_barrier();

  if (!has_tail) {
    // state in front of step 0 = encoder_hidden[:2] (:667-669)
    ct_fwd_init_state(pf, sv, B, H, b0, nullptr, ldh);
  } else {
    // ---- (a) BatchNorm statistics of u_t (batch statistics: this rollout is the training forward) ------------------------
    ct_bn_finish_fwd<false>(w, sv, dm, t, st, red, red_scratch, tid);
    lds_barrier();
    // ---- (b) a_t = ReLU(BN(u_t)); stage the previous hidden states -----------------------------------------------------
    ct_bn_relu_stage(pf, w, sv, st, Xa, Xh0, Xh1, ldh, t, B, H, b0);
    lds_barrier();
    // ---- (c) GRU layer 0, (d) GRU layer 1 ------------------------------------------------------------------------------
    const bool drop = keep_l0 && dm.p_drop > 0.f;
    ct_cells_fwd(pk, w, sv, keep_l0, drop, dm, t, b0, nrows, Xa, Xh0, Xh1, Xx1, Xh1n, lane, wave);
    // ---- (e) y_t = out(h1_{t+1}) -> outputs[t + 1]; fed back: also the x tile of step j and its saved row -----------------
    ct_out_feed_fwd(pk.out, w.b_out, Xh1n, ldh, Hp, E, sv.logits + ((int64_t)t * B + b0) * E, feed, Xe, ldx,
                    sv.ec + ((int64_t)j * B + b0) * E, E, nrows, lane, wave);
  }
  if (!has_head) return;
  // ---- head of step j: x_j = target_j while teacher-forced (else the tile the out layer just left in LDS) ------------------
  if (!feed) {
    const int E4 = E >> 2;
    for (int e = tid; e < 16 * E4; e += NTHR) {
      const int r = e / E4, c = (e - r * E4) * 4;
      if (r >= nrows) continue;
      const float4 v = *reinterpret_cast<const float4*>(target + ((int64_t)j * B + b0 + r) * E + c);
      *reinterpret_cast<float4*>(Xe + r * ldx + c) = v;
      *reinterpret_cast<float4*>(sv.ec + ((int64_t)j * B + b0 + r) * E + c) = v;
    }
  }
  lds_barrier();
  // ---- u_j = pre_linear.0(x_j) and per-workgroup BatchNorm partial sums of (u - b) --------------------------------------------
  ct_pre_linear_partials(pk.pre, Ep >> 4, Xe, nullptr, 0, nullptr, ldx, w, sv, dm, j, b0, nrows, lane, wave);
}

// =====================================================================================================================
// backward: launch for step t = S1-1 .. 0, and a last launch t = -1 that only finishes step 0's BatchNorm backward.
// Part A (t < S1-1): finish the BN backward of step s = t+1 from the per-workgroup partials -> du_s; if step s read y_t
// (s >= npre): the feedback term du_s W_pre into the d y tile.  Part B: the cells of step t (code_bwd_cells<true>), which adds the
// loss's own gradient g_t to the tile, leaves d y_t in `dy` and the BN-backward partial sums of step t.  The carries travel
// between the launches in d_hidden0.     (a.d_logits = g (S1,B,E); dm.K = E)
// =====================================================================================================================
__global__ __launch_bounds__(CT_NTHR) void latent_step_bwd_kernel(CodeBwdArgs a, CodeDims dm, int t, const float* __restrict__ pre_t,
                                                                  float* __restrict__ dy) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NTHR = CT_NTHR, NW = CT_NW;
  const CtBwdLds L = ct_bwd_lds(dm.H, dm.K);
  const int S1 = dm.S1, B = dm.B, H = dm.H, E = dm.K;
  const int Hp = (H + 15) & ~15, ldh = Hp + 4, Ep = (E + 15) & ~15, ldk = Ep + 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int b0 = blockIdx.x * 16, nrows = min(16, B - b0);
  const int npre = max(1, min(dm.n_pre, S1));
  float* C0 = smem + L.c0;
  float* C1 = smem + L.c1;
  float* Xdy = smem + L.xdl;               // [16][ldk]   the feedback term, then d y_t (code_bwd_cells' d-logits tile)
  float* Xdu = smem + L.gi;                // [16][ldh]   du_{t+1} (Gi is free until the cells)
  float* red = smem + L.gh;                // [2H] BatchNorm backward sums (Gh is free until the cells)
  float* red_scratch = red + 2 * Hp;       // [dm.scratch]
  const bool last = (t == S1 - 1);
  const bool fed = !last && t >= 0 && (t + 1) >= npre;      // step t+1 read y_t
  for (int e = tid; e < L.total; e += NTHR) smem[e] = 0.f;
  lds_barrier();
  if (!last) {
    if (t >= 0) ct_bwd_load_carries(a, dm, C0, C1, b0, nrows, tid);      // carries of step t+1 (written by the previous launch)
    // ================= Part A: BatchNorm backward of step s = t+1 =========================================================
    const int s = t + 1;
    ct_bn_bwd_finish(a, dm, s, red, red_scratch, Xdu, b0, nrows, tid);
    if (t < 0) return;
    lds_barrier();
    // the feedback term: d y_t += du_s W_pre   (rows = output feature e, contraction over the H outputs of pre_linear)
    if (fed) {
      const int nte = Ep >> 4;
      for (int et = wave; et < nte; et += NW) {
        f32x4 acc[1] = {(f32x4){0.f, 0.f, 0.f, 0.f}};
        wave_gemm_p<1, 0>(acc, pre_t, Hp >> 4, et, 0, Xdu, ldh, lane);
        *reinterpret_cast<float4*>(Xdy + i * ldk + 16 * et + 4 * q) = make_float4(acc[0][0], acc[0][1], acc[0][2], acc[0][3]);
      }
    }
    lds_barrier();
    // Gi / Gh were borrowed: padding back to zero for the cells
    for (int e = tid + L.gi; e < L.dd; e += NTHR) smem[e] = 0.f;
    lds_barrier();
  }
  code_bwd_cells<true>(a, dm, L, smem, t, b0, nrows, tid, last, fed, dy);
  code_bwd_write_hidden0(a, dm, L, smem, b0, nrows, tid);
}

}  // namespace g2v

// ---------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------
using namespace g2v;

extern "C" int g2v_latent_rollout_ok(int S1, int B, int H, int E, int attention) {
  if (attention) return 0;            // with attention d(context) couples the steps as well: the per-operator chain serves it
  if (S1 < 1 || B < 1 || H < 16 || (H & 3) || H > 256 || E < 4 || (E & 3) || E > 1024) return 0;
  const size_t lf = (size_t)ct_fwd_lds(H, E, 0, 1024).total * 4;
  const size_t lb = (size_t)ct_bwd_lds(H, E).total * 4;
  const int Hp = (H + 15) & ~15;
  if (2 * Hp + 1024 > 16 * (((3 * H + 15) & ~15) + 4)) return 0;      // what Part A of the backward borrows from the gate tile
  return lf <= 160 * 1024 && lb <= 160 * 1024;
}

static size_t lt_fwd_pack_floats(int H, int E) {
  return pack_floats(H, 1, E) + 4 * pack_floats(H, 3, H) + (size_t)ct_ktiles_alloc(E) * pack_ks(H) * 256;
}
extern "C" size_t g2v_latent_rollout_fwd_workspace(int H, int E) {
  if (H < 1 || E < 1) return 0;
  return al256(lt_fwd_pack_floats(H, E) * sizeof(float));
}

extern "C" int g2v_latent_rollout_fwd(const float* target, const float* h_init, const g2v_code_dec_weights* w,
                                      const g2v_code_dec_saved* s, const uint8_t* keep_l0, float p_drop, int n_pre, int S1, int B,
                                      int H, int E, void* workspace, size_t workspace_bytes, g2v_stream_t stream) {
  G2V_REQUIRE(target && h_init && w && s && workspace, "null pointer");
  G2V_REQUIRE(!w->w_attn, "the fused latent rollout serves the attention-free decoder");
  G2V_REQUIRE((w->bn_running_mean == nullptr) == (w->bn_running_var == nullptr), "BatchNorm running statistics: both or neither");
  G2V_REQUIRE(w->w_pre && w->b_pre && w->bn_w && w->bn_b && w->w_ih0 && w->w_hh0 && w->b_ih0 && w->b_hh0 && w->w_ih1 && w->w_hh1 &&
              w->b_ih1 && w->b_hh1 && w->w_out && w->b_out, "missing weight");
  G2V_REQUIRE(s->ec && s->u && s->a && s->bn_stats && s->h0 && s->h1 && s->gates0 && s->gates1 && s->logits && s->bn_partial,
              "missing state buffer");
  G2V_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "bad dropout probability");
  const bool drop = keep_l0 && p_drop > 0.f;
  G2V_REQUIRE(!drop || s->x1, "inter-layer dropout: no x1 buffer");
  if (!g2v_latent_rollout_ok(S1, B, H, E, 0)) {
    set_error("g2v_latent_rollout_fwd: shape not served (g2v_latent_rollout_ok)");
    return G2V_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < g2v_latent_rollout_fwd_workspace(H, E)) {
    set_error("g2v_latent_rollout_fwd: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  const void* al[] = {target, h_init, w->b_pre, w->bn_w, w->bn_b, w->b_ih0, w->b_hh0, w->b_ih1, w->b_hh1, w->b_out, s->ec, s->u, s->a,
                      s->h0, s->h1, s->x1, s->gates0, s->gates1, s->logits, s->bn_partial, keep_l0, workspace};
  for (const void* p : al) G2V_REQUIRE(ct_al16(p), "16-byte alignment");
  hipStream_t st = (hipStream_t)stream;
  // ---- pack the weights into MFMA fragment order (one launch) ----
  float* p = (float*)workspace;
  PackBatch pb;
  CodePackF pk{};
  pb.n = 0;
  pb.d[pb.n++] = PackDesc{w->w_pre, p, H, 1, 0, E, E, 0, 0}; pk.pre = p; p += pack_floats(H, 1, E);
  pb.d[pb.n++] = PackDesc{w->w_ih0, p, H, 3, H, H, H, 0, 0}; pk.ih0 = p; p += pack_floats(H, 3, H);
  pb.d[pb.n++] = PackDesc{w->w_hh0, p, H, 3, H, H, H, 0, 0}; pk.hh0 = p; p += pack_floats(H, 3, H);
  pb.d[pb.n++] = PackDesc{w->w_ih1, p, H, 3, H, H, H, 0, 0}; pk.ih1 = p; p += pack_floats(H, 3, H);
  pb.d[pb.n++] = PackDesc{w->w_hh1, p, H, 3, H, H, H, 0, 0}; pk.hh1 = p; p += pack_floats(H, 3, H);
  pb.d[pb.n++] = PackDesc{w->w_out, p, E, 1, 0, H, H, 0, ct_ktiles_alloc(E)}; pk.out = p;
  launch_pack(pb, st);
  G2V_CHECK_LAUNCH();
  const int scratch = ct_scratch((size_t)ct_fwd_lds(H, E, 0, 0).total);
  CodeDims dm{S1, B, H, E, E, 0, drop ? p_drop : 0.f, n_pre, 1, cdiv(B, 16), 0, scratch};
  const size_t lds = (size_t)ct_fwd_lds(H, E, 0, scratch).total * sizeof(float);
  if (!g2v_internal_lds_reserve((const void*)latent_step_fwd_kernel, lds)) return G2V_ERR_LAUNCH;
  for (int j = 0; j <= S1; ++j)
    hipLaunchKernelGGL(latent_step_fwd_kernel, dim3(dm.nblk), dim3(CT_NTHR), lds, st, target, h_init, *w, pk, *s,
                       drop ? keep_l0 : nullptr, dm, j);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

// ---- backward workspace layout (bytes, every region 256-byte aligned) ----------------------------------------------------
struct LtBwdWs {
  size_t pack, dgi0, dgh0, dgi1, dgh1, dbn, du, dy, bn_part, bn_sums, wg, total;
};
static LtBwdWs lt_bwd_ws(int S1, int B, int H, int E) {
  const size_t M = (size_t)S1 * B, G = 3 * (size_t)H, nblk = cdiv(B, 16);
  LtBwdWs l;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += al256(bytes); return at; };
  l.pack = take((pack_floats(H, 1, E) + 4 * pack_floats(H, 1, 3 * H) + pack_floats(E, 1, H)) * 4);
  l.dgi0 = take(M * G * 4); l.dgh0 = take(M * G * 4); l.dgi1 = take(M * G * 4); l.dgh1 = take(M * G * 4);
  l.dbn = take(M * H * 4);
  l.du = take(M * H * 4);
  l.dy = take(M * E * 4);
  l.bn_part = take((size_t)S1 * nblk * 2 * H * 4);
  l.bn_sums = take((size_t)S1 * 2 * H * 4);
  size_t wg = 4 * g2v_linear_bwd_weight_workspace((int)M, H, 3 * H);
  wg = wg > g2v_linear_bwd_weight_workspace((int)M, H, E) ? wg : g2v_linear_bwd_weight_workspace((int)M, H, E);
  wg = wg > g2v_linear_bwd_weight_workspace((int)M, E, H) ? wg : g2v_linear_bwd_weight_workspace((int)M, E, H);
  l.wg = take(wg);
  l.total = o;
  return l;
}
extern "C" size_t g2v_latent_rollout_bwd_workspace(int S1, int B, int H, int E) {
  if (S1 < 1 || B < 1 || H < 1 || E < 1) return 0;
  return lt_bwd_ws(S1, B, H, E).total;
}

extern "C" int g2v_latent_rollout_bwd(const float* d_out, const g2v_code_dec_weights* w, const g2v_code_dec_saved* s,
                                      const g2v_code_dec_grads* g, const uint8_t* keep_l0, float p_drop, int n_pre, int S1, int B,
                                      int H, int E, void* workspace, size_t workspace_bytes, g2v_stream_t stream) {
  G2V_REQUIRE(d_out && w && s && g && workspace, "null pointer");
  G2V_REQUIRE(!w->w_attn, "the fused latent rollout serves the attention-free decoder");
  G2V_REQUIRE(w->w_pre && w->bn_w && w->w_ih0 && w->w_hh0 && w->w_ih1 && w->w_hh1 && w->w_out, "missing weight");
  G2V_REQUIRE(s->ec && s->u && s->a && s->bn_stats && s->h0 && s->h1 && s->gates0 && s->gates1, "missing saved buffer");
  G2V_REQUIRE(g->d_hidden0 && g->d_w_pre && g->d_b_pre && g->d_bn_w && g->d_bn_b && g->d_w_ih0 && g->d_w_hh0 && g->d_b_ih0 &&
              g->d_b_hh0 && g->d_w_ih1 && g->d_w_hh1 && g->d_b_ih1 && g->d_b_hh1 && g->d_w_out && g->d_b_out, "missing gradient buffer");
  const bool drop = keep_l0 && p_drop > 0.f;
  G2V_REQUIRE(!drop || s->x1, "inter-layer dropout: x1 was not saved");
  if (!g2v_latent_rollout_ok(S1, B, H, E, 0)) {
    set_error("g2v_latent_rollout_bwd: shape not served (g2v_latent_rollout_ok)");
    return G2V_ERR_UNSUPPORTED;
  }
  const LtBwdWs L = lt_bwd_ws(S1, B, H, E);
  if (workspace_bytes < L.total) {
    set_error("g2v_latent_rollout_bwd: workspace too small");
    return G2V_ERR_WORKSPACE;
  }
  const void* al[] = {workspace, d_out, g->d_hidden0, w->bn_w, s->u, s->a, s->bn_stats, s->h0, s->h1, s->gates0, s->gates1, keep_l0};
  for (const void* p : al) G2V_REQUIRE(ct_al16(p), "16-byte alignment");
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)workspace;
  const int G = 3 * H, M = S1 * B;
  // ---- transposed packs ----
  float* p = (float*)(base + L.pack);
  PackBatch pb;
  CodeBwdArgs a{};
  pb.n = 0;
  pb.d[pb.n++] = PackDesc{w->w_out, p, H, 1, 0, E, H, 1, 0}; a.tw.out_t = p; p += pack_floats(H, 1, E);      // rows f, k = e: W_out[e][f]
  pb.d[pb.n++] = PackDesc{w->w_ih0, p, H, 1, 0, G, H, 1, 0}; a.tw.ih0_t = p; p += pack_floats(H, 1, G);
  pb.d[pb.n++] = PackDesc{w->w_hh0, p, H, 1, 0, G, H, 1, 0}; a.tw.hh0_t = p; p += pack_floats(H, 1, G);
  pb.d[pb.n++] = PackDesc{w->w_ih1, p, H, 1, 0, G, H, 1, 0}; a.tw.ih1_t = p; p += pack_floats(H, 1, G);
  pb.d[pb.n++] = PackDesc{w->w_hh1, p, H, 1, 0, G, H, 1, 0}; a.tw.hh1_t = p; p += pack_floats(H, 1, G);
  const float* pre_t = p;                                                                                     // rows e, k = f: W_pre[f][e]
  pb.d[pb.n++] = PackDesc{w->w_pre, p, E, 1, 0, H, E, 1, 0};
  launch_pack(pb, st);
  G2V_CHECK_LAUNCH();
  a.d_logits = d_out; a.w = *w; a.sv = *s; a.keep_l0 = drop ? keep_l0 : nullptr;
  a.dgi0 = (float*)(base + L.dgi0); a.dgh0 = (float*)(base + L.dgh0); a.dgi1 = (float*)(base + L.dgi1); a.dgh1 = (float*)(base + L.dgh1);
  a.dbn = (float*)(base + L.dbn); a.du = (float*)(base + L.du);
  a.bn_part = (float*)(base + L.bn_part); a.bn_sums = (float*)(base + L.bn_sums); a.d_hidden0 = g->d_hidden0;
  float* dy = (float*)(base + L.dy);
  const int Hp = (H + 15) & ~15;
  const int scratch = (2 * Hp + 2048 <= 16 * (((3 * H + 15) & ~15) + 4)) ? 2048 : 1024;      // (Part A's reduction scratch lives in Gh)
  CodeDims dm{S1, B, H, E, E, 0, drop ? p_drop : 0.f, n_pre, 1, cdiv(B, 16), 0, scratch};
  const size_t lds = (size_t)ct_bwd_lds(H, E).total * sizeof(float);
  if (!g2v_internal_lds_reserve((const void*)latent_step_bwd_kernel, lds)) return G2V_ERR_LAUNCH;
  for (int t = S1 - 1; t >= -1; --t)
    hipLaunchKernelGGL(latent_step_bwd_kernel, dim3(dm.nblk), dim3(CT_NTHR), lds, st, a, dm, t, pre_t, dy);
  hipLaunchKernelGGL(code_small_sums_kernel, dim3(1), dim3(256), 0, st, a.bn_sums, S1, H, g->d_bn_w, g->d_bn_b, (const float*)nullptr,
                     dm.nblk, (float*)nullptr);
  G2V_CHECK_LAUNCH();
  // ---- every weight gradient: one launch over the S1 x B rows each ---------------------------------------------------------
  void* wgws = base + L.wg;
  const size_t wgn = L.total - L.wg;
  int rc;
  if ((rc = g2v_linear_bwd_weight(dy, E, s->h1 + (size_t)B * H, H, 0, 0, 0, nullptr, 1.0f, g->d_w_out, g->d_b_out, M, H, E, 0, wgws, wgn,
                                  stream)) != G2V_OK)
    return rc;
  if ((rc = g2v_linear_bwd_weight(a.du, H, s->ec, E, 0, 0, 0, nullptr, 1.0f, g->d_w_pre, g->d_b_pre, M, E, H, 0, wgws, wgn, stream)) !=
      G2V_OK)
    return rc;
  g2v_wgrad_item it[4];
  const float* x1 = drop ? s->x1 : s->h0 + (size_t)B * H;     // layer 1's input: dropped h0_{t+1}
  it[0] = g2v_wgrad_item{a.dgi0, s->a, g->d_w_ih0, g->d_b_ih0};
  it[1] = g2v_wgrad_item{a.dgh0, s->h0, g->d_w_hh0, g->d_b_hh0};
  it[2] = g2v_wgrad_item{a.dgi1, x1, g->d_w_ih1, g->d_b_ih1};
  it[3] = g2v_wgrad_item{a.dgh1, s->h1, g->d_w_hh1, g->d_b_hh1};
  return g2v_linear_bwd_weight_batch(it, 4, G, H, M, H, G, 0, wgws, wgn, stream);
}
