/* g2v.h -- C-ABI of the MI355X-native Gesture2Vec hot path (libg2v_hip.so).
 *
 * The reference (pjyazdian/Gesture2Vec) is pure Python on PyTorch: it has no FFI / plugin
 * boundary of its own.  The boundary it DOES have is the Python operator
 * surface (scripts/model/ classes, scripts/train_eval/train_seq2seq.py functions); each
 * entry point below names the reference call site whose arithmetic it replaces.  The Python
 * host in gesture2vec_amd/ binds these with ctypes (INTEGRATION.md shows the stub) and exposes
 * the reference's own class / function names on top.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory (PyTorch-ROCm allocations);
 *     the library never allocates, frees, synchronises or touches the default stream;
 *   - `stream` is a hipStream_t passed as void*; all work is stream-ordered, capture-safe
 *     (hipGraph), re-entrant per stream;
 *   - return value: 0 = success, negative = G2V_ERR_*; g2v_last_error() gives a message;
 *   - all arithmetic is IEEE fp32 (MFMA v_mfma_f32_16x16x4_f32 = exact fp32 fma chains);
 *     code indices are int64 (the reference's torch.argmin dtype), masks are uint8 keep-masks;
 *   - matrices are row-major; "ld" = row stride in elements;
 *   - sequence tensors are (T,B,F) "time-major" unless stated.
 */
#ifndef G2V_H
#define G2V_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* g2v_stream_t; /* hipStream_t */
#define G2V_HOST /* host memory; every untagged pointer is device memory or a caller-owned struct */

#define G2V_OK 0
#define G2V_ERR_ARG (-1)         /* bad argument (null pointer, non-positive size, misalignment) */
#define G2V_ERR_LAUNCH (-2)      /* hipLaunch / runtime error */
#define G2V_ERR_WORKSPACE (-3)   /* workspace too small */
#define G2V_ERR_UNSUPPORTED (-4) /* configuration outside what the kernels implement */

const char* g2v_version(void);
const char* g2v_last_error(void);
/* 1 when a gfx950 device is visible to this process, else 0 (never throws). */
int g2v_device_ok(void);

/* ------------------------------------------------------------------------------------------
 * Dense layers.  Replaces nn.Linear call sites on the path:
 *   EncoderRNN.in_layer            model/Autoencoder_VQVAE_model.py:93
 *   VQ_Payam_EMA.pre_linear        model/Autoencoder_VQVAE_model.py:1230
 *   GRU input projections          (nn.GRU internals, :94, text2embedding_model.py:131)
 *   DAE_Network encoder/decoder    model/DAE_model.py:107-110
 * y[m, n] = act( sum_k xin[m, k] * w[n, k] + bias[n] ),  xin = x * keep * x_scale (keep optional)
 * Row m of x is read at  x + (m / rows_inner) * stride_outer + (m % rows_inner) * stride_inner
 * when rows_inner > 0 (lets a (B,T,D) tensor be consumed in (T,B) row order without a copy),
 * else at x + m * ldx.  x_keep (uint8, may be NULL) is indexed [m * K + k].
 * act: 0 = identity, 1 = ReLU, 2 = tanh.
 * ------------------------------------------------------------------------------------------ */
/* LEGACY FORWARD = g2v_ctx_set_option(NULL, G2V_OPT_SMALLM_ROWS, rows) (measurement only): largest row count served by the
 * wave-per-tile kernel of g2v_linear_fwd / g2v_linear_bwd_data (0 = never); returns the previous value, rows < 0 only queries */
int g2v_linear_set_smallm_rows(int rows);
/* IMPLEMENTATION SWITCHES, complete list (everything else is per call).  The library reads NO environment variable.  All of
 * them select between implementations that produce the same results (measurements, parity tests, and the fall-back after a latched
 * residency fault of the persistent kernels):
 *   G2V_OPT_SMALLM_ROWS   row count up to which the wave-per-tile dense kernels are used (default 1024)
 *   G2V_OPT_PERSISTENT    0..3: persistent rollout kernels vs one launch per step (default 1; levels: see g2v_dec_rollout_set_persistent)
 *   G2V_OPT_GRU_CLUSTER   0 / 1: small-batch g2v_gru_seq_fwd / _bwd as one persistent launch vs one launch per step
 *   G2V_OPT_GRU_RESIDENT_ROWS   batch rows from which g2v_gru_seq_fwd (192 < H <= 208) and g2v_gru_seq_bwd (H = 200) keep W_hh
 *                         resident in each CU's registers + LDS for the whole sequence instead of streaming it from L2 every step
 *                         (default 1025: every batch beyond the small-batch cluster kernels; 0 = never).  Forward: bitwise the
 *                         streaming kernel's results; BPTT: equal to summation order
 *   G2V_OPT_GRU_RESIDENT_BWD    0 / 1 (default 1): the BPTT too.  A resident launch takes a CU's whole LDS and register file, so
 *                         nothing co-resides with it: a caller that runs other launches BESIDE the BPTT (the VQ-VAE engine: the
 *                         decoder's weight gradients on other queues) turns it off in its context
 *   G2V_OPT_PRECLEAR_NOTES      READ-ONLY (set: G2V_ERR_ARG): the live "already clear" notes of g2v_cluster_exchange_preclear in the context
 * They live in a CALLER-OWNED CONTEXT (round 6; until round 5 they were process-global variables, so two engines in one
 * process shared them and a fault in one switched off the fast path of the other):
 *   g2v_ctx_create()              a context with the defaults above (host memory; NULL on allocation failure)
 *   g2v_ctx_destroy(ctx)          (unbinds it from the calling thread if bound there; never destroy a context bound elsewhere)
 *   g2v_ctx_bind(ctx)             binds it to the CALLING THREAD and returns the previous binding; NULL = the process's default
 *                                 context.  Every entry point of this library reads the switches of the calling thread's bound
 *                                 context at call time -- launches already captured in a hipGraph keep what they were captured with.
 *   g2v_ctx_set_option(ctx, option, value) / g2v_ctx_get_option(ctx, option)
 *                                 ctx = NULL: the calling thread's bound context (the default context if none).  set returns the
 *                                 previous value; both return G2V_ERR_ARG (< 0) for an unknown option.  Setting
 *                                 G2V_OPT_PERSISTENT or G2V_OPT_GRU_CLUSTER voids the "already clear" notes of THAT context.
 * g2v_linear_set_smallm_rows, g2v_dec_rollout_set_persistent and g2v_gru_seq_set_cluster are LEGACY FORWARDS (ctx = NULL).
 * A thread that never binds a context behaves as before (one set of switches per process, in the default context).
 * What stays process-wide: one device-side error latch, g2v_dec_rollout_persist_fault (below) -- a fault of the DEVICE, not an
 * option.  (The "already clear" notes of g2v_cluster_exchange_preclear belong to the bound context too.) */
typedef struct g2v_ctx g2v_ctx;
#define G2V_OPT_PERSISTENT 1
#define G2V_OPT_GRU_CLUSTER 2
#define G2V_OPT_SMALLM_ROWS 3
#define G2V_OPT_GRU_RESIDENT_ROWS 4
#define G2V_OPT_GRU_RESIDENT_BWD 5
#define G2V_OPT_PRECLEAR_NOTES 6
g2v_ctx* g2v_ctx_create(void);
void g2v_ctx_destroy(g2v_ctx* ctx);
g2v_ctx* g2v_ctx_bind(g2v_ctx* ctx);
int g2v_ctx_set_option(g2v_ctx* ctx, int option, int value);
int g2v_ctx_get_option(const g2v_ctx* ctx, int option);
int g2v_linear_fwd(const float* x, int64_t ldx, int rows_inner, int64_t stride_outer, int64_t stride_inner,
                   const uint8_t* x_keep, float x_scale,
                   const float* w, const float* bias, float* y, int64_t ldy,
                   int M, int K, int N, int act, g2v_stream_t stream);

/* Two linear layers in a row composed into one, for two second layers p = 0, 1 on the same first layer:
 *     wc_p = w_p w_in ([G][D]),  bc_p = w_p b_in + b_p ([G])     (w_p: [G][H], w_in: [H][D])
 * so that (x w_in^T + b_in) w_p^T + b_p = x wc_p^T + bc_p: EncoderRNN.in_layer :93 straight into the bidirectional nn.GRU's input
 * projections :94 at the shipped dims (pose dim < hidden_size): D / H of the arithmetic, equal to the two-layer form to rounding.
 * The caller then never forms the first layer's output (its gradients: g2v_linear_bwd_weight_fold2 / _chain2). */
int g2v_linear_compose2(const float* w0, const float* b0, const float* w1, const float* b1, const float* w_in, const float* b_in,
                        float* wc0, float* bc0, float* wc1, float* bc1, int G, int H, int D, g2v_stream_t stream);

/* y_a = act(x w_a^T + bias_a), y_b = act(x w_b^T + bias_b) (plain rows, no mask; y_a / y_b share ldy): the input projections of
 * the two directions of a bidirectional nn.GRU layer (ref Autoencoder_VQVAE_model.py:94: weight_ih_l0 / weight_ih_l0_reverse on
 * the same input) in ONE launch where that pays (small row counts); results bitwise those of two g2v_linear_fwd calls. */
int g2v_linear_fwd_pair(const float* x, int64_t ldx, const float* w_a, const float* bias_a, float* y_a, const float* w_b,
                        const float* bias_b, float* y_b, int64_t ldy, int M, int K, int N, int act, g2v_stream_t stream);

/* y_a = x w_a^T + bias_a (M x N_a, row stride ldya), y_b = x w_b^T + bias_b (M x N_b, ldyb): two g2v_linear_fwd calls on the same
 * rows -- a decode step of Part d with attention multiplies the new top state twice, for the logits (out :389-391) and for the
 * next step's attention query (attn :173-185).  One launch at small row counts (bitwise the two calls), two otherwise. */
int g2v_linear_fwd_dual(const float* x, int64_t ldx, const float* w_a, const float* bias_a, float* y_a, int64_t ldya, int N_a,
                        const float* w_b, const float* bias_b, float* y_b, int64_t ldyb, int N_b, int M, int K,
                        g2v_stream_t stream);

/* dx[m, k] (+)= sum_n dy[m, n] * w[n, k]      (w is the forward weight, [N][K] row-major) */
int g2v_linear_bwd_data(const float* dy, int64_t lddy, const float* w, float* dx, int64_t lddx,
                        int M, int K, int N, int accumulate, g2v_stream_t stream);

/* Which kernel a forward / data-gradient product above runs on: ONE decision (dense_plan, csrc/linear.hip; DESIGN.md section 3.6.2 has
 * the measurement behind every row count), asked by the four entry points (host arithmetic only, no launch).  The first row that
 * matches decides; C is the contraction length and O the output columns (forward: C = K, O = N; data gradient: C = N, O = K),
 * "float4 rows": no row map, C % 4 == 0, ldx % 4 == 0 and ALIGN_X:
 *   SMALLM   float4 rows, M <= smallm_rows, a keep mask only with ALIGN_KEEP, and for the forward ALIGN_W: one wave per 16 x 16 tn
 *            output tile; variant tn = 1 / 2 / 4 while the 16 x 16 tiles number <= 2048 / <= 8192 / more
 *   STREAM   float4 rows, no keep mask, M >= 1024, (C, O) in {(64, 192), (192, 64), (128, 128), (64, 64)} (C rounded up to 16),
 *            act != 2, ALIGN_Y with ldy % 4 == 0, a bias only with ALIGN_BIAS (the weights' alignment is not asked): the streaming
 *            kernel; variant = O / 16 << 4 | ceil(C / 16)
 *   K4       forward, no keep mask, K == 135, N == 64, M >= 4096, M % 16 == 0, act != 2, ALIGN_Y with ldy % 4 == 0, a bias only
 *            with ALIGN_BIAS: the kernel of unaligned 135-float rows; variant 1 with a row map
 *   TILED    everything else: the LDS-tiled kernel; variant 4 (float4 operand loads) without a keep mask when K % 4 == 0 (data
 *            gradient: and N % 4 == 0), ALIGN_X, ALIGN_W and ldx % 4 == 0 (row map: both strides % 4 == 0), variant 1 otherwise
 * forms FWD_PAIR / FWD_DUAL answer for the single g2v_linear_fwd call on (M, K, N) and add G2V_DENSE_ROUTE_ONE_LAUNCH where the
 * entry point runs both products in one launch: pair on TILED*4 with N > 192 and M <= 16384; dual where N and N_b are both SMALLM
 * with tn = 1.  Otherwise they are two g2v_linear_fwd calls, each planned from its own pointers.
 * g2v_linear_route returns G2V_DENSE_ROUTE_* in bits 0-7, the variant in bits 8-15 and ONE_LAUNCH above, or 0 for a refused call
 * (a size <= 0, act outside 0..2, an unknown form).  K, N: the weight is [N][K] in every form; ldx / ldy: row strides of the array
 * read (x, dy) and written (y, dx); what a form's entry point has no argument for is ignored (N_b outside FWD_DUAL; act, bias, keep
 * and row map of BWD_DATA; keep and row map of the pair and dual forms, whose ALIGN_W speaks of both weights).  smallm_rows: -1 =
 * the bound context's G2V_OPT_SMALLM_ROWS; align: an or of G2V_DENSE_ALIGN_*.  A function of its arguments alone otherwise. */
#define G2V_DENSE_FORM_FWD 0
#define G2V_DENSE_FORM_BWD_DATA 1
#define G2V_DENSE_FORM_FWD_PAIR 2
#define G2V_DENSE_FORM_FWD_DUAL 3
#define G2V_DENSE_ROUTE_SMALLM 1
#define G2V_DENSE_ROUTE_STREAM 2
#define G2V_DENSE_ROUTE_K4 3
#define G2V_DENSE_ROUTE_TILED 4
#define G2V_DENSE_ROUTE_ONE_LAUNCH 65536
#define G2V_DENSE_ALIGN_X 1         /* x (dy) is 16-byte aligned */
#define G2V_DENSE_ALIGN_W 2         /* w is */
#define G2V_DENSE_ALIGN_Y 4         /* y (dx) is */
#define G2V_DENSE_ALIGN_BIAS 8      /* bias is */
#define G2V_DENSE_ALIGN_KEEP 16     /* the keep mask is 4-byte aligned */
int g2v_linear_route(int form, int M, int K, int N, int N_b, int act, int has_bias, int has_keep, int rows_inner,
                     int64_t stride_outer, int64_t stride_inner, int64_t ldx, int64_t ldy, int smallm_rows, int align);

/* dw[n, k] (+)= sum_m dy[m, n] * xin[m, k];  db[n] (+)= sum_m dy[m, n]  (db may be NULL).
 * xin addressing / keep-mask exactly as in g2v_linear_fwd.  Deterministic (split-M slabs + ordered
 * reduction, no float atomics).  workspace >= g2v_linear_bwd_weight_workspace(M,K,N) bytes.
 * `accumulate` is a flag word: bit 0 = add into dw / db; bit 1 (G2V_WGRAD_BF16X3) = allow the products to run on
 * the bf16 matrix pipe as a 3-term split (x = hi + lo; hi*hi + hi*lo + lo*hi, fp32 accumulation, ~1.5e-5 relative per
 * product instead of fp32's 6e-8; db stays exact fp32).  Honoured by the wave-autonomous kernels (large M), ignored
 * elsewhere.  Default (bit clear) is exact fp32 MFMA. */
#define G2V_WGRAD_ACCUMULATE 1
#define G2V_WGRAD_BF16X3 2

/* Up to 4 weight-gradient problems of ONE shape (same M, K, N, row strides; plain row addressing, no keep mask) in one call:
 * the large-M kernels run them in one launch (their workgroups fill each other's ramp-up / tail) followed by one slab
 * reduction.  workspace >= nprob * g2v_linear_bwd_weight_workspace(M,K,N).  flags as above.  db may be NULL per item. */
typedef struct {
  const float* dy;   /* (M,N), row stride lddy */
  const float* x;    /* (M,K), row stride ldx  */
  float* dw;         /* (N,K) */
  float* db;         /* (N) or NULL */
} g2v_wgrad_item;
int g2v_linear_bwd_weight_batch(const g2v_wgrad_item* items, int nprob, int64_t lddy, int64_t ldx, int M, int K, int N,
                                int flags, void* workspace, size_t workspace_bytes, g2v_stream_t stream);
/* ... with xin row-mapped as in g2v_linear_fwd (rows_inner / stride_outer / stride_inner: the (B,T,D) network input read in
 * (T,B) row order), the same map for every item. */
int g2v_linear_bwd_weight_batch_mapped(const g2v_wgrad_item* items, int nprob, int64_t lddy, int64_t ldx, int rows_inner,
                                       int64_t stride_outer, int64_t stride_inner, int M, int K, int N, int flags,
                                       void* workspace, size_t workspace_bytes, g2v_stream_t stream);

/* Deferred slab reductions (round 6).  Every large-M weight-gradient call above is [products into split-M slabs] + [one ordered
 * reduction of the slabs into dw / db]; a chain of such calls on one stream makes every product wait for the reduction in front
 * of it.  g2v_linear_bwd_weight_deferred is the union of the calls above -- nprob = 1: one product; rows_inner > 0: xin
 * row-mapped; dy_b != NULL (nprob = 1): (dy + dy_b)^T xin as g2v_linear_bwd_weight_sum2 -- WITHOUT the reduction: it fills the
 * caller-owned `pending` record, and g2v_linear_bwd_weight_reduce runs the reductions of up to G2V_WGRAD_PENDING_MAX records in
 * ONE launch, wherever the caller places it.  Until then the slabs live in `workspace`: one workspace per pending call (same size
 * rule as the immediate calls).  Results are bitwise those of the immediate calls.  A shape whose path has no slab reduction
 * (small row counts) or needs dw finished at once (ragged row counts) is completed inside the call and leaves `pending` empty
 * (nprob = 0), which g2v_linear_bwd_weight_reduce skips.  No hidden state: the record is plain data owned by the caller. */
#define G2V_WGRAD_PENDING_MAX 8
typedef struct {
  const float* slab_w[4]; float* out_w[4];   /* per problem: split-M slabs of dw (nsplit x n floats) and dw itself */
  const float* slab_b[4]; float* out_b[4];   /* ... of db (nsplit x nb floats), NULL where the item had no db */
  int64_t n, nb;                             /* N * K and N */
  int nsplit, nprob, accumulate, reserved;
} g2v_wgrad_pending;
int g2v_linear_bwd_weight_deferred(const g2v_wgrad_item* items, int nprob, int64_t lddy, int64_t ldx, int rows_inner,
                                   int64_t stride_outer, int64_t stride_inner, const float* dy_b, int M, int K, int N, int flags,
                                   void* workspace, size_t workspace_bytes, g2v_wgrad_pending* pending, g2v_stream_t stream);
int g2v_linear_bwd_weight_reduce(const g2v_wgrad_pending* pending, int count, g2v_stream_t stream);
size_t g2v_linear_bwd_weight_workspace(int M, int K, int N);
/* Which kernel family a weight-gradient call of the family above runs on (host arithmetic only, no launch): one of
 * G2V_WGRAD_ROUTE_*, with G2V_WGRAD_ROUTE_RAGGED_TAIL or-ed in when M % 16 leftover rows are added by a second small launch and
 * the route is that of the M & ~15 main product; 0 for a size or problem count the calls reject and for has_dy_b on a shape
 * g2v_linear_bwd_weight_sum2_ok() rejects.  has_keep / mapped / has_dy_b: the call has a keep mask / rows_inner > 0 / a second
 * addend; align: the largest power of two, up to 16, that divides every dy and x pointer of the call. */
#define G2V_WGRAD_ROUTE_SMALL_LDS 1      /* M <= 4095: LDS-staged, float4 operands */
#define G2V_WGRAD_ROUTE_SMALL_RT 2       /* ... register-tiled, 2 x 2 tiles per workgroup */
#define G2V_WGRAD_ROUTE_SMALL_MASKED 3   /* ... one tile per workgroup, keep mask */
#define G2V_WGRAD_ROUTE_SMALL_WAVES16 4  /* ... one tile per workgroup, 16 waves split the rows */
#define G2V_WGRAD_ROUTE_SMALL_TILE 5     /* ... one tile per workgroup, 4 waves */
#define G2V_WGRAD_ROUTE_WAVE 6           /* M >= 4096: wave-autonomous, slabs */
#define G2V_WGRAD_ROUTE_WAVE_DUAL 7      /* ... its two-addend form */
#define G2V_WGRAD_ROUTE_WAVE_GEN 8       /* ... output-blocked */
#define G2V_WGRAD_ROUTE_LDS_TILED 9      /* everything else: LDS-tiled split kernel, slabs */
#define G2V_WGRAD_ROUTE_RAGGED_TAIL 256
int g2v_linear_bwd_weight_route(int M, int K, int N, int nprob, int flags, int has_keep, int mapped, int has_dy_b, int64_t lddy,
                                int64_t ldx, int align);
/* The weight gradient of a layer y = x W_in^T + b_in (W_in: [H][D]) that feeds TWO layers g_p = y W_p^T (W_p: [G][H]; the two
 * directions' input projections of the bidirectional encoder GRU, ref Autoencoder_VQVAE_model.py:447-464 + EncoderRNN.in_layer
 * :93), from the weight-gradient-shaped products p_p = dg_p^T x ([G][D]) and c_p = column sums of dg_p ([G]) -- both are what
 * g2v_linear_bwd_weight(_batch)(dy = dg_p, x) returns as dw / db:
 *     dw[h][d] (+)= sum_g w0[g][h] p0[g][d] + sum_g w1[g][h] p1[g][d],    db[h] (+)= sum_g w0[g][h] c0[g] + sum_g w1[g][h] c1[g]
 * = autograd's dW_in = (dg_0 W_0 + dg_1 W_1)^T x re-associated (equal to summation order): the (M x H) gradient of y, which
 * nothing else reads when x is the network's input, is never formed -- D / H of its arithmetic.  Deterministic. */
int g2v_linear_bwd_weight_fold2(const float* w0, const float* w1, const float* p0, const float* p1, const float* c0,
                                const float* c1, float* dw, float* db, int G, int H, int D, int accumulate, g2v_stream_t stream);
/* ... and the weight gradients of those two layers themselves, dW_p = dg_p^T y with y = x W_in^T + b_in, from the same p_p, c_p:
 *     dw_p[g][h] (+)= sum_d p_p[g][d] w_in[h][d] + c_p[g] b_in[h]        (w_in: [H][D], b_in: [H], dw_p: [G][H])
 * = autograd's dW_ih = dgi^T in_layer(x) re-associated (ref EncoderRNN: in_layer :93 straight into the GRU :94); db_p = c_p.  A
 * (G x D)(D x H) product instead of (G x M)(M x H).  Deterministic. */
int g2v_linear_bwd_weight_chain2(const float* p0, const float* p1, const float* c0, const float* c1, const float* w_in,
                                 const float* b_in, float* dw0, float* dw1, int G, int H, int D, int accumulate, g2v_stream_t stream);
/* Both of the above (overwrite form) in ONE launch -- they read the same p, c and nothing of each other; bitwise their results. */
int g2v_linear_bwd_weight_fold_chain2(const float* w0, const float* w1, const float* p0, const float* p1, const float* c0,
                                      const float* c1, const float* w_in, const float* b_in, float* dw_in, float* db_in,
                                      float* dw0, float* dw1, int G, int H, int D, g2v_stream_t stream);
/* dw = (dy_a + dy_b)^T x (+ db = column sums of dy_a + dy_b): the addends are summed as the operand fragments are used --
 * the arithmetic of "add, then g2v_linear_bwd_weight" without the add pass.  The encoder's input layer uses it: its dx
 * arrives as one array per GRU direction (ref Autoencoder_VQVAE_model.py:447-464, the bidirectional nn.GRU's input
 * gradient).  Served for dW shapes of 4 x 9 tiles (64 x 135) with M % 16 == 0 above the small-M threshold:
 * g2v_linear_bwd_weight_sum2_ok() says so, G2V_ERR_UNSUPPORTED otherwise.  Row addressing of x and workspace as for
 * g2v_linear_bwd_weight. */
int g2v_linear_bwd_weight_sum2_ok(int M, int K, int N);
int g2v_linear_bwd_weight_sum2(const float* dy_a, const float* dy_b, int64_t lddy, const float* x, int64_t ldx, int rows_inner,
                               int64_t stride_outer, int64_t stride_inner, float* dw, float* db, int M, int K, int N,
                               int accumulate, void* workspace, size_t workspace_bytes, g2v_stream_t stream);
int g2v_linear_bwd_weight(const float* dy, int64_t lddy,
                          const float* x, int64_t ldx, int rows_inner, int64_t stride_outer, int64_t stride_inner,
                          const uint8_t* x_keep, float x_scale,
                          float* dw, float* db, int M, int K, int N, int accumulate,
                          void* workspace, size_t workspace_bytes, g2v_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Vector quantiser.  Replaces VQ_Payam_EMA.forward / its autograd
 * (model/Autoencoder_VQVAE_model.py:1217-1296), also VQ_Payam (:1114-1173) and the
 * code-assignment call sites (data_loader/lmdb_data_loader.py:1274-1281, Clustering.py:151-157).
 *
 * g2v_vq_assign_fwd   K1+K2+K5:  d = ||x||^2 + ||W||^2 - 2 x W^T  (x = flat rows, fp32 MFMA),
 *                     idx = argmin_k d (lowest index on ties), q = W[idx],
 *                     quantized = z + (q - z), sse_partial[block] = sum (q - z)^2.
 *   flat      (N,E) rows the distances are computed from (pre_linear(z) for the EMA variant, :1230)
 *   z         (N,E) raw rows used for the loss and the straight-through output (:1285,1292)
 *   codebook  (K,E);  code_sqnorm (K) = sum_e W^2  (from g2v_vq_code_sqnorm)
 *   idx (N) int64 out; quantized (N,E) out (may be NULL); dist_min (N) out (may be NULL);
 *   sse_partial (g2v_vq_assign_blocks(N)) out (may be NULL when quantized is NULL).
 * ------------------------------------------------------------------------------------------ */
int g2v_vq_assign_blocks(int N);
int g2v_vq_code_sqnorm(const float* codebook, float* code_sqnorm, int K, int E, g2v_stream_t stream);
int g2v_vq_assign_fwd(const float* flat, const float* z, const float* codebook, const float* code_sqnorm,
                      int64_t* idx, float* quantized, float* dist_min, float* sse_partial,
                      int N, int E, int K, g2v_stream_t stream);

/* Which kernel a code assignment runs on: ONE decision (vq_route_plan, csrc/vq.hip; DESIGN.md section 3.5.1 has the measurement behind
 * every row count), asked by the entry points below, by their *_ok queries and by the Python dispatchers.  The first row that
 * matches decides ("tuned shape": E == 128 and K % 128 == 0; "aligned": no G2V_VQ_PLAN_UNALIGNED):
 *   form RAW (latents z and pre_linear are given)
 *     BX       wants FULL, tuned shape with K <= 512 (K in {128, 256, 384, 512}), aligned: g2v_vq_fused_assign_bx_fwd
 *     FUSED    wants FULL, any other tuned shape, aligned: g2v_vq_fused_assign_packed_fwd (variant 1), or with
 *              G2V_VQ_PLAN_NO_FRAG g2v_vq_fused_assign_fwd on the codebook in place (variant 0)
 *     BULK_Z   wants IDX_BULK, N >= G2V_VQ_BULK_Z_MIN_ROWS, and the kernels serve it: E == 400, K % 16 == 0, 32 <= K <= 512, N >= 2048,
 *              N > smallm_rows (g2v_linear_fwd takes another kernel up to there: no longer its bits), aligned: g2v_vq_assign_bulk_z
 *     PROJECT  anything else: g2v_linear_fwd, then the ROWS route of the same wants, N, E, K and facts
 *   form ROWS (projected rows flat are given)
 *     BULK     wants IDX_BULK, N >= G2V_VQ_BULK_MIN_ROWS, tuned shape with K <= 8192, aligned: g2v_vq_assign_bulk; variant = bits of a code index
 *     PACKED   N >= G2V_VQ_PACKED_MIN_ROWS, not a tuned shape, no G2V_VQ_PLAN_NO_FRAG, aligned, and the kernel serves it: E % 16 == 0,
 *              K % 16 == 0, 64 rows of E + 4 floats fit the LDS (E <= 608): g2v_vq_pack_codebook + g2v_vq_assign_packed_fwd; variant =
 *              row tiles per workgroup, 4 / 2 / 1 at N >= G2V_VQ_PACKED_NR4_ROWS / >= G2V_VQ_PACKED_NR2_ROWS / below
 *     RT, FAST tuned shape, aligned: g2v_vq_assign_fwd's own kernels, RT (64 rows per workgroup, variant 4) from
 *              G2V_VQ_RT_MIN_ROWS rows, FAST (16 rows, variant 1) below
 *     SPLIT    at most G2V_VQ_SPLIT_MAX_ROW_TILES tiles of 16 rows and at least G2V_VQ_SPLIT_MIN_CODE_TILES tiles of 16 codes: the
 *              codes split over variant = 2 .. 8 workgroups per row tile, then a finishing launch (g2v_vq_assign_fwd)
 *     GENERIC  the rest (g2v_vq_assign_fwd); refused where 16 rows of E floats exceed 160 KB of LDS (E > 2544)
 * G2V_VQ_PLAN_ENTRY: the call came in through a route's own entry point (g2v_vq_assign_packed_fwd for ROWS, g2v_vq_assign_bulk for
 * ROWS + IDX_BULK, g2v_vq_assign_bulk_z for RAW + IDX_BULK): the row counts G2V_VQ_*_MIN_ROWS and PACKED's "not a tuned shape" do not
 * apply, only what the kernels serve, and a shape they do not serve is refused.  g2v_vq_assign_fwd plans with G2V_VQ_PLAN_NO_FRAG.
 * g2v_vq_assign_route returns G2V_VQ_ROUTE_* in bits 0-7 and the variant in bits 8-15, or 0 for a refused call; a PROJECT answer
 * carries the answer of its ROWS route (route and variant) in bits 16-31.  smallm_rows: -1 = the bound context's smallm_max_rows;
 * facts: an or of G2V_VQ_PLAN_*.  A function of its arguments alone otherwise. */
#define G2V_VQ_FORM_ROWS 0
#define G2V_VQ_FORM_RAW 1
#define G2V_VQ_WANTS_FULL 0         /* quantized + SSE partials (and idx) */
#define G2V_VQ_WANTS_IDX 1          /* indices only */
#define G2V_VQ_WANTS_IDX_BULK 2     /* indices only, and the caller supplies a workspace: the screened bulk routes are accepted */
#define G2V_VQ_ROUTE_BX 1
#define G2V_VQ_ROUTE_FUSED 2
#define G2V_VQ_ROUTE_BULK_Z 3
#define G2V_VQ_ROUTE_PROJECT 4
#define G2V_VQ_ROUTE_BULK 5
#define G2V_VQ_ROUTE_PACKED 6
#define G2V_VQ_ROUTE_RT 7
#define G2V_VQ_ROUTE_FAST 8
#define G2V_VQ_ROUTE_SPLIT 9
#define G2V_VQ_ROUTE_GENERIC 10
#define G2V_VQ_PLAN_UNALIGNED 1     /* an array the vector kernels read or write as float4s is not 16-byte aligned */
#define G2V_VQ_PLAN_NO_FRAG 2       /* the caller has no room for a fragment-major codebook image */
#define G2V_VQ_PLAN_ENTRY 4         /* called through the route's own entry point (above) */
#define G2V_VQ_PACKED_MIN_ROWS 2048
#define G2V_VQ_PACKED_NR2_ROWS 8192
#define G2V_VQ_PACKED_NR4_ROWS 32768
#define G2V_VQ_RT_MIN_ROWS 16384
#define G2V_VQ_BULK_Z_MIN_ROWS 32768
#define G2V_VQ_BULK_MIN_ROWS 131072
#define G2V_VQ_SPLIT_MAX_ROW_TILES 64
#define G2V_VQ_SPLIT_MIN_CODE_TILES 8
int g2v_vq_assign_route(int form, int wants, int N, int E, int K, int smallm_rows, int facts);

/* pre_linear + assign in ONE launch (the FUSED row of g2v_vq_assign_route; G2V_ERR_UNSUPPORTED otherwise -> g2v_linear_fwd +
 * g2v_vq_assign_fwd): flat = z w_pre^T + b_pre (:1230) is written to flat_out (the code statistics read it), the
 * distances / argmin use it from LDS, quantized / sse_partial use the raw z as in g2v_vq_assign_fwd. */
/* Bulk code assignment (row f-2: latents of a whole corpus -> code indices, pipeline.chunks_to_codes): idx only, N large.
 * The -2 x W^T contraction runs on the bf16 matrix pipe as a 3-term split (xh.wh + xh.wl + xl.wh, fp32 accumulate); a row
 * whose best and second-best approximate distances are closer than 2^-11 |x| max|w| (more than twice the split's error
 * bound) is assigned again by the exact fp32 kernel of g2v_vq_assign_fwd, so the result is the fp32 argmin
 * (Autoencoder_VQVAE_model.py:1234-1259) at ~5x fewer matrix cycles.  Shapes: the BULK row of g2v_vq_assign_route.  undecided (device int, may be
 * NULL): number of rows that took the exact path. */
size_t g2v_vq_assign_bulk_workspace(int N, int E, int K);
int g2v_vq_assign_bulk(const float* flat, const float* codebook, const float* code_sqnorm, int64_t* idx, int N, int E, int K,
                       void* workspace, size_t workspace_bytes, int* undecided, g2v_stream_t stream);
/* Bulk code assignment from RAW latents at the checkpoints' width (the BULK_Z row of g2v_vq_assign_route): idx = argmin_k
 * |z w_pre^T + b_pre - codebook[k]|^2 without writing the projected rows.  The distances are screened in z-space on the bf16
 * matrix pipe (u_k = w_pre^T w_k, 3-term hi / lo split); a row whose winner does not clear every other code by the per-code
 * error radius is recomputed with the arithmetic of g2v_linear_fwd (tiled kernel) + g2v_vq_assign_packed_fwd, so idx is
 * bitwise that route's at the same N (ties: lowest index; non-finite rows or codes included).  code_sqnorm must be
 * g2v_vq_code_sqnorm's.  _ok: 1 where a call through this entry point is served (G2V_VQ_PLAN_ENTRY, the bound context's smallm_max_rows).
 * undecided (device int, may be NULL): number of rows that took the exact path. */
int g2v_vq_assign_bulk_z_ok(int N, int E, int K);
size_t g2v_vq_assign_bulk_z_workspace(int N, int E, int K);
int g2v_vq_assign_bulk_z(const float* z, const float* w_pre, const float* b_pre, const float* codebook, const float* code_sqnorm,
                         int64_t* idx, int N, int E, int K, void* workspace, size_t workspace_bytes, int* undecided,
                         g2v_stream_t stream);
int g2v_vq_fused_assign_fwd(const float* z, const float* w_pre, const float* b_pre, const float* codebook,
                            const float* code_sqnorm, float* flat_out, int64_t* idx, float* quantized,
                            float* sse_partial, int N, int E, int K, g2v_stream_t stream);
/* The same launch reading the codebook's MFMA fragments from a fragment-major image (coalesced 1 KB runs instead of 16
 * half-used cache lines per wave-level load; 14.6 -> 12.8 us at N = 4096, K = 512).  g2v_vq_pack_codebook writes the image
 * ([K/16][E/16][64][4] floats, K * E in all) and has to be called whenever the codebook changed (after g2v_vq_ema_update);
 * the row-major codebook is still read for the gather of the chosen codes.  Results are bitwise those of
 * g2v_vq_fused_assign_fwd. */
int g2v_vq_pack_codebook(const float* codebook, float* codebook_frag, int K, int E, g2v_stream_t stream);
/* Round 5: g2v_vq_assign_fwd on that image (K * E floats; shapes: the PACKED row of g2v_vq_assign_route, _ok: 1 where a call through
 * this entry point is served) -- the reference's own quantiser
 * shapes, E = hidden_size * n_layers = 400 with K = 512 (config/VQ-VAE.yml) or 400 (VQ-VAE_GENEA.yml), which g2v_vq_assign_fwd
 * serves at 0.22 of the fp32 matrix peak.  Same outputs bit for bit (idx, dist_min, quantized, the SSE partials per 16 rows);
 * eight waves per workgroup, 1 / 2 / 4 row tiles per workgroup (bulk assignment: every fragment feeds all of them). */
int g2v_vq_assign_packed_ok(int N, int E, int K);
int g2v_vq_assign_packed_fwd(const float* flat, const float* z, const float* codebook, const float* codebook_frag,
                             const float* code_sqnorm, int64_t* idx, float* quantized, float* dist_min, float* sse_partial,
                             int N, int E, int K, g2v_stream_t stream);
int g2v_vq_fused_assign_packed_fwd(const float* z, const float* w_pre, const float* b_pre, const float* codebook,
                                   const float* codebook_frag, const float* code_sqnorm, float* flat_out, int64_t* idx,
                                   float* quantized, float* sse_partial, int N, int E, int K, g2v_stream_t stream);
/* The north-star form (round 3): pre_linear in fp32 MFMA and, BESIDE it in the same launch, the -2 x W^T contraction SCREENED on
 * the bf16 matrix pipe in z-space: flat.w_k = z.u_k + b.w_k with u_k = w_pre^T w_k, so e_k = (|w_k|^2 - 2 b.w_k) - 2 (zh + zl).bf16(u_k)
 * (fp32 accumulate, 8 v_mfma_f32_16x16x32_bf16 per 16 x 16 x 128 tile instead of 32 fp32 MFMAs) needs no projected row.  With the
 * per-code radius r_k = 2^-7 (1 + 2^-5) |z||u_k| + 2^-13 |flat|^ |w_k| + 2^-20 (|flat|^^2 + |w_k|^2)  (|flat|^ = |w_pre|_F |z| + |b|; an
 * upper bound of |e_k - (d_k - |flat|^2)| for the fp32 kernel's d_k, derivation in vq.hip) every code with e_k - r_k <= min_j (e_j + r_j)
 * is re-evaluated IN THE SAME LAUNCH with the exact fp32 chain of g2v_vq_fused_assign_fwd on the projected rows, the row's code
 * being the torch.argmin (:1259) of those exact distances: flat_out, idx and quantized are bitwise those of
 * g2v_vq_fused_assign_fwd (sse_partial: the same sum in another order).  A 16-row tile with a non-finite screening value or more
 * than 128 candidates takes the exact fp32 sweep over all K codes instead.  Shapes: the BX row of g2v_vq_assign_route
 * (g2v_vq_fused_assign_bx_ok: 1 where an ideal RAW call that wants FULL runs as BX).
 *   w_pre_frag  g2v_vq_pack_codebook(w_pre, ., E, E): pre_linear's weight as fp32 MFMA fragments (E * E floats)
 *   image       g2v_vq_bx_pack(codebook, code_sqnorm, w_pre, b_pre, ., K, E): bf16 MFMA fragments of U = W w_pre, s'_k, the radius
 *               coefficients (g2v_vq_bx_image_bytes(K, E) bytes); rewrite it whenever the codebook / code_sqnorm / pre_linear changed
 *   diag        device int[4] or NULL: [0] += tiles that took the exact sweep, [1] += (row, candidate) pairs re-evaluated
 *   flags       G2V_VQ_BX_*: explicit per-call switches (no process-global state) */
#define G2V_VQ_BX_EXACT 1      /* every tile takes the exact fp32 sweep: the A/B reference of the screened path */
size_t g2v_vq_bx_image_bytes(int K, int E);
int g2v_vq_bx_pack(const float* codebook, const float* code_sqnorm, const float* w_pre, const float* b_pre, void* image, int K, int E,
                   g2v_stream_t stream);
int g2v_vq_fused_assign_bx_ok(int N, int E, int K);
int g2v_vq_fused_assign_bx_fwd(const float* z, const float* w_pre_frag, const float* b_pre, const float* codebook,
                               const void* image, const float* code_sqnorm, float* flat_out, int64_t* idx, float* quantized,
                               float* sse_partial, int* diag, int N, int E, int K, int flags, g2v_stream_t stream);
/* K3: cnt[k] = #{i: idx[i]=k};  dw[k,:] = sum_{i: idx[i]=k} flat[i,:]   (:1265,1275).
 * Deterministic one-hot^T x flat MFMA contraction (the one-hot is generated on the fly from idx).
 * stats layout: [cnt (K) | dw (K*E)] contiguous fp32, so it can be all-reduced as one buffer. */
size_t g2v_vq_stats_workspace(int N, int E, int K);
int g2v_vq_stats(const int64_t* idx, const float* flat, float* stats /* K + K*E */, int N, int E, int K,
                 void* workspace, size_t workspace_bytes, g2v_stream_t stream);

/* K4 + K5 scalars (:1263-1282, :1285-1294).  In place on ema_cluster_size (K), ema_w (K,E), codebook (K,E):
 *   cs = cs*decay + (1-decay)*cnt; n = sum cs; cs = (cs+eps)/(n+K*eps)*n;
 *   ema_w = ema_w*decay + (1-decay)*dw; codebook = ema_w / cs[:,None]; code_sqnorm refreshed.
 * update = 0 skips the EMA part (eval mode, :1262) and only produces the scalars.
 * scalars out (2 floats): [0] loss = beta * sum(sse_partial) / (N_loss*E), [1] perplexity = exp(-sum p log(p+1e-10)),
 * p = cnt / N_cnt.  N_cnt is the number of rows behind `stats` (global batch under data parallelism). */
int g2v_vq_ema_update(const float* stats, const float* sse_partial, int n_sse_partial,
                      float* ema_cluster_size, float* ema_w, float* codebook, float* code_sqnorm,
                      float* scalars, int N_loss, int N_cnt, int E, int K,
                      float beta, float decay, float eps, int update, g2v_stream_t stream);
/* The same with the weight of the new statistics formed as torch forms the reference's Python scalar: (float)(1.0 - decay) in double,
 * where g2v_vq_ema_update takes 1.0f - (float)decay (9.3e-7 apart at decay 0.99; it shows where a cluster size starts from zero,
 * as the frame-level quantiser of Part a does). */
int g2v_vq_ema_update_exact(const float* stats, const float* sse_partial, int n_sse_partial,
                            float* ema_cluster_size, float* ema_w, float* codebook, float* code_sqnorm,
                            float* scalars, int N_loss, int N_cnt, int E, int K,
                            float beta, double decay, float eps, int update, g2v_stream_t stream);

/* K5': gz = g_quantized + g_loss * 2*beta/(N*E) * (z - W[idx])   (autograd of :1285-1292).
 * g_loss is a device scalar (d total / d loss_vq), g_quantized may be NULL.
 * idx == NULL: `codebook` is instead the dense (N,E) forward output `quantized` (= z + (W[idx]-z)), so the
 * backward does not depend on a codebook that the EMA update has already moved. */
int g2v_vq_bwd(const float* g_quantized, const float* g_loss, const float* z, const float* codebook,
               const int64_t* idx, float* gz, int N, int E, float beta, g2v_stream_t stream);

/* Codebook gradient of the NON-EMA quantiser VQ_Payam (:1114-1173, loss = q_latent + beta*e_latent):
 *   g_codebook[k,:] = g_loss * 2/(N*E) * (cnt[k]*W[k,:] - sum_{i: idx[i]=k} z[i,:])
 * with `stats` = g2v_vq_stats(idx, z).  The gradient wrt z is g2v_vq_bwd (e_latent term only, :1158-1159). */
int g2v_vq_codebook_grad(const float* stats, const float* codebook, const float* g_loss, float* g_codebook,
                         int N, int E, int K, g2v_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Full-sequence GRU direction (K8, K12).  Replaces one direction of one layer of
 * nn.GRU in EncoderRNN (model/Autoencoder_VQVAE_model.py:94, model/text2embedding_model.py:131).
 *   gi (T,B,3H) = x W_ih^T + b_ih (from g2v_linear_fwd), gate order r,z,n (PyTorch)
 *   r = s(gi_r + W_hr h + b_hr); z = s(gi_z + W_hz h + b_hz); n = tanh(gi_n + r*(W_hn h + b_hn)); h' = (1-z) n + z h
 *   lengths (B) int32 or NULL: pack_padded_sequence semantics (rows freeze after their last valid step,
 *   padded outputs are zero, the reverse direction starts at each row's own last step).
 *   hs row (t,b) is written at hs + (t*B + b)*hs_ld  (hs_ld >= H lets both directions share a (T,B,2H) buffer).
 *   gates (T,B,4H) = r,z,n,W_hn h + b_hn  saved for the backward (NULL = inference).
 * ------------------------------------------------------------------------------------------ */
typedef struct {          /* one direction of one layer, forward */
  const float* gi;        /* (T,B,3H) input projections incl. b_ih          */
  const float* w_hh;      /* (3H,H)                                         */
  const float* b_hh;      /* (3H)                                           */
  const float* h0;        /* (B,H) or NULL = zeros                          */
  float* hs;              /* out: hidden states, row (t,b) at hs + (t*B+b)*hs_ld */
  float* h_n;             /* out: (B,H) final state (may be NULL)           */
  float* gates;           /* out: (T,B,4H) saved for backward (NULL = inference) */
  int reverse;            /* 0: t = 0..T-1, 1: t = T-1..0                   */
  /* Fused input projection (gi == NULL): gi_t = x_t W_ih^T + b_ih is computed inside the recurrent kernel, one step
   * ahead of its use (the gi array, its GEMM and its HBM round trip disappear).  The FAST route with in_dim == H only
   * (g2v_gru_seq_route below); otherwise G2V_ERR_UNSUPPORTED and the caller computes gi with g2v_linear_fwd. */
  const float* x;         /* (T,B,in_dim) layer input                       */
  const float* w_ih;      /* (3H,in_dim)                                    */
  const float* b_ih;      /* (3H)                                           */
  int in_dim;
  /* Packed input projections (round 5; NULL = the (T,B,3H) layout): a HOST array of T row offsets.  gi then holds only the
   * positions inside their sequences, step-major: row (t,b) at gi + (gi_row_off[t] + b) * 3H for b < n_t = #{lengths > t}
   * (lengths sorted descending, as pack_padded_sequence(enforce_sorted) requires; gi_row_off[t] = n_0 + ... + n_{t-1}) -- the
   * dense product that makes gi runs over sum(lengths) rows instead of T x B.  Where g2v_gru_seq_packed_ok says so (the rule:
   * g2v_gru_seq_route below); every direction of the call must carry the same offsets.  hs / gates keep the (T,B,.) layout. */
  G2V_HOST const int32_t* gi_row_off;
  /* Gathered input projections (round 6; NULL = off): gi is a TABLE (V, 3H), and row r of the layout above -- r = t * B + b, or
   * gi_row_off[t] + b when packed -- is gi + gi_gather[r] * 3H.  The encoder the reference feeds straight from nn.Embedding
   * (model/text2embedding_model.py:126-131): the projected table G = E W_ih^T + b_ih is gathered inside the recurrent kernel
   * instead of being materialised per position.  Served by the W_hh-resident forward only: g2v_gru_seq_gather_ok(T, B, H, ndir)
   * (the rule: g2v_gru_seq_route below); otherwise G2V_ERR_UNSUPPORTED.  Entries of positions outside their sequences are never read. */
  const int64_t* gi_gather;
} g2v_gru_dir;
int g2v_gru_seq_packed_ok(int T, int B, int H);
int g2v_gru_seq_gather_ok(int T, int B, int H, int ndir);
/* Round 5.  At small batch (B <= 1024, H % 4 == 0, H <= 256, H != 64) g2v_gru_seq_fwd / _bwd run one launch per time step over
 * (16 rows x 16 hidden units x direction) workgroups.  While that grid fits the device with one workgroup per CU (B = 128 at
 * H = 200, both directions: 208 workgroups) the same workgroups instead stay resident for ALL steps of ONE launch, their W_hh rows
 * in registers, and hand each other the state rows (forward) / the hidden-side gate gradients (backward) through tagged 8-byte
 * granules in the call's workspace (csrc/gru.hip: gru_cluster_*_kernel).  Forward results are bitwise those of the per-step
 * launches, backward results equal to summation order.  Like the persistent rollouts these kernels need their workgroups
 * co-resident; a bounded wait that runs out latches g2v_dec_rollout_persist_fault.  This switch (default 1; 0 = one launch per
 * step) exists for parity tests, A/B measurements and the fall-back after a latched fault.  Returns the previous setting.
 * LEGACY FORWARD = g2v_ctx_set_option(NULL, G2V_OPT_GRU_CLUSTER, enable). */
int g2v_gru_seq_set_cluster(int enable);
/* 1: an ideal call of this shape runs as CLUSTER under the current setting (g2v_gru_seq_route below; then g2v_gru_dir_bwd.hn_z ..
 * hn_coef, the fused quantiser backward, are honoured at H != 64 too).  0 at H == 64: that call runs as FAST. */
int g2v_gru_seq_cluster_ok(int T, int B, int H, int ndir);
/* A persistent cluster launch (g2v_gru_seq_fwd / _bwd, g2v_dec_rollout_fwd / _bwd at the shapes their *_cluster_ok queries
 * name) clears its exchange records in front of the kernel: a memset of 1-11 MB, 5-12 us on the caller's chain.  A caller that hands
 * such a call a workspace NOTHING ELSE WRITES can have the records cleared ahead of time, e.g. on a side stream at the start of the
 * step: this call issues the memset on `stream` now and notes it; the next cluster launch of that kind over this workspace takes
 * the note (one shot) and starts with its kernel.  The caller orders `stream` in front of that launch and keeps the workspace
 * untouched in between.  kind: 0 / 1 = g2v_gru_seq_fwd / _bwd (T, B, H, ndir; D ignored), 2 / 3 = g2v_dec_rollout_fwd / _bwd
 * (T, B, D, H; ndir ignored).  Shapes that do not run as a cluster: G2V_OK, nothing happens.  A launch over the workspace that does
 * not run as a cluster, and either of the two switches above, forget the note. */
int g2v_cluster_exchange_preclear(int kind, int T, int B, int D, int H, int ndir, void* workspace, size_t workspace_bytes,
                                  g2v_stream_t stream);
/* Void the "already clear" notes of the calling thread's context that lie inside [workspace, workspace + workspace_bytes)
 * (workspace = NULL: all of them): for an owner that abandons a step between g2v_cluster_exchange_preclear and the launch that
 * would have taken the note, or frees / re-purposes the workspace.  The notes belong to the bound context (g2v_ctx above). */
int g2v_cluster_exchange_preclear_drop(const void* workspace, size_t workspace_bytes);

/* Which implementation a g2v_gru_seq_fwd / _bwd call runs on (csrc/gru.hip: gru_route_plan).  Plain
 * arithmetic on the direction of travel, T, B, H, ndir, three options of the bound context, the device's CU count and the facts
 * of the call; first match wins.  "Aligned": 16-byte aligned in every direction, NULL counts as aligned.
 *   FAST      H == 64, the leading dimensions (hs_ld; backward d_hs_ld too) multiples of 4, and every array the kernels move as
 *             16-byte vectors aligned: forward gi, b_hh, hs, h_n, gates, x, b_ih; backward gates, dgi, dgh, hs, h0, dh0, d_hs, d_hn,
 *             dx, wslab.  Asked through the lists below, one fact per list: STEP's list and the vector body's (backward:
 *             RESIDENT's) aligned, and x, b_ih / dx, wslab.  That is a superset: the forward's w_hh and h0 are on STEP's list
 *             though FAST reads them element-wise.  An H == 64 call that misses it goes to the next route that admits it, as
 *             one with hs_ld % 4 != 0 does.  The weights as fragment packs in the workspace (g2v_gru_seq_prepare).  The only
 *             route that fuses the input projection (gi == NULL) / the input gradient (dx != NULL), both with in_dim == H,
 *             and the weight gradients (dw_hh ...).  Variant forward: 0, 1 projection fused; backward: 0, 1 dx fused, 2 and
 *             dW_hh, db_hh, 3 and dW_ih, db_ih.
 *   CLUSTER   the conditions of STEP, and G2V_OPT_GRU_CLUSTER != 0, 2 <= T <= 2^20, ceil(B/16) * ceil(H/16) * ndir <= CUs, the
 *             kernel resident with a workgroup per CU: ONE launch for all steps.
 *   STEP      B <= 1024, ceil(B/16) * ndir <= 128, H % 4 == 0, H <= 256, and aligned forward gi, w_hh, b_hh, h0, gates, h_n;
 *             backward gates, dgi, dgh, d_hn, h0, dh0: one launch per time step.
 *   RESIDENT  W_hh kept in the CU.  Forward: 192 < H <= 208, B >= G2V_OPT_GRU_RESIDENT_ROWS > 0 and the vector conditions of STREAM.
 *             Backward: H == 200, B >= G2V_OPT_GRU_RESIDENT_ROWS > 0, G2V_OPT_GRU_RESIDENT_BWD != 0, the leading dimensions
 *             multiples of 4, aligned gates, dgi, dgh, hs, h0, dh0, d_hs, d_hn.
 *   STREAM    everything else with at most 160 KB of LDS per workgroup (G2V_ERR_ARG beyond).  Variant 1, the vector body: H % 4 == 0,
 *             H <= 256, the leading dimensions multiples of 4, aligned forward gi, b_hh, hs, gates; backward gates, dgi, dgh, hs,
 *             h0, dh0, d_hs.  Variant 2 (forward): two row tiles per workgroup, from ceil(B/32) * ndir >= 192.  Variant 0: the scalar body.
 * Optional fields, G2V_ERR_UNSUPPORTED off the routes that serve them, before anything is launched:
 *   gi_gather              RESIDENT (forward) at a shape outside STEP's: g2v_gru_seq_gather_ok
 *   gi_row_off/dgi_row_off T <= 64, 4 <= H <= 256, H % 4 == 0, H != 64 (g2v_gru_seq_packed_ok), with lengths; not STREAM's scalar body
 *   gi == NULL, dx         FAST with in_dim == H
 *   dw_hh ... wslab        FAST with dx; dgh (with dw_ih: dgi too) may then be NULL, nowhere else
 *   hn_z ...               FAST or CLUSTER, with d_hn, hn_q, hn_gloss and aligned hn_z, hn_q
 * g2v_gru_seq_route returns G2V_GRU_ROUTE_* with the variant in bits 8 and up, or 0 for a call the entry point refuses.  cluster,
 * resident_rows, resident_bwd: the three options, -1 = the bound context's; cus <= 0: the device's; facts: an or of G2V_GRU_PLAN_*
 * (0: the ideal call -- aligned arrays, a workspace of the queried size, lengths given, no optional field).  The queries
 * g2v_gru_seq_cluster_ok / _gather_ok / _packed_ok are fields of the ideal call's plan. */
#define G2V_GRU_ROUTE_FAST 1
#define G2V_GRU_ROUTE_CLUSTER 2
#define G2V_GRU_ROUTE_STEP 3
#define G2V_GRU_ROUTE_RESIDENT 4
#define G2V_GRU_ROUTE_STREAM 5
#define G2V_GRU_PLAN_SPLIT_UNALIGNED 1     /* an array of STEP's list is not aligned */
#define G2V_GRU_PLAN_VEC_UNALIGNED 2       /* an array of the vector body's list */
#define G2V_GRU_PLAN_D_HN_UNALIGNED 4      /* d_hn (the backward RESIDENT's list beyond the vector body's) */
#define G2V_GRU_PLAN_HS_LD 8               /* hs_ld % 4 != 0 */
#define G2V_GRU_PLAN_D_HS_LD 16            /* d_hs_ld % 4 != 0 */
#define G2V_GRU_PLAN_PACKED 32             /* gi_row_off / dgi_row_off is set */
#define G2V_GRU_PLAN_GATHERED 64           /* gi_gather is set */
#define G2V_GRU_PLAN_NO_LENGTHS 128        /* lengths == NULL */
#define G2V_GRU_PLAN_FUSED 256             /* gi == NULL / dx != NULL */
#define G2V_GRU_PLAN_IN_DIM 512            /* ... with in_dim != H */
#define G2V_GRU_PLAN_WGRAD_HH 1024         /* dw_hh, db_hh, wslab are set */
#define G2V_GRU_PLAN_WGRAD_IH 2048         /* dw_ih, db_ih, x are set */
#define G2V_GRU_PLAN_WGRAD_PARTIAL 4096    /* ... but some direction lacks one of its group */
#define G2V_GRU_PLAN_HN 8192               /* hn_z is set */
#define G2V_GRU_PLAN_HN_UNUSABLE 16384     /* ... without d_hn, hn_q or hn_gloss, or hn_z / hn_q not aligned */
#define G2V_GRU_PLAN_NO_DGI 32768          /* dgi or dgh is NULL */
#define G2V_GRU_PLAN_PREPARED 65536        /* the *_prepared entry points: FAST launches no pack */
#define G2V_GRU_PLAN_SMALL_WORKSPACE 131072 /* workspace_bytes below the queried size */
#define G2V_GRU_PLAN_NOT_RESIDENT 262144   /* the cluster kernel does not fit a CU */
#define G2V_GRU_PLAN_FAST_UNALIGNED 524288  /* x, b_ih (forward) / dx, wslab (backward): FAST's list beyond the three above */
int g2v_gru_seq_route(int backward, int T, int B, int H, int ndir, int cluster, int resident_rows, int resident_bwd, int cus, int facts);

/* Up to 2 directions per call run in ONE launch (the two directions of a bidirectional layer are independent).  The workspace is
 * the largest of three regions: the fragment packs (per direction W_hh and W_ih), the per-step launches' state, the cluster
 * kernels' exchange records (which depend on the device's CU count).  workspace: 16-byte aligned, whatever the route
 * (G2V_ERR_ARG otherwise): the routes that use it move the packs, the state and the carry as 16-byte vectors, and no alignment
 * list of the plan carries it. */
size_t g2v_gru_seq_fwd_workspace(int ndir, int H);
int g2v_gru_seq_fwd(const g2v_gru_dir* dirs, int ndir, const int32_t* lengths, int64_t hs_ld,
                    int T, int B, int H, void* workspace, size_t workspace_bytes, g2v_stream_t stream);

/* BPTT of the above.  d_hs (row stride d_hs_ld) / d_hn may be NULL.  Produces dgi (T,B,3H) (grad wrt gi:
 * feeds W_ih, b_ih, x grads through g2v_linear_bwd_*), dgh (T,B,3H) (feeds W_hh, b_hh) and dh0 (B,H) (may be NULL). */
typedef struct {
  const float* d_hs; const float* d_hn;       /* incoming gradients (either may be NULL)            */
  const float* hs; const float* h0; const float* gates; const float* w_hh;   /* forward tensors */
  float* dgi; float* dgh; float* dh0;         /* outputs (dh0 may be NULL)                          */
  int reverse;
  /* Fused input gradient (dx != NULL): dx (T,B,in_dim) = dgi W_ih is produced by the recurrent kernel itself (a second,
   * independent MFMA chain next to the dh chain).  The FAST route with in_dim == H only; otherwise G2V_ERR_UNSUPPORTED and the caller
   * uses g2v_linear_bwd_data on dgi.  Each direction writes its own dx (the caller sums the two directions). */
  const float* w_ih;      /* (3H,in_dim) */
  float* dx;              /* out: (T,B,in_dim), overwritten */
  int in_dim;
  /* Fused weight gradients (dw_hh != NULL; with the fused input gradient on the FAST route, every direction alike;
   * G2V_ERR_UNSUPPORTED on any other route): the
   * recurrent kernel also accumulates dW_hh = sum dgh^T h_prev, dW_ih = sum dgi^T x and the two bias gradients (overwritten);
   * dgh, and with dw_ih dgi too, are then neither written nor needed (may be NULL).  x: the layer input (T,B,in_dim); wslab: scratch of
   * g2v_gru_seq_bwd_wslab_bytes(B, H) bytes PER DIRECTION. */
  const float* x;
  float* dw_hh; float* db_hh; float* dw_ih; float* db_ih;
  float* wslab;
  /* Optional (hn_z != NULL; the FAST and CLUSTER routes of g2v_gru_seq_route, G2V_ERR_UNSUPPORTED on any other, whatever took the
   * call off them): the quantiser's backward (K5', g2v_vq_bwd
   * with a dense quantised tensor) applied where d_hn is read,
   *   d_hn_effective[b,h] = d_hn[b,h] + hn_gloss[0] * hn_coef * (hn_z[b,h] - hn_q[b,h]),
   * i.e. the straight-through gradient plus the commitment term (model/Autoencoder_VQVAE_model.py:1285-1292) when the final
   * state of this direction IS the quantiser's input: hn_z / hn_q are the (B,H) slices of the encoder state and of its
   * quantised value, hn_coef = 2 beta / (N E).  Same arithmetic as g2v_vq_bwd; saves its launch on the critical chain. */
  const float* hn_z; const float* hn_q; const float* hn_gloss;
  float hn_coef;
  /* Packed dgi (NULL = (T,B,3H)): as g2v_gru_dir.gi_row_off -- dgi row (t,b) at dgi + (dgi_row_off[t] + b) * 3H, only positions
   * inside their sequences are written (sum(lengths) rows); dgh keeps the (T,B,3H) layout with zero rows at padded positions. */
  G2V_HOST const int32_t* dgi_row_off;
} g2v_gru_dir_bwd;
size_t g2v_gru_seq_bwd_wslab_bytes(int B, int H);
size_t g2v_gru_seq_bwd_workspace(int ndir, int H);   /* the largest of its three regions, as g2v_gru_seq_fwd_workspace */
int g2v_gru_seq_bwd(const g2v_gru_dir_bwd* dirs, int ndir, const int32_t* lengths, int64_t d_hs_ld, int64_t hs_ld,
                    int T, int B, int H, void* workspace, size_t workspace_bytes, g2v_stream_t stream);

/* ONE GRU cell step at small batch with the input projection included (nn.GRU cell, the code decoder of Part d,
 * model/text2embedding_model.py:372-380, where every call is one time step):
 *   gi = (x * x_keep * x_scale) W_ih^T + b_ih,  gh = h_prev W_hh^T + b_hh,  r, z, n as in g2v_gru_seq_fwd,  h_new = (1-z) n + z h_prev
 *   gates (B,4H) = r, z, n, gh_n saved for the backward (NULL = inference).  x_keep (uint8 (B,in_dim), may be NULL): the
 *   inter-layer dropout of nn.GRU on this layer's input.  One launch instead of g2v_linear_fwd + g2v_gru_seq_fwd(T = 1), same
 *   contraction order (gates bit-identical, h_new within an ulp).  in_dim, H multiples of 4 and <= 256.
 * g2v_gru_cell_bwd: d_h = d_h_a + d_h_b (gradient arriving at h_new from above / from the next step; either may be NULL) ->
 *   dgi, dgh (B,3H), d_hprev (B,H) = d_h z + dgh W_hh, dx (B,in_dim) = (dgi W_ih) * x_keep * x_scale (dx may be NULL).
 *   Two launches (gate gradients; both products) instead of four. */
int g2v_gru_cell_fwd(const float* x, int in_dim, const uint8_t* x_keep, float x_scale, const float* h_prev, const float* w_ih,
                     const float* w_hh, const float* b_ih, const float* b_hh, float* h_new, float* gates, int B, int H,
                     g2v_stream_t stream);
int g2v_gru_cell_bwd(const float* d_h_a, const float* d_h_b, const float* gates, const float* h_prev, const float* w_ih,
                     const float* w_hh, const uint8_t* x_keep, float x_scale, float* dgi, float* dgh, float* d_hprev, float* dx,
                     int in_dim, int B, int H, g2v_stream_t stream);

/* Ahead-of-time weight packs (the fused train step runs them as a parallel branch while the step's first kernels execute):
 * g2v_gru_seq_prepare launches the fragment packs of ONE g2v_gru_seq_fwd + ONE g2v_gru_seq_bwd call of the H == 64 fast
 * kernels into their two workspaces (w_hh / w_ih: one pointer per direction; fused != 0: the calls fuse the input projection /
 * input gradient, so w_ih is packed too; either workspace may be NULL); the *_prepared entry points then skip their pack launch.
 * Nothing else may touch the workspaces in between.  Other hidden sizes: prepare is a no-op and *_prepared == the plain call. */
int g2v_gru_seq_prepare(const float* const* w_hh, const float* const* w_ih, int ndir, int H, int fused, void* fwd_workspace,
                        size_t fwd_bytes, void* bwd_workspace, size_t bwd_bytes, g2v_stream_t stream);
int g2v_gru_seq_fwd_prepared(const g2v_gru_dir* dirs, int ndir, const int32_t* lengths, int64_t hs_ld, int T, int B, int H,
                             void* workspace, size_t workspace_bytes, g2v_stream_t stream);
int g2v_gru_seq_bwd_prepared(const g2v_gru_dir_bwd* dirs, int ndir, const int32_t* lengths, int64_t d_hs_ld, int64_t hs_ld,
                             int T, int B, int H, void* workspace, size_t workspace_bytes, g2v_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Autoregressive pose-decoder rollout (K9).  Replaces the T-1 step loop
 * model/Autoencoder_VQVAE_model.py:1039-1054 over Generator.forward (:646-683) ->
 * BahdanauAttnDecoderRNN.forward (:499-592) with autoencoder_att == "False", n_layers == 2:
 *   xin_t = keep95_t * y_{t-1} / 0.05   (inline nn.Dropout(0.95), ALWAYS active :570; zeros if !conditioned :568)
 *   u_t   = xin_t W_pre^T + b_pre;  a_t = ReLU(BatchNorm1d(u_t))   (batch stats if training, running stats else)
 *   h0_t  = GRUcell0(a_t, h0_{t-1});  x1_t = keep_l0_t * h0_t / (1-p)  (nn.GRU inter-layer dropout, training only)
 *   h1_t  = GRUcell1(x1_t, h1_{t-1});  y_t = h1_t W_out^T + b_out;  y_0 = target frame 0;
 *   next input = target[t] if t < n_pre_poses else y_t (:1049-1052).
 * One launch per time step (the BatchNorm batch statistics are a grid-wide reduction: the seam is a
 * kernel boundary), 16 batch rows per workgroup.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* w_pre;  const float* b_pre;     /* (H,D), (H)   decoder.decoder.pre_linear.0 */
  const float* bn_w;   const float* bn_b;      /* (H), (H)     decoder.decoder.pre_linear.1 */
  float* bn_running_mean; float* bn_running_var; /* (H) each, updated in place when training; both NULL while training: not updated (g2v_bn_running_update) */
  const float* w_ih0; const float* w_hh0; const float* b_ih0; const float* b_hh0; /* (3H,H),(3H,H),(3H),(3H) */
  const float* w_ih1; const float* w_hh1; const float* b_ih1; const float* b_hh1;
  const float* w_out;  const float* b_out;     /* (D,H), (D)   decoder.decoder.out_layer */
} g2v_dec_weights;

typedef struct {           /* saved-for-backward / state arrays, all caller-owned */
  float* y;                /* (T,B,D)   outputs, y[0] = target frame 0                       */
  float* xin;              /* (T-1,B,D) dropped decoder inputs xin_t (t = 1..T-1 at index t-1) */
  float* u;                /* (T-1,B,H) pre-BatchNorm activations                             */
  float* a;                /* (T-1,B,H) post BN+ReLU                                          */
  float* h0;               /* (T,B,H)   layer-0 hidden states, h0[0] = initial state          */
  float* h1;               /* (T,B,H)   layer-1 hidden states, h1[0] = initial state          */
  float* x1;               /* (T-1,B,H) dropped layer-0 outputs (NULL => aliases h0[1:], p == 0 or eval) */
  float* gates0;           /* (T-1,B,4H) r,z,n,ghn of layer 0 (NULL in inference)             */
  float* gates1;           /* (T-1,B,4H)                                                      */
  float* bn_partial;       /* (2, nblk, 2, H) ping-pong per-block sums of (u-b), (u-b)^2      */
  float* bn_stats;         /* (T-1,2,H) batch mean / biased var per step (training)           */
  /* Optional, all NULL / 0 = off: custom_loss (K10, train_eval/train_seq2seq.py:40-88) carried by the rollout pair and a
   * CHASER kernel, with the rollout's `target` as the loss target.  Where g2v_dec_rollout_fuses_loss() says 1 (training only):
   *   g2v_dec_rollout_prepare(...)                      (clears the forward's progress words with its exchange records)
   *   g2v_dec_rollout_fwd_prepared(..., s with loss_* set, ...)   on stream A: stores y_t write-through and publishes, per
   *                                                     workgroup and step, that y_t is in memory
   *   g2v_custom_loss_chase(..., same s, same workspace) on stream B, ordered behind g2v_dec_rollout_prepare and dispatched
   *                                                     BEHIND the forward (see its comment): consumes y_t as it lands,
   *                                                     writes loss_code, loss_coef, loss_partial
   *   (join A and B)
   *   g2v_dec_rollout_bwd[_prepared](..., same s, ...)  forms dLoss/dy_t from y_t, the code byte and the column coefficient in
   *                                                     its own tile load; `dy` of g2v_dec_grads is OUTPUT only; writes loss_terms
   * g2v_custom_loss_fwd_bwd is not called.  Same dy bits as g2v_custom_loss_fwd_bwd(g_scale = 1); the four loss sums are added
   * in a different order.  Removes the 62 + 6 us launch pair that sat alone between the rollouts and 150 MB of HBM traffic per
   * step at B = 4096, T = 34. */
  uint8_t* loss_code;      /* (T,B,D)   sign codes of the three |.| terms + the Dropout(0.95) flag */
  float* loss_coef;        /* (B,D)     w_var / numel / ||y[:,b,d]||_2                             */
  float* loss_partial;     /* (nblk,4)  per-workgroup loss sums                                    */
  float* loss_terms;       /* (5)       total, l1, cont, var, mse -- as g2v_custom_loss_fwd_bwd    */
  float loss_w[3];         /* w_l1, w_cont, w_var (custom_loss's loss_regularization weights)     */
} g2v_dec_saved;

int g2v_dec_rollout_blocks(int B);
/* Five implementations sit behind g2v_dec_rollout_fwd / _bwd (same arguments, same saved arrays, results equal to summation
 * order, each bitwise reproducible).  Which one a call runs on is decided once, from its sizes, the G2V_OPT_PERSISTENT level
 * (0..3, default 1), the device's CU count and a few facts of the call; g2v_dec_rollout_route reports the decision (host
 * arithmetic only, no launch).  nblk = ceil(B / 16) row tiles, nt = ceil(H / 16) hidden-unit tiles.  In order:
 *   PERSIST    H == 64, D == 135, B % 4 == 0 (a ragged last tile where B % 16 != 0), level >= 1, every array of the call 16-byte
 *              aligned, and R = max(ceil(nblk / min(CUs, 256)), min(level, nblk)) <= 3 row tiles per workgroup: ONE launch for
 *              the whole rollout, register / LDS-resident weights, an in-kernel two-level exchange of the BatchNorm partial sums
 *              (csrc/dec_persist.hpp).  Levels 2 / 3 ask for AT LEAST that many tiles per workgroup: how the parity tests reach
 *              the multi-tile kernels at small batches.  With R == 1 and B % 16 == 0 it also carries custom_loss
 *              (g2v_dec_rollout_fuses_loss, 2 <= T <= 256) and the W_hh1 weight gradient (g2v_dec_rollout_bwd_fuses_wgrad).
 *   CLUSTER    H != 64 or D != 135, H % 4 == 0, 4 <= H <= 208, D <= 64 (every shipped YAML's H = 200), T >= 3, level >= 1,
 *              nblk <= 64 and nblk * nt <= CUs (B <= 304 at H = 200 on 256 CUs), the split route's arrays and keep_l0 16-byte
 *              aligned, the exchange records within workspace_bytes, the kernel resident at one workgroup per CU: ONE launch for
 *              the forward and one for the backward over (hidden-unit tile x row group) workgroups, weight rows in registers,
 *              the rows a kernel boundary used to hand over (u / h0 / h1 and the BatchNorm sums forward; dbn rows, BatchNorm-
 *              backward sums and the partial products of the 3H-long contractions backward) exchanged through tagged 8-byte
 *              granules in the workspace (csrc/dec_rollout.hip: dec_cluster_fwd_kernel / dec_cluster_bwd_kernel).
 *   SPLIT      H != 64 or D != 135, H % 4 == 0, H <= 256, D <= 64, nblk <= 64 (B <= 1024), its arrays 16-byte aligned: forward
 *              step 0 as the generic per-step kernel, then three launches per step over the same workgroups; backward six
 *              transposes, then three / four launches per step.
 *   STEP_FAST  H == 64, D == 135 otherwise: one fused launch per time step, dims compile-time constants.
 *   STEP       every other shape: the same with run-time dims.
 * The optional fields no route but PERSIST honours -- the loss_* fields of g2v_dec_saved, dw_gru / db_gru of g2v_dec_grads -- are
 * refused with G2V_ERR_UNSUPPORTED on every other route, nothing launched, never silently ignored; a shape whose step kernel
 * would need more than 160 KB of LDS is refused likewise.
 * g2v_dec_rollout_route returns G2V_DEC_ROUTE_* (PERSIST: with R in bits 8..9), or 0 for sizes the calls reject (T < 2, B, D or
 * H < 1) and for flag combinations they refuse.  persistent: the level, -1 = the bound context's; cus: the CU count, 0 = the
 * device's; flags: G2V_DEC_PLAN_* facts of the call (0: aligned arrays, a workspace of the queried size, no optional field). */
#define G2V_DEC_ROUTE_STEP 1        /* generic per-step kernel */
#define G2V_DEC_ROUTE_STEP_FAST 2   /* H = 64, D = 135 per-step kernel */
#define G2V_DEC_ROUTE_SPLIT 3       /* step 0 generic, then per-phase launches */
#define G2V_DEC_ROUTE_CLUSTER 4     /* one launch for t >= 1 (forward) / the whole backward */
#define G2V_DEC_ROUTE_PERSIST 5     /* one launch; tiles per workgroup in bits 8..9 */
#define G2V_DEC_PLAN_UNALIGNED 1    /* some pointer of the call is not 16-byte aligned */
#define G2V_DEC_PLAN_WGRAD 2        /* dw_gru / db_gru of g2v_dec_rollout_bwd_fuses_wgrad() are set */
#define G2V_DEC_PLAN_LOSS 4         /* the loss_* fields are set */
int g2v_dec_rollout_route(int backward, int T, int B, int D, int H, int training, int persistent /* 0..3, -1: the bound context's */,
                          int cus /* 0: the device's */, int flags);
/* The G2V_OPT_PERSISTENT level of the calling thread's context (see g2v_dec_rollout_route; it also switches the code decoder's
 * cluster kernel): exists for A/B measurements, parity tests and the fall-back after a latched fault.  Returns the previous
 * setting.  LEGACY FORWARD = g2v_ctx_set_option(NULL, G2V_OPT_PERSISTENT, enable). */
int g2v_dec_rollout_set_persistent(int enable);
/* 0, or R = 1..3 where a call of this shape runs as PERSIST with R row tiles per workgroup (g2v_dec_rollout_route, no flags) */
int g2v_dec_rollout_tiles_per_workgroup(int B, int D, int H);
/* 1 where a call of this shape with T >= 3 runs as CLUSTER (g2v_dec_rollout_route, no flags), 0: not */
int g2v_dec_rollout_cluster_ok(int B, int D, int H);
/* The persistent kernels need every workgroup of their launch resident at once; what a plain launch can check is checked
 * (B / 16 <= CU count, the occupancy query).  What it cannot see -- a CU mask, another tenant or a second persistent launch
 * interleaved on the same device -- ends in a bounded wait running out: the kernel then LATCHES a device-side fault word and
 * stops waiting (its outputs are garbage) instead of trapping.  g2v_dec_rollout_persist_fault returns the latch (0 / 1; -1 if
 * it cannot be read) and clears it when `clear` != 0.  It is SYNCHRONOUS (a one-word device-to-host copy): call it where the
 * host synchronises anyway (bench.py at the end of the timed region; train_iter reads the latch as part of its one read-back,
 * g2v_iteration_readback); on 1 discard the step, g2v_dec_rollout_set_persistent(0), and run the step again on the per-step
 * kernels.  clear < 0 is the test hook of that path: it LATCHES the value -clear, as a bounded wait running out would. */
int g2v_dec_rollout_persist_fault(int clear);
/* Data parallelism (one process per GPU): the latch is per process.  from_flag == 0: flag[0] = 1.0f if this process' latch is set,
 * else 0.0f -- in front of the SUM all-reduce, with `flag` a slot of the communication buffer; from_flag != 0: a non-zero
 * (reduced) flag latches this process too (value 3), so that EVERY rank's commit kernels skip the step a faulting rank poisoned. */
int g2v_dec_rollout_fault_flag(float* flag, int from_flag, g2v_stream_t stream);
/* 1 where the rollout pair + chaser can carry custom_loss (the loss_* fields of g2v_dec_saved; training only): PERSIST with one
 * full row tile per workgroup and 2 <= T <= 256 (g2v_dec_rollout_route).  Elsewhere leave the loss_* fields NULL and call
 * g2v_custom_loss_fwd_bwd between the two rollouts (setting them anyway is refused with G2V_ERR_UNSUPPORTED). */
int g2v_dec_rollout_fuses_loss(int B, int D, int H, int T);
/* The chaser (csrc/dec_persist.hip, loss_chase_kernel): one light workgroup per 16 batch rows (256 threads, <= 128 registers per
 * lane, 64 B of LDS) that is CO-RESIDENT with the persistent forward rollout -- which runs one wave per SIMD and leaves a third of
 * every CU's registers unused -- polls that workgroup's progress word and consumes y_t as it lands.  `s`: the SAME struct the
 * forward of this call runs with (y, loss_code, loss_coef, loss_partial, loss_w); `fwd_workspace`: the SAME workspace (its
 * progress words).  Launch it on a second stream, ordered behind g2v_dec_rollout_prepare, and so that it is DISPATCHED BEHIND the
 * forward (the engine puts it behind the ~30 us of quantiser-statistics kernels of its side branch): the chaser waits for the
 * rollout, never the other way round, but a CU that already holds two chaser workgroups has no room for a rollout workgroup.
 * Every wait is bounded and ends in the fault latch (g2v_dec_rollout_persist_fault), as the exchange's do. */
int g2v_custom_loss_chase(const float* target /* (B,T,D) */, const g2v_dec_saved* s, const uint8_t* keep95 /* (T-1,B,D) */,
                          int T, int B, int D, int H, void* fwd_workspace, size_t fwd_workspace_bytes, g2v_stream_t stream);
/* workspace: the weights re-laid-out in MFMA fragment order (packed once per call) + the persistent kernel's exchange
 * state (zeroed by a memset node in front of its launch). */
size_t g2v_dec_rollout_fwd_workspace(int D, int H);
int g2v_dec_rollout_fwd(const float* target /* (B,T,D) row-major */, const float* h_init /* (2,B,H) */,
                        const g2v_dec_weights* w, const g2v_dec_saved* s,
                        const uint8_t* keep95 /* (T-1,B,D) */, const uint8_t* keep_l0 /* (T-1,B,H) or NULL */,
                        float p_drop, int n_pre_poses, int conditioned, int training,
                        int T, int B, int D, int H, void* workspace, size_t workspace_bytes, g2v_stream_t stream);

typedef struct {           /* gradient outputs of the rollout backward, caller-owned */
  float* dy;               /* (T,B,D) in: dLoss/dy_t (t=0 row ignored); out: total dL/dy_t incl. feedback */
  float* du;               /* (T-1,B,H) grad wrt pre-BN activations          -> W_pre, b_pre        */
  float* dbn;              /* (T-1,B,H) scratch: grad wrt BN output after ReLU                     */
  float* dgi0; float* dgh0;/* (T-1,B,3H) each                                -> W_ih0/b_ih0, W_hh0/b_hh0 */
  float* dgi1; float* dgh1;/* (T-1,B,3H)                                                             */
  float* dh_init;          /* (2,B,H) grad wrt the initial hidden state (the quantised latent)     */
  float* d_bn_w; float* d_bn_b; /* (H) each, overwritten                                           */
  float* bn_bwd_partial;   /* (2, nblk, 2, H) ping-pong per-block sums                              */
  /* Optional: GRU weight / bias gradients dW (3H,H), db (3H), indexed ih0, hh0, ih1, hh1, overwritten.  Set exactly the
   * entries named by g2v_dec_rollout_bwd_fuses_wgrad() (or none): those are accumulated INSIDE the persistent backward kernel,
   * in the shadow of its BatchNorm exchange, and the matching dgi / dgh array (dgh1 for W_hh1) is neither written nor needed. */
  float* dw_gru[4];
  float* db_gru[4];
} g2v_dec_grads;

/* workspace: transposed weights in MFMA fragment order. */
size_t g2v_dec_rollout_bwd_workspace(int D, int H);
/* Which GRU weight gradients g2v_dec_rollout_bwd accumulates inside its persistent kernel at this batch / shape: bit m of the
 * result <-> matrix m of (W_ih0, W_hh0, W_ih1, W_hh1).  Today 8 (W_hh1: what the kernel's register budget has room for) on
 * PERSIST with one full row tile per workgroup (g2v_dec_rollout_route), else 0.  The caller sets dw_gru[m] / db_gru[m] for exactly
 * those matrices (or for none) and forms the other products itself; anything else is refused with G2V_ERR_UNSUPPORTED. */
int g2v_dec_rollout_bwd_fuses_wgrad(int B, int D, int H);
int g2v_dec_rollout_bwd(const g2v_dec_weights* w, const g2v_dec_saved* s, const g2v_dec_grads* g,
                        const uint8_t* keep95, const uint8_t* keep_l0, float p_drop, int n_pre_poses,
                        int conditioned, int T, int B, int D, int H,
                        void* workspace, size_t workspace_bytes, g2v_stream_t stream);

/* The same for a rollout pair: the forward and backward fragment packs AND the clearing of the two exchange regions of the
 * persistent kernels (everything of the pair that depends on the weights only), ahead of time; g2v_dec_rollout_fwd_prepared /
 * _bwd_prepared then start with their first real kernel.  Honoured for H == 64, D == 135 (the fused kernels); other shapes:
 * prepare is a no-op and *_prepared == the plain call.  bwd_workspace may be NULL (inference). */
int g2v_dec_rollout_prepare(const g2v_dec_weights* w, int D, int H, void* fwd_workspace, size_t fwd_bytes,
                            void* bwd_workspace, size_t bwd_bytes, g2v_stream_t stream);
/* Round 5: g2v_dec_rollout_prepare (both workspaces) AND g2v_gru_seq_prepare (backward workspace only; w_hh / w_ih: one pointer
 * per direction) of one fused train step as ONE launch instead of six (three packs, two memset nodes, one pack).  H == 64,
 * D == 135 only (G2V_ERR_UNSUPPORTED otherwise, nothing launched: call the two functions). */
int g2v_train_step_prepare(const g2v_dec_weights* w, int D, int H, void* dec_fwd_workspace, size_t dec_fwd_bytes,
                           void* dec_bwd_workspace, size_t dec_bwd_bytes, const float* const* gru_w_hh,
                           const float* const* gru_w_ih, int gru_ndir, int gru_fused, void* gru_bwd_workspace,
                           size_t gru_bwd_bytes, g2v_stream_t stream);
/* Deferred commit of BatchNorm1d's running statistics (momentum 0.1, unbiased variance, `steps` = T-1 updates in step order)
 * from g2v_dec_saved.bn_stats of a TRAINING rollout that was given bn_running_mean = bn_running_var = NULL: the forward rollout
 * then leaves them alone, and this call -- placed where the whole step is known to be valid, e.g. behind the backward rollout --
 * applies them unless the persistent rollouts' fault latch is set (g2v_dec_rollout_persist_fault). */
int g2v_bn_running_update(const float* bn_stats, float* running_mean, float* running_var, int steps, int H, int B,
                          g2v_stream_t stream);
int g2v_dec_rollout_fwd_prepared(const float* target, const float* h_init, const g2v_dec_weights* w, const g2v_dec_saved* s,
                                 const uint8_t* keep95, const uint8_t* keep_l0, float p_drop, int n_pre_poses,
                                 int conditioned, int training, int T, int B, int D, int H, void* workspace,
                                 size_t workspace_bytes, g2v_stream_t stream);
int g2v_dec_rollout_bwd_prepared(const g2v_dec_weights* w, const g2v_dec_saved* s, const g2v_dec_grads* g,
                                 const uint8_t* keep95, const uint8_t* keep_l0, float p_drop, int n_pre_poses,
                                 int conditioned, int T, int B, int D, int H, void* workspace, size_t workspace_bytes,
                                 g2v_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Gesture generation: the decoder's chain over the chunks of a clip, in ONE launch (csrc/dec_chain.hip).  Replaces the decode
 * loops of Clustering.py:198-261 (make_VQ_Centers), inference_Autoencoder.py:124-244 and inference_text2embedding.py:400-547.
 * step(x, h, keep) is the recurrence stated above g2v_dec_weights in EVAL mode (running statistics, no inter-layer dropout;
 * the inline Dropout(0.95) stays active).  For clip b, with S = warmup + T - 1 steps per chunk:
 *   carry = start[b] (NULL: zeros)
 *   for c in 0..C-1:
 *     h = rows[ids[b,c]] (ids NULL: rows[b C + c]), split as [layer 0 | layer 1];  inp = carry;  out[b, c T + 0] = inp
 *     for s in 0..warmup-1:  _, h = step(inp, h, keep95[c,s,b])                      (output discarded)
 *     for t in 1..T-1:       y, h = step(inp, h, keep95[c,warmup+t-1,b]);  out[b, c T + t] = y
 *                            inp = teacher[b,c,t] if teacher != NULL and t < n_pre_poses else y
 *     carry = inp            (conditioned == 0: xin is zero in every step and carry = zeros)
 * rows (R,2H); ids (B,C) int64 or NULL; start (B,D) or NULL; teacher (B,C,T,D) or NULL; keep95 (C,S,B,D) uint8 (may be NULL when
 * conditioned == 0); out (B,C T,D); h_last (2,B,H) or NULL: the hidden state after the last step.  Arrays need their natural
 * alignment only (4 bytes, ids 8, masks 1); the workspace 16 bytes.  An id outside [0, R) reads nothing and seeds a ZERO hidden state (callers check ids
 * first).  w: bn_running_mean / bn_running_var are required and not modified.
 * One workgroup owns 16 clips and is independent of every other: no exchange, no wait, nothing for the fault latch.  BatchNorm
 * is folded into pre_linear when the weights are packed into the workspace (once per call), so `a` differs from the unfused
 * kernels' by rounding; results are bitwise reproducible and a clip's bits do not depend on the batch it is decoded in.
 * g2v_dec_chain_ok: 1 for exactly C >= 1, T >= 2, warmup >= 0, B >= 1, 1 <= D <= 256, 1 <= H <= 256, C <= 2^20 and
 * warmup + T - 1 <= 2^20; else 0, and g2v_dec_chain_fwd returns G2V_ERR_UNSUPPORTED (host arithmetic only).
 * g2v_dec_chain_workspace: bytes (0 where D or H is outside the served set).
 * ------------------------------------------------------------------------------------------ */
int g2v_dec_chain_ok(int C, int T, int warmup, int B, int D, int H);
size_t g2v_dec_chain_workspace(int D, int H);
int g2v_dec_chain_fwd(const float* rows, int64_t R, const int64_t* ids, const float* start, const float* teacher,
                      const uint8_t* keep95, const g2v_dec_weights* w, float* out, float* h_last, int n_pre_poses,
                      int conditioned, int C, int T, int warmup, int B, int D, int H, void* workspace, size_t workspace_bytes,
                      g2v_stream_t stream);
/* The tail of a generated clip, r (B,F,Dr) -> out (B,F,Dr), F = C T, r != out:
 *   1. blend across every chunk boundary o = c T, c >= 1 (inference_Autoencoder.py:388-395 with its literal 30 as T), n = blend:
 *        r'[o+i] = r[o-i] (n-i)/(n+1) + r[o+i] (i+1)/(n+1),  i = 0..n-1, reading the un-blended r.
 *      blend == 0: none.  This equals the reference's in-place loop only for T >= 2 n - 1; below that: G2V_ERR_ARG.
 *   2. * max(std, 0.01) + mean (:400-403); mean, std (Dr) or both NULL: none.
 *   3. savgol != NULL: a Savitzky-Golay filter along time, window 25 (inference_text2embedding_GENEA.py:600), from a host-made
 *      table of 625 floats: 25 interior taps, then the 12 x 25 matrices that give the first / last 12 frames from the first /
 *      last 25 (scipy's mode="interp").  Needs F >= 25 (else G2V_ERR_ARG) and tmp (B,F,Dr), distinct from r and out. */
int g2v_clip_finish(const float* r, float* out, const float* mean, const float* std, const float* savgol, float* tmp, int T,
                    int blend, int B, int F, int Dr, g2v_stream_t stream);
/* Joint angles from a finished clip (csrc/clip_angles.hip): what every make_bvh of the reference computes between the clip's 3x3
 * matrices and the BVH writer (inference_Autoencoder.py:584-592, inference_text2embedding_GENEA.py:602-612).
 *
 * g2v_rotmat_to_euler: frames (N, 9 J) -> angles (N, 3 J) in degrees; columns joint-major, each joint's matrix row-major, its
 * angles (Z, X, Y) with R = Rz(Z) Rx(X) Ry(Y): scipy's Rotation.from_matrix(m).as_euler("ZXY", degrees=True).  The matrices are a
 * decoder's output and not orthogonal, and scipy's from_matrix is two functions across versions; `method` picks one:
 *   G2V_ROT_MARKLEY     scipy 1.10.1, the reference's pin: Markley's quaternion from the RAW entries (the branch of the largest of
 *                       m00, m11, m22, trace; the first on ties), normalised.
 *   G2V_ROT_PROCRUSTES  scipy 1.15.3: the matrix is first replaced by the nearest rotation (its orthogonal polar factor, U V^T of
 *                       its SVD; here by a scaled Newton iteration converged below 1e-13), then Markley.
 * On exact rotations the two agree to rounding.  Past the quaternion both share scipy's rule: X in [-90, 90]; within 1e-7 rad of
 * X = +-90 degrees Y is exactly 0 and Z carries the combined rotation; Z and Y lie in [-180, 180].  Arithmetic is float64 from the
 * float32 entries with ONE rounding to float32 on output (at most 180 * 2^-24 = 1.07e-5 degrees).
 * A matrix whose determinant is not > 0 (zero, a reflection, a NaN entry), under either method, gets NaN in its three angles and adds
 * 1 to bad[0] (int64[1], cleared by the caller; an integer atomic); its neighbours are untouched.  N >= 1, J >= 1,
 * N * J <= (2^31 - 1) * 256, method one of the two constants: G2V_ERR_ARG otherwise, nothing launched.  frames and angles must not
 * overlap.  No workspace.
 *
 * g2v_smoothing_spline: y (B, F, Cn) -> out (B, F, Cn), de Boor's cubic smoothing spline of every (clip, channel) column along F at
 * unit-spaced knots with unit weights, evaluated at the knots: csaps.csaps(x, y, x, smooth=p), the reference's
 * smoothing_function("spline", .) with p = 0.5, which is scipy's make_smoothing_spline(x, y, lam=(1-p)/p)(x).  With n = F - 2:
 *   (6 (1-p) Q^T Q + p R) u = Q^T y,   out = y - 6 (1-p) Q u,    Q (F, n) with columns (1, -2, 1),  R (n, n) tridiagonal (1, 4, 1).
 * p = 1 returns y and p = 0 the least-squares straight line; F == 2 returns y.  The pentadiagonal matrix depends on F and p only: it
 * is factored once per call (L D L^T, float64, 3 n doubles at the start of the workspace), then one lane per column solves in
 * float64 and keeps its intermediate vector in the workspace as (n, B Cn) float64; one rounding to float32 on output.  Both launches
 * go to `stream`; nothing is read back.  The same input gives the same bits and a clip's bits do not depend on the other clips.
 * out may BE y (in place); any other overlap of the two is not allowed.
 * 0 <= smooth <= 1, B >= 1, F >= 2, Cn >= 1 (G2V_ERR_ARG otherwise); F <= 2^20 and B Cn < 2^31 (G2V_ERR_UNSUPPORTED beyond).
 * g2v_smoothing_spline_workspace: bytes, (3 + B Cn)(F - 2) * 8; 0 for F == 2 and outside those limits.  The workspace is 8-byte
 * aligned, may hold anything on entry and is needed whatever smooth is; fewer bytes: G2V_ERR_WORKSPACE.  Every refusal comes before
 * the first launch: nothing is written. */
#define G2V_ROT_MARKLEY 0
#define G2V_ROT_PROCRUSTES 1
int g2v_rotmat_to_euler(const float* frames, float* angles, int64_t* bad, int64_t N, int J, int method, g2v_stream_t stream);
size_t g2v_smoothing_spline_workspace(int B, int F, int Cn);
int g2v_smoothing_spline(const float* y, float* out, double smooth, int B, int F, int Cn, void* workspace,
                         size_t workspace_bytes, g2v_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * custom_loss forward + gradient (K10), train_eval/train_seq2seq.py:40-88.
 *   loss = w_l1*mean|y-tgt| + w_cont*sum_t|y_t-y_{t-1}|/numel - w_var*sum_{b,d}||y[b,:,d]||_2/numel
 * y is time-major (T,B,D) (the rollout's buffer), target is (B,T,D).  dy (T,B,D) = g_scale * dloss/dy
 * (may be NULL).  terms out (5 floats): total, l1, cont, var, mse (= mean (y-tgt)^2, the metric of
 * evaluate_testset train_autoencoder_VQVAE.py:350-410).  partial: >= g2v_custom_loss_blocks(B,D)*4 floats.
 * ------------------------------------------------------------------------------------------ */
int g2v_custom_loss_blocks(int B, int D);
int g2v_custom_loss_fwd_bwd(const float* y, const float* target, float* dy, float* terms, float* partial,
                            float w_l1, float w_cont, float w_var, float g_scale,
                            int T, int B, int D, g2v_stream_t stream);

/* MSE loss + gradient (train_iter_DAE, train_eval/train_seq2seq.py:208-222): loss[0] = mean((y-t)^2),
 * dy = g_scale * 2 (y-t)/n (dy may be NULL).  partial: >= g2v_mse_blocks(n) floats. */
int g2v_mse_blocks(int64_t n);
int g2v_mse_fwd_bwd(const float* y, const float* target, float* dy, float* loss, float* partial, int64_t n,
                    float g_scale, g2v_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused clip_grad_norm_(5) + Adam over one flat parameter buffer (K11),
 * train_eval/train_seq2seq.py:743-744, train_autoencoder_VQVAE.py:193-195.
 *   total = ||grad||_2; coef = min(1, max_norm/(total+1e-6)); g = grad*coef*grad_scale;
 *   m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * step_counter: device int32, incremented by this call before use (so hipGraph replays advance it).
 * gnorm_out (1 float, may be NULL).  partial: >= g2v_adam_blocks(n) floats.
 * ------------------------------------------------------------------------------------------ */
int g2v_adam_blocks(int64_t n);
/* out4[k] = *s_k (NULL: 0), k < 3; out4[3] = g2v_dec_rollout_persist_fault's latch as a float: the scalars an iteration reads
 * back (loss terms, perplexity) plus the latch in ONE device array, i.e. one device-to-host copy at the iteration's sync point. */
int g2v_iteration_readback(const float* s0, const float* s1, const float* s2, float* out4, g2v_stream_t stream);
/* g2v_clip_adam_step with g2v_iteration_readback(s0, s1, s2, out4) folded into its second launch (out4 is written also when the
 * fault latch holds the update back) */
int g2v_clip_adam_step_readback(float* param, const float* grad, float* m, float* v, int64_t n,
                                float* partial, int32_t* step_counter, float* gnorm_out,
                                float max_norm, float grad_scale, float lr, float beta1, float beta2, float eps,
                                const float* s0, const float* s1, const float* s2, float* out4, g2v_stream_t stream);
int g2v_clip_adam_step(float* param, const float* grad, float* m, float* v, int64_t n,
                       float* partial, int32_t* step_counter, float* gnorm_out,
                       float max_norm, float grad_scale, float lr, float beta1, float beta2, float eps,
                       g2v_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Soft quantiser VQ_Payam_GSSoft (model/Autoencoder_VQVAE_model.py:1304-1438; the variant Autoencoder_VQVAE ships with,
 * :816-820).  flat = mean_layer(x) and logvar = logvar_layer(flat) are g2v_linear_fwd calls, dots = flat W^T too.
 *   g2v_vq_soft_fwd   d = |flat|^2 + |W|^2 - 2 dots (written over `dots_to_dist`), smooth = 1/exp(logvar)^2,
 *                     probs = row-normalised exp(-(d/400) * 0.5 * smooth)/sqrt(smooth) (:1349-1372,1396-1411);
 *                     perplexity[0] = exp(-sum_k avg_k log(avg_k + 1e-10)), avg = mean_n probs (:1432-1433; may be NULL)
 *   g2v_vq_soft_bwd   from dprobs: dd (N,K) = dL/d distance, dlogvar (N,K), rowsum (N) = sum_k dd
 *   g2v_rowscale_combine  out[r,c] = 2 a[r,c] v[r] - 2 t[r,c]: the gradient of d wrt flat (a = flat, v = rowsum,
 *                     t = dd W) and wrt the codebook (a = W, v = column sums of dd, t = dd^T flat)
 *   g2v_ste_f32       out = z + (q - z)   (the straight-through value, :1431)
 *   g2v_vq_soft_perplexity  the same perplexity from probs as its own call over the whole device (two launches: per-row-range
 *                     column sums into `workspace`, >= g2v_vq_soft_perplexity_workspace(N, K) bytes, then one workgroup; fixed
 *                     summation order).  g2v_vq_soft_fwd's built-in one runs as ONE workgroup (it has no workspace to spread
 *                     over): 255 us at N = 4096, K = 512 against 12 here -- pass perplexity = NULL there and call this.
 * q = probs W is g2v_linear_bwd_data(probs, W); its gradients are g2v_linear_fwd / g2v_linear_bwd_weight.
 * ------------------------------------------------------------------------------------------ */
size_t g2v_vq_soft_perplexity_workspace(int N, int K);
int g2v_vq_soft_perplexity(const float* probs, float* perplexity, int N, int K, void* workspace, size_t workspace_bytes,
                           g2v_stream_t stream);
int g2v_vq_soft_fwd(const float* flat, float* dots_to_dist, const float* logvar, const float* code_sqnorm, float* probs,
                    float* perplexity, int N, int E, int K, g2v_stream_t stream);
int g2v_vq_soft_bwd(const float* probs, const float* dprobs, const float* dist, const float* logvar, float* dd,
                    float* dlogvar, float* rowsum, int N, int K, g2v_stream_t stream);
int g2v_rowscale_combine(const float* a, const float* v, const float* t, float* out, int64_t rows, int cols,
                         g2v_stream_t stream);
int g2v_ste_f32(const float* z, const float* q, float* out, int64_t n, g2v_stream_t stream);
/* The same quantiser, fused (csrc/vq_soft.hip; E == 128, K % 128 == 0, K <= 1024: g2v_vq_soft_fused_ok, else use the calls above).
 * A workgroup owns 16 rows of x (N,E); nothing (N,K)-sized travels between launches:
 *   g2v_vq_soft_fused_fwd   flat = mean_layer(x), logvar = logvar_layer(flat), dist, probs, q = probs W (all written: the
 *                           backward and the weight gradients read them), dq = 2 g_scale (q - x) / (N E) (the q_latent gradient),
 *                           quant = x + (q - x), mse_partial[blk] = sum over the workgroup's rows of (q - x)^2 and -- colsum may be
 *                           NULL -- colsum[blk][K] = column sums of probs; blk < g2v_vq_soft_fused_blocks(N)
 *   g2v_vq_soft_finish      mse = sum mse_partial / (N E) (mse may be NULL), loss_vq = mse * one_plus_beta[0] (device scalar),
 *                           perplexity = exp(-sum_k avg_k log(avg_k + 1e-10)) from colsum (both may be NULL); one workgroup
 *   g2v_vq_soft_fused_bwd   gz = [dh + g_loss[0] 2 beta (x - q) / (N E)] + dflat W_mean with dflat = (2 flat sum_k dd - 2 dd W) +
 *                           dlogvar W_logvar, (dd, dlogvar) = the backward of probs wrt (dist, logvar) at dprobs = dq W^T; dd,
 *                           dlogvar (N,K) and dflat (N,E) are written for g2v_linear_bwd_weight.  dh / g_loss may be NULL (= 0).
 * Element-wise arithmetic as in the separate kernels; the K- and E-long sums meet in another fixed order (fp32 rounding). */
int g2v_vq_soft_fused_ok(int N, int E, int K);
int g2v_vq_soft_fused_blocks(int N);
int g2v_vq_soft_fused_fwd(const float* x, const float* w_mean, const float* b_mean, const float* w_logvar, const float* b_logvar,
                          const float* codebook, const float* code_sqnorm, float* flat, float* logvar, float* dist, float* probs,
                          float* q, float* dq, float* quant, float* mse_partial, float* colsum, float g_scale, int N, int E, int K,
                          g2v_stream_t stream);
int g2v_vq_soft_finish(const float* mse_partial, const float* colsum, const float* one_plus_beta, float* mse, float* loss_vq,
                       float* perplexity, int N, int E, int K, g2v_stream_t stream);
int g2v_vq_soft_fused_bwd(const float* dh, const float* g_loss, const float* x, const float* q, const float* dq, const float* flat,
                          const float* probs, const float* dist, const float* logvar, const float* w_mean, const float* w_logvar,
                          const float* codebook, float* dd, float* dlogvar, float* dflat, float* gz, float beta, int N, int E, int K,
                          g2v_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The variational block of the chunk autoencoder (autoencoder_vae == "True", model/Autoencoder_VQVAE_model.py:776-789, 879-899,
 * 989-1010; train_eval/train_seq2seq.py:710-729), between the encoder state (or the quantiser's output) h (L,B,H) and the decoder's
 * initial state d (L,B,H).  E = L H; row b of hf = h.transpose(1, 0).reshape(B, E) is [h[0, b] ; h[1, b] ; ...] and is read
 * straight from the (L,B,H) layout (d and dh are written straight into it).  A workgroup owns 16 whole rows.
 *   g2v_vae_latent_fwd   mean = hf w_mean^T + b_mean, logvar = hf w_std^T + b_std, z = mean + exp(logvar / 2) eps,
 *                        d = z w_dec^T + b_dec, kl[0] = 0.5 mean(exp(logvar) - logvar - 1 + mean^2) over the B E elements -- one
 *                        launch + a one-workgroup finish of kl (fixed-order sums, no atomics: the same input gives the same bits).
 *                        sample != 0: eps = eps_in (B,E) when given, else drawn from the g2v_keep_mask stream (seed,
 *                        offset_counter[0]; Philox block g <-> elements 4g .. 4g+3 of (B,E), two Box-Muller pairs per block), the
 *                        counter then advances by 1; eps_out (B,E) receives the eps used (required when drawn, else may be NULL).
 *                        sample == 0: z = mean bit for bit (reparameterize(train=False)), eps is neither read nor written.
 *                        mean, logvar, z (B,E) are always written; hf (B,E) (the gathered rows, for the weight gradients) may be
 *                        NULL; w_dec, b_dec, d may be NULL together (no third product).
 *                        workspace >= g2v_vae_latent_fwd_workspace(B, E) bytes (the workgroups' KL partials).
 *   g2v_vae_latent_bwd   dz = g_d w_dec (g_d (L,B,H): the decoder stage's dh_init), c = g_kl[0] / (B E) (g_kl: device scalar
 *                        d loss / d kl, NULL = 0),
 *                          dmean   = dz + c mean,    dlogvar = dz 0.5 exp(logvar / 2) eps + c 0.5 (exp(logvar) - 1),
 *                          dh      = dmean w_mean + dlogvar w_std   (one accumulation over the concatenated K = 2 E) -> (L,B,H);
 *                        dmean, dlogvar (B,E) are written for g2v_linear_bwd_weight.  eps NULL: the forward had sample == 0.
 *                        g_mean, g_logvar (B,E; NULL = 0): gradients that reach mean / logvar directly (a caller's own loss on the
 *                        returned tensors) are added to dmean / dlogvar.
 * Served (g2v_vae_latent_ok): E % 16 == 0, E <= 512, any B >= 1; H % 4 == 0.  Anything else: G2V_ERR_UNSUPPORTED, no launch.
 * All pointers 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int g2v_vae_latent_ok(int B, int E);
int g2v_vae_latent_blocks(int B);
size_t g2v_vae_latent_fwd_workspace(int B, int E);
int g2v_vae_latent_fwd(const float* h, const float* w_mean, const float* b_mean, const float* w_std, const float* b_std,
                       const float* w_dec, const float* b_dec, const float* eps_in, uint64_t seed, int64_t* offset_counter,
                       int sample, float* mean, float* logvar, float* z, float* eps_out, float* hf, float* d, float* kl,
                       void* workspace, size_t workspace_bytes, int B, int L, int H, g2v_stream_t stream);
int g2v_vae_latent_bwd(const float* g_d, const float* g_kl, const float* g_mean, const float* g_logvar, const float* mean,
                       const float* logvar, const float* eps, const float* w_mean, const float* w_std, const float* w_dec,
                       float* dmean, float* dlogvar, float* dh, int B, int L, int H, g2v_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Remaining operators of Part d (text -> gesture-code seq2seq, model/text2embedding_model.py).
 *   g2v_embedding_fwd   out[r,:] = table[ids[r],:] * keep * scale   (nn.Embedding :90-92,126 / :252,340-343 with the
 *                       decoder's nn.Dropout(0.5) fused; keep may be NULL; row r of out starts at out + r * ldo, e.g. the
 *                       first half of the attention decoder's (B,2H) input)
 *   g2v_embedding_bwd   d_table[v,:] (+)= sum_{r: ids[r]=v} d_out[r,:] * keep * scale.  No float atomics: tokens are counting-
 *                       sorted by row (stable), 128-token chunks of the sorted list are summed in order and rows that span
 *                       chunks add their chunk partials in order -- a fixed summation tree, bitwise reproducible.
 *                       zero_first bit 0: overwrite instead of accumulate; bit 1 (round 6): `ws` still holds the sort of THESE
 *                       ids from the previous call (same ids, n, V, untouched since) -- the sort is skipped (the two directions of
 *                       a bidirectional layer scatter-add by the same words).  ws: g2v_embedding_bwd_ws_bytes(n, dim, V) bytes
 *                       of device scratch (ids outside [0,V) contribute nothing)
 *   g2v_batchnorm_fwd   nn.BatchNorm1d(H) on (B,H) (+ optional fused ReLU), decoder.pre_linear[1:] :286-290; training:
 *                       batch statistics, running stats updated with momentum 0.1 / unbiased variance (both NULL while training:
 *                       left alone, the caller commits them with g2v_bn_running_update_invstd); save_* for bwd
 *   g2v_batchnorm_bwd   dx, dweight, dbias (overwritten) from dy (the ReLU mask is taken from y > 0 when relu)
 *   g2v_batchnorm_bwd_steps   the same for the `steps` calls of a decode loop in one launch (dy, x, y, dx: (steps,B,H); row s
 *                       of save_* at + s * stat_stride floats; B < 1024): dx per step bitwise g2v_batchnorm_bwd's, dw / db the
 *                       SUM over the steps in call order (autograd's accumulation over the loop's T-1 BatchNorm nodes,
 *                       model/text2embedding_model.py:286-290 under :701-744)
 *   g2v_one_hot_rows    out[r,:] = one_hot(ids[r]) as float (row r at out + r * ld; an id outside [0,K) gives a zero row):
 *                       outputs[:, 0, :] of Part d (model/text2embedding_model.py:676-677)
 *   g2v_cross_entropy_fwd_bwd   loss[0] = mean_r( logsumexp(logits[r]) - logits[r, t_r] ), dlogits = g_scale *
 *                       (softmax - onehot)/M  (torch.nn.CrossEntropyLoss, train_eval/train_seq2seq.py:520-530);
 *                       row_loss: M floats of scratch; dlogits may be NULL
 *   g2v_argmax_rows     out[r] = argmax_k x[r,k] (lowest index on ties): greedy feedback :740
 * ------------------------------------------------------------------------------------------ */
int g2v_embedding_fwd(const float* table, const int64_t* ids, const uint8_t* keep, float scale, float* out, int64_t ldo,
                      int64_t n, int dim, int64_t V, g2v_stream_t stream);
size_t g2v_embedding_bwd_ws_bytes(int64_t n, int dim, int64_t V);
int g2v_embedding_bwd(const float* d_out, const int64_t* ids, const uint8_t* keep, float scale, float* d_table,
                      int64_t n, int dim, int64_t V, int zero_first, void* ws, size_t ws_bytes, g2v_stream_t stream);
int g2v_batchnorm_fwd(const float* x, const float* weight, const float* bias, float* running_mean, float* running_var,
                      int training, int relu, float* y, float* save_mean, float* save_invstd, int B, int H,
                      g2v_stream_t stream);
/* Deferred commit of the running statistics from the saved (mean, 1/sqrt(var + eps)) of `steps` training calls that were given
 * running_mean = running_var = NULL (g2v_batchnorm_fwd, g2v_attn_code_rollout_fwd), in call order; row s of either array starts
 * at + s * step_stride floats.  Does nothing while the persistent kernels' fault latch is set (g2v_dec_rollout_persist_fault):
 * place it behind the backward, in front of the optimiser step.  Replaces the T-1 in-place updates of the reference's
 * nn.BatchNorm1d inside the decode loop (model/text2embedding_model.py:286-290 under :701-744). */
int g2v_bn_running_update_invstd(const float* save_mean, const float* save_invstd, int64_t step_stride, float* running_mean,
                                 float* running_var, int steps, int H, int B, g2v_stream_t stream);
int g2v_batchnorm_bwd(const float* dy, const float* x, const float* y, const float* weight, const float* save_mean,
                      const float* save_invstd, int relu, float* dx, float* dw, float* db, int B, int H,
                      g2v_stream_t stream);
int g2v_batchnorm_bwd_steps(const float* dy, const float* x, const float* y, const float* weight, const float* save_mean,
                            const float* save_invstd, int64_t stat_stride, int relu, float* dx, float* dw, float* db, int steps,
                            int B, int H, g2v_stream_t stream);
int g2v_one_hot_rows(const int64_t* ids, float* out, int64_t ld, int M, int K, g2v_stream_t stream);
int g2v_cross_entropy_fwd_bwd(const float* logits, int64_t ld, const int64_t* targets, float* loss, float* row_loss,
                              float* dlogits, int64_t ldd, int M, int K, float g_scale, g2v_stream_t stream);
int g2v_argmax_rows(const float* x, int64_t ld, int64_t* out, int M, int K, g2v_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Bahdanau attention of the code decoder (autoencoder_att == "True", config/seq2seqtxt.yml:37):
 * Attn.forward / Attn.score (model/text2embedding_model.py:160-198) + the context product :353-359.
 *   energy[t,b,:] = tanh(attn([h_b ; enc[t,b,:]])) = tanh(hp[b,:] + ep[t,b,:]) with
 *     hp (B,H) = h W_attn[:, :H]^T + b_attn   (g2v_linear_fwd, once per decode step)
 *     ep (T,B,H) = enc W_attn[:, H:]^T        (g2v_linear_fwd, once per batch of sentences)
 *   weights[b,:] = softmax_t( v . energy[t,b,:] )  over ALL T positions (no padding mask, as in the reference)
 *   ctx[b,:]     = sum_t weights[b,t] * enc[t,b,:]           (written with row stride ldctx, e.g. into the second
 *                                                              half of the (B,2H) decoder input)
 * g2v_attn_bwd: from d_ctx (row stride ldd) computes d_hp (B,H), d_ep (T,B,H), d_enc (T,B,H) [the direct context
 * term only; the ep path continues through g2v_linear_bwd_data] and d_v (H); accumulate != 0 adds into d_ep / d_enc /
 * d_v (the S-1 decode steps share them).  Deterministic (fixed summation order, no atomics).  d_v == NULL: the per-row
 * partials (B,H) stay in `workspace` and the caller sums them (g2v_slab_sum; one reduction behind the last step instead of one
 * per step when every step is handed its own workspace slab).
 * g2v_attn_step_fwd (round 6): the row-local head of a decode step in one launch -- id[b] = argmax_k logits[b,k] (the greedy
 * feedback :740, lowest index on ties; logits == NULL: ids[b] is given, the teacher-forced steps), written to ids;
 * ec[b, :H] = table[id[b], :] * keep[b, :] * emb_scale (Embedding + Dropout(0.5) :340-343; keep may be NULL; table is (K,H));
 * ec[b, H:2H] = the attention context of g2v_attn_fwd (row b of ec at ec + b * ldec, ldec >= 2H); weights as g2v_attn_fwd.
 * ------------------------------------------------------------------------------------------ */
int g2v_attn_fwd(const float* hp, const float* ep, const float* enc, const float* v, float* weights, float* ctx,
                 int64_t ldctx, int T, int B, int H, g2v_stream_t stream);
int g2v_attn_step_fwd(const float* logits, int64_t ldl, int K, int64_t* ids, const float* table, const uint8_t* keep,
                      float emb_scale, float* ec, int64_t ldec, const float* hp, const float* ep, const float* enc,
                      const float* v, float* weights, int T, int B, int H, g2v_stream_t stream);
/* out (+)= slab 0 + slab 1 + ... + slab n-1 (n slabs of `len` floats, added in slab order) */
int g2v_slab_sum(const float* slabs, int n, int64_t len, float* out, int accumulate, g2v_stream_t stream);
size_t g2v_attn_bwd_workspace(int B, int H);
int g2v_attn_bwd(const float* d_ctx, int64_t ldd, const float* hp, const float* ep, const float* enc, const float* v,
                 const float* weights, float* d_hp, float* d_ep, float* d_enc, float* d_v, int accumulate, int T, int B,
                 int H, void* workspace, size_t workspace_bytes, g2v_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K13 + K14 (SURVEY.md 8(b) "attn_code_rollout_fwd/bwd"): the greedy gesture-code decoder of Part d as FUSED PER-STEP KERNELS.
 * Replaces the loop model/text2embedding_model.py:701-744 over BahdanauAttnDecoderRNN.forward (:338-395), n_layers == 2,
 * discrete_representation (code ids in, logits out):
 *   e_t   = Dropout(0.5)(Embedding(id_t))                                  (:340-343; keep_emb, scale 2)
 *   [att] w_t = softmax_tw( v . tanh(attn([h1_{t} ; enc[tw]])) ), ctx_t = sum_tw w_t[tw] enc[tw]; x_t = [e_t | ctx_t]   (:347-359)
 *   u_t   = x_t W_pre^T + b_pre;  a_t = ReLU(BatchNorm1d(u_t))              (:376, batch statistics when training)
 *   h0_{t+1}, h1_{t+1} = GRU(a_t; h0_t, h1_t)  (inter-layer dropout p on h0: keep_l0)      (:380)
 *   logits_t = h1_{t+1} W_out^T + b_out                                     (:390)
 *   id_{t+1} = codes[t+1] while t + 1 < n_pre, else argmax_k logits_t (lowest index on ties)    (:737-744)
 * for t = 0 .. S1-1 (S1 = sentence_frame_length // n_frames - 1; id_0 = codes[0]).  The step is row-local except for
 * BatchNorm's batch statistics, so the forward is S1 + 1 launches of ONE kernel (16 batch rows per 512-thread workgroup; launch j =
 * [BatchNorm finish of u_{j-1}, both GRU cells, out layer, argmax] + [embedding, attention, pre_linear of step j, per-workgroup
 * partial sums]); every contraction is v_mfma_f32_16x16x4_f32 on weights packed once per call.  Without attention nothing in
 * the BACKWARD couples batch rows between steps (the argmax feedback carries no gradient), so the whole BPTT over the S1 steps is
 * ONE launch (carries in LDS), followed by the BatchNorm backward of all steps at once and the batched products that do not
 * feed the recurrence (embedding gradient, every weight gradient over the S1 x B rows).  With attention the context gradient
 * needs BatchNorm's backward sums of the same step: the backward is S1 launches, each [BatchNorm backward finish of step t+1 ->
 * d(input) -> attention backward -> d(h1_t)] + [cells of step t].
 * H % 4 == 0, H <= 256, K <= 1024, Tw <= 64; g2v_attn_code_rollout_ok() says whether a shape is served (0: chain the operators
 * above from the host, as rounds 1-4 did).  All arrays caller-owned, time-major, fp32 unless said.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* emb;              /* (K,H)    decoder.embedding.weight                         */
  const float* w_pre;            /* (H,Hin)  decoder.pre_linear.0.weight; Hin = H, or 2H with attention */
  const float* b_pre;            /* (H)                                                       */
  const float* bn_w;             /* (H)      pre_linear.1.weight                              */
  const float* bn_b;             /* (H)                                                       */
  float* bn_running_mean;        /* (H)      updated once per step when training; both NULL while training: left alone
                                  *          (the caller commits them later: g2v_bn_running_update_invstd on bn_stats)        */
  float* bn_running_var;         /* (H)                                                       */
  const float* w_ih0; const float* w_hh0; const float* b_ih0; const float* b_hh0;   /* (3H,H), (3H) */
  const float* w_ih1; const float* w_hh1; const float* b_ih1; const float* b_hh1;
  const float* w_out;            /* (K,H)    decoder.out.weight                               */
  const float* b_out;            /* (K)                                                       */
  const float* w_attn;           /* (H,2H)   attn.attn.weight: [:, :H] on the state, [:, H:] on the encoder outputs; NULL = no attention */
  const float* b_attn;           /* (H)                                                       */
  const float* v_attn;           /* (H)      attn.v                                           */
} g2v_code_dec_weights;

typedef struct {                 /* outputs + saved for backward                              */
  int64_t* ids;                  /* (S1,B)    the code fed at every step                      */
  float* ec;                     /* (S1,B,Hin) dropped embedding [| context]                  */
  float* u;                      /* (S1,B,H)                                                  */
  float* a;                      /* (S1,B,H)                                                  */
  float* bn_stats;               /* (S1,2,H)  batch mean / 1/sqrt(biased var + eps) per step  */
  float* h0;                     /* (S1+1,B,H) slot t = state in front of step t              */
  float* h1;                     /* (S1+1,B,H)                                                */
  float* x1;                     /* (S1,B,H)  dropped h0_{t+1} (layer 1's input); NULL without inter-layer dropout */
  float* gates0;                 /* (S1,B,4H) r, z, n, W_hn h + b_hn                          */
  float* gates1;                 /* (S1,B,4H)                                                 */
  float* logits;                 /* (S1,B,K)                                                  */
  float* bn_partial;             /* (2,nblk,2,H) scratch, nblk = g2v_attn_code_rollout_blocks(B) */
  float* hp;                     /* (S1,B,H)  attention: h1_t W_attn[:, :H]^T + b_attn; NULL without attention */
  float* attw;                   /* (S1,B,Tw) attention weights                               */
} g2v_code_dec_saved;

typedef struct {                 /* gradients (overwritten)                                   */
  float* d_hidden0;              /* (2,B,H)   w.r.t. the initial state                        */
  float* d_emb;                  /* (K,H)                                                     */
  float* d_w_pre; float* d_b_pre; float* d_bn_w; float* d_bn_b;
  float* d_w_ih0; float* d_w_hh0; float* d_b_ih0; float* d_b_hh0;
  float* d_w_ih1; float* d_w_hh1; float* d_b_ih1; float* d_b_hh1;
  float* d_w_out; float* d_b_out;
  float* d_w_attn; float* d_b_attn; float* d_v_attn;      /* attention only                    */
  float* d_enc;                  /* (Tw,B,H)  w.r.t. the encoder outputs (context + energies)  */
} g2v_code_dec_grads;

/* Which kernels run one training call of the code decoder -- its forward and the backward behind it -- is decided once, from its
 * sizes, the caller's row count for the fused pair, the G2V_OPT_PERSISTENT level, the device's CU count and a few facts of the
 * call; g2v_attn_code_rollout_route reports the decision (host arithmetic only, no launch).  nblk = ceil(B / 16) row groups,
 * nt = ceil(H / 16) hidden-unit tiles.
 *   served    n_layers == 2, S1 >= 1, B >= 1, 16 <= H <= 256, H % 4 == 0, 4 <= K <= 1024, K % 4 == 0, with attention 1 <= Tw <= 64,
 *             and the step kernels' LDS carves within 160 KB (which in effect ends H at 224, and K at 688 where H = 200).
 *   grid      no attention, H <= 208, level >= 1 and nt * nblk <= CUs (B <= 304 at H = 200 on 256 CUs): a CU per workgroup of
 *             the (hidden-unit tile x row group) grid of either cluster kernel.
 *   pair      the caller is the C entry itself (G2V_CODE_PLAN_ENTRY), or B >= fused_min_rows.
 *                           forward                                           backward
 *   CLUSTER   code_cluster_fwd_kernel, ONE launch: served, grid,              g2v_code_cluster_bptt (code_cluster_bptt_kernel, ONE
 *             ceil(K / 16) <= 3 nt; and pair, or the caller accepts it        launch), then the caller's batched tail: a forward
 *             below the pair's row count                                      CLUSTER without pair, the cluster BPTT accepted
 *   STEP      S1 + 1 launches of code_step_fwd_kernel: pair, served,          g2v_attn_code_rollout_bwd: pair.  Variant 0, no
 *             not CLUSTER                                                     attention: code_bptt_kernel, one launch; variant 1,
 *                                                                             attention: code_step_bwd_att_kernel, one per step
 *   CHAIN     the operators one by one from the host: everything else         the same; also behind a forward CLUSTER without pair
 *                                                                             where the cluster BPTT is not accepted
 * So STEP goes with STEP and CHAIN with CHAIN; a forward CLUSTER goes with STEP from fused_min_rows rows on -- the entry takes the
 * cluster kernel whenever it can, which no switch of the caller's but the level turns off: asking for the fused pair at a small
 * batch does NOT force the step forward -- and with CLUSTER or CHAIN below.  CHAIN is an answer for the caller only: the entries
 * never run it.  With G2V_CODE_PLAN_ENTRY a shape that is not served returns 0, as the entries refuse it (G2V_ERR_UNSUPPORTED).
 * What only the call itself can tell may still move a forward CLUSTER to STEP inside the entry, silently and with equal results:
 * the cluster kernel not resident at a workgroup per CU (asked of the runtime only once the plan says CLUSTER).
 * g2v_attn_code_rollout_route returns G2V_CODE_ROUTE_* in bits 0..7 and the variant above, or 0 for a call the entries refuse.
 * backward: 0 the forward, 1 the backward, 2 g2v_code_cluster_bptt called by itself (K, Tw, layers and fused_min_rows are not read;
 * CLUSTER where grid holds, else 0).  persistent: the level, -1 = the bound context's; cus: the CU count, 0 = the device's (none:
 * no grid fits); facts: G2V_CODE_PLAN_* (0: a caller above the entries that accepts both cluster kernels, workspaces as queried). */
#define G2V_CODE_ROUTE_CLUSTER 1
#define G2V_CODE_ROUTE_STEP 2
#define G2V_CODE_ROUTE_CHAIN 3
#define G2V_CODE_PLAN_ENTRY 1            /* the C entry itself is called: pair holds at every B; not served = refused */
#define G2V_CODE_PLAN_NO_CLUSTER_FWD 2   /* without pair the caller does not take the cluster forward: CHAIN / CHAIN */
#define G2V_CODE_PLAN_NO_CLUSTER_BPTT 4  /* ... takes the forward but not the cluster BPTT: CLUSTER / CHAIN */
#define G2V_CODE_PLAN_WS_SMALL 8         /* the workspace is below the size query's answer, so too small for the records as well: a call
                                            that runs a kernel is refused (G2V_ERR_WORKSPACE) */
int g2v_attn_code_rollout_route(int backward, int S1, int B, int H, int K, int Tw, int attention, int layers, int fused_min_rows,
                                int persistent /* -1: the bound context's */, int cus /* 0: the device's */, int facts);
/* 1 where the entries serve the shape: g2v_attn_code_rollout_route(.., G2V_CODE_PLAN_ENTRY) != 0 (0: chain the operators above
 * from the host, as rounds 1-4 did) */
int g2v_attn_code_rollout_ok(int S1, int B, int H, int K, int Tw, int attention);
/* 1 where g2v_attn_code_rollout_fwd runs the shape as CLUSTER under the bound context's level on this device
 * (g2v_attn_code_rollout_route, forward, G2V_CODE_PLAN_ENTRY).  The cluster kernel writes the same arrays as the step kernels,
 * so g2v_attn_code_rollout_bwd or a per-operator backward run on them unchanged. */
int g2v_attn_code_rollout_cluster_ok(int S1, int B, int H, int K, int attention);
/* Round 5: where `grid` holds (g2v_attn_code_rollout_route, backward = 2), the BPTT through the two GRU cells of the attention-free
 * rollout as ONE persistent cluster launch
 * (code_cluster_bptt_kernel: the partial-product exchange of the pose decoder's backward cluster).  Nothing but the cells couples
 * two steps there (the greedy feedback carries no gradient), so the caller forms dh_top (S1,B,H) = dLogits W_out for all steps
 * first (g2v_linear_bwd_data) and runs BatchNorm's backward, the embedding gradient and every weight gradient afterwards over all
 * steps at once.  Writes dgi0 / dgh0 / dgi1 / dgh1 (S1,B,3H), da (S1,B,H) = the gradient w.r.t. a_t = ReLU(BN(u_t)) before the
 * ReLU mask, d_hidden0 (2,B,H); reads s->gates0 / gates1 / h0 / h1; keep_l0 (S1,B,H) or NULL: the inter-layer dropout masks. */
size_t g2v_code_cluster_bptt_workspace(int B, int H);
int g2v_code_cluster_bptt(const float* dh_top, const g2v_code_dec_weights* w, const g2v_code_dec_saved* s, const uint8_t* keep_l0,
                          float p_drop, float* dgi0, float* dgh0, float* dgi1, float* dgh1, float* da, float* d_hidden0,
                          int S1, int B, int H, void* workspace, size_t workspace_bytes, g2v_stream_t stream);
int g2v_attn_code_rollout_blocks(int B);
size_t g2v_attn_code_rollout_fwd_workspace(int H, int K, int attention);
/* codes (S,B) int64 (rows 0 .. max(1, n_pre) - 1 are read); h_init (2,B,H); enc (Tw,B,H) and enc_proj = enc W_attn[:, H:]^T
 * (Tw,B,H) with attention, else NULL; keep_emb / keep_l0 (S1,B,H) uint8 keep masks (NULL: no dropout; training == 0: eval
 * BatchNorm on the running statistics). */
int g2v_attn_code_rollout_fwd(const int64_t* codes, const float* h_init, const float* enc, const float* enc_proj,
                              const g2v_code_dec_weights* w, const g2v_code_dec_saved* s, const uint8_t* keep_emb,
                              const uint8_t* keep_l0, float p_drop, int n_pre, int training, int S1, int B, int H, int K,
                              int Tw, void* workspace, size_t workspace_bytes, g2v_stream_t stream);
size_t g2v_attn_code_rollout_bwd_workspace(int S1, int B, int H, int K, int Tw, int attention);
/* d_logits (S1,B,K); everything else as passed to the forward of the same call.
 * Alignment.  The three entries refuse, before any launch, with "16-byte alignment" (G2V_ERR_ARG), an array their
 * kernels move as float4s or as words of four keep flags that does not start on a 16-byte boundary; the arrays they move one
 * element at a time need their element's alignment only.
 *   g2v_attn_code_rollout_fwd   16 bytes: h_init, enc, enc_proj, keep_emb, keep_l0, workspace, every member of the weights but
 *                               w_attn and bn_running_mean / _var, every member of the saved arrays but ids, bn_stats and attw.
 *                               Element-wise: codes, ids, w_attn, bn_running_mean / _var, bn_stats, attw.
 *   g2v_attn_code_rollout_bwd   16 bytes: d_logits, enc, enc_proj, keep_emb, keep_l0, workspace, w_pre, bn_w, v_attn, every saved
 *                               array it is passed (ids included), every member of the gradients.  Element-wise: w_ih0 / w_hh0 /
 *                               w_ih1 / w_hh1, w_out, w_attn.  The other weights are not read.
 *   g2v_code_cluster_bptt       16 bytes: dh_top, keep_l0, dgi0 / dgh0 / dgi1 / dgh1, da, d_hidden0, gates0 / gates1, h0, h1,
 *                               workspace.  Element-wise: w_ih0 / w_hh0 / w_ih1 / w_hh1.  Nothing else is read. */
int g2v_attn_code_rollout_bwd(const float* d_logits, const float* enc, const float* enc_proj, const g2v_code_dec_weights* w,
                              const g2v_code_dec_saved* s, const g2v_code_dec_grads* g, const uint8_t* keep_emb,
                              const uint8_t* keep_l0, float p_drop, int S1, int B, int H, int K, int Tw, void* workspace,
                              size_t workspace_bytes, g2v_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Part d on continuous latents (text2_embedding_discrete: False; reference model/text2embedding_model.py:338-395, 701-744):
 * the attention-free decoder that regresses each chunk's latent vector (width E = n_layers * hidden_size), csrc/t2e_latent.hip.
 *   x_t   = target[t] while t < max(1, n_pre), else y_{t-1} -- the previous OUTPUT, with its gradient (:741)
 *   u_t   = x_t W_pre^T + b_pre;  a_t = ReLU(BatchNorm1d(u_t))  (batch statistics: this is the training forward)
 *   h0_{t+1}, h1_{t+1} = GRU(a_t; h0_t, h1_t)  (inter-layer dropout p on h0: keep_l0)
 *   y_t   = h1_{t+1} W_out^T + b_out
 * for t = 0 .. S1-1.  No embedding, no Dropout(0.5), no argmax.  The forward is S1 + 1 launches of one kernel (the tiling of
 * g2v_attn_code_rollout_fwd).  The backward cannot be the discrete decoder's single launch: d loss / d y_t = d_out_t +
 * du_{t+1} W_pre where step t+1 was fed back, and du_{t+1} comes out of BatchNorm's backward of step t+1, a sum over all batch
 * rows -- so it is S1 + 1 launches of one kernel, descending, a kernel boundary per step as the only grid-wide seam (no kernel waits
 * on another workgroup); every weight and bias gradient is one batched product over the S1 x B rows behind the loop.
 * The structs of the code decoder are reused with K := E: w_pre (H,E), w_out (E,H), b_out (E); s->ec (S1,B,E) = the x rows,
 * s->logits (S1,B,E) = y; emb, ids, d_emb, hp, attw and every attention member are NULL (w_attn != NULL is refused).
 * g2v_latent_rollout_ok() is 0 with attention and for shapes not served (H % 4 == 0, H <= 256, E % 4 == 0, E <= 1024, the
 * tiles within the CU's 160 KB of LDS): chain the operators from the host there.  target (S1+1,B,E) step-major (slots
 * 0 .. max(1, n_pre) - 1 are read); h_init (2,B,H); d_out (S1,B,E) = d loss / d y as the loss alone gives it.
 * ------------------------------------------------------------------------------------------ */
int g2v_latent_rollout_ok(int S1, int B, int H, int E, int attention);
size_t g2v_latent_rollout_fwd_workspace(int H, int E);
int g2v_latent_rollout_fwd(const float* target, const float* h_init, const g2v_code_dec_weights* w, const g2v_code_dec_saved* s,
                           const uint8_t* keep_l0, float p_drop, int n_pre, int S1, int B, int H, int E, void* workspace,
                           size_t workspace_bytes, g2v_stream_t stream);
size_t g2v_latent_rollout_bwd_workspace(int S1, int B, int H, int E);
int g2v_latent_rollout_bwd(const float* d_out, const g2v_code_dec_weights* w, const g2v_code_dec_saved* s,
                           const g2v_code_dec_grads* g, const uint8_t* keep_l0, float p_drop, int n_pre, int S1, int B, int H, int E,
                           void* workspace, size_t workspace_bytes, g2v_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The text -> pose seq2seq baseline (reference model/seq2seq_net.py:92-257, Seq2SeqNet): the continuous decoder WITH Bahdanau
 * attention, fed back with its gradient, as fused per-step kernels (csrc/pose_attn.hip).
 *   x_t   = target[t] while t < max(1, n_pre), else y_{t-1} -- the previous OUTPUT, with its gradient (:252-255)       (D)
 *   w_t   = softmax_tw( v . tanh(h1_t W_attn[:, :H]^T + b_attn + enc_proj[tw]) ) over ALL Tw positions (no length mask)
 *   c_t   = sum_tw w_t[tw] enc[tw]                                                                                   (H)
 *   u_t   = [x_t | c_t] W_pre^T + b_pre;  a_t = ReLU(BatchNorm1d(u_t))  (batch statistics: this is the training forward)
 *   h0_{t+1}, h1_{t+1} = GRU(a_t; h0_t, h1_t)  (inter-layer dropout p on h0: keep_l0);   y_t = h1_{t+1} W_out^T + b_out
 * for t = 0 .. S1-1; h1_t is the top state in front of the step's GRU.  Forward: S1 + 1 launches of one kernel; backward: S1 + 1
 * launches of one kernel, descending (the launch of step t finishes BatchNorm's backward of step t+1, splits du_{t+1} W_pre into
 * the feedback into d y_t and d c_{t+1}, and runs the attention backward of step t+1 in front of the cells of step t); a kernel
 * boundary is the only grid-wide seam, no kernel waits on another workgroup, no float atomics.  Every weight and bias gradient is
 * one batched product over the S1 x B rows behind the loop.
 * The structs of the code decoder are reused with K := D (as g2v_latent_rollout_*): w_pre (H, D + H), w_out (D,H), b_out (D),
 * w_attn (H,2H), b_attn, v_attn; s->logits (S1,B,D) = y; s->hp (S1,B,H), s->attw (S1,B,Tw); s->ec (S1,B,ldec) = the input rows
 * [x | c], D + H floats at the row stride ldec = round_up(D + H, 4); emb, ids are not read.
 * Gradients: everything in g2v_code_dec_grads but d_emb is what its name says, with
 *   d_enc    (Tw,B,H)  the CONTEXT term only (sum_t w_t[tw] d c_t);
 *   d_emb    (Tw,B,H)  this mode has no embedding: the member carries d loss / d enc_proj, so that no struct changes;
 *   d_w_attn (H,2H)    [:, :H] = the state half, [:, H:] = 0.
 * The enc_proj -> enc path through W_attn[:, H:] stays with the caller, as for g2v_attn_bwd: d W_attn[:, H:] = d_enc_proj^T enc
 * (g2v_linear_bwd_weight) and d enc += d_enc_proj W_attn[:, H:] (g2v_linear_bwd_data).
 * Served (g2v_pose_attn_rollout_ok): S1 >= 1, B >= 2 (train-mode BatchNorm has no variance at one row), 16 <= H <= 256, H % 4 == 0,
 * 1 <= D <= 256 -- D % 4 != 0 included: D = 135 is the width the model is trained at --, 1 <= Tw <= 64, both LDS carves within
 * 160 KB (which in effect ends H at 224).  g2v_pose_attn_rollout_plan is the ONE decision between the per-operator chain (0) and
 * these entries (1): served and B >= fused_min_rows; C and Python ask it.
 * target (S1+1,B,D) step-major (slots 0 .. max(1, n_pre) - 1 are read); h_init (2,B,H); enc, enc_proj (Tw,B,H);
 * d_out (S1,B,D) = d loss / d y as the loss alone gives it; keep_l0 (S1,B,H) uint8 or NULL.
 * Alignment.  Both entries refuse, before any launch, with "16-byte alignment" (G2V_ERR_ARG), an array their kernels move as
 * float4s or as words of four keep flags that does not start on a 16-byte boundary; the arrays they move one element at a time
 * need their element's alignment only.  At D % 4 != 0 the rows of target, y (s->logits) and d_out are not 16-byte aligned: those
 * arrays, b_out and the context half of an ec row move element-wise; nothing is staged at a padded stride of its own.
 *   g2v_pose_attn_rollout_fwd   16 bytes: h_init, enc, enc_proj, keep_l0, workspace, every bias, bn_w / bn_b, v_attn, every saved
 *                               array but bn_stats and attw; at D % 4 == 0 also target, s->logits and b_out.  Element-wise: the
 *                               weight matrices, bn_running_mean / _var, bn_stats, attw.
 *   g2v_pose_attn_rollout_bwd   16 bytes: enc, enc_proj, keep_l0, workspace, bn_w, v_attn, every saved array it reads but attw
 *                               (bn_stats included), d_hidden0, d_enc, d_emb; at D % 4 == 0 also d_out.  Element-wise: the weight
 *                               matrices, attw; the other gradients go to the dense kernels, which choose their own widths.
 * ------------------------------------------------------------------------------------------ */
int g2v_pose_attn_rollout_ok(int S1, int B, int H, int D, int Tw);
int g2v_pose_attn_rollout_plan(int S1, int B, int H, int D, int Tw, int fused_min_rows);
size_t g2v_pose_attn_rollout_fwd_workspace(int H, int D);
int g2v_pose_attn_rollout_fwd(const float* target, const float* h_init, const float* enc, const float* enc_proj,
                              const g2v_code_dec_weights* w, const g2v_code_dec_saved* s, const uint8_t* keep_l0, float p_drop,
                              int n_pre, int S1, int B, int H, int D, int Tw, void* workspace, size_t workspace_bytes,
                              g2v_stream_t stream);
size_t g2v_pose_attn_rollout_bwd_workspace(int S1, int B, int H, int D, int Tw);
int g2v_pose_attn_rollout_bwd(const float* d_out, const float* enc, const float* enc_proj, const g2v_code_dec_weights* w,
                              const g2v_code_dec_saved* s, const g2v_code_dec_grads* g, const uint8_t* keep_l0, float p_drop,
                              int n_pre, int S1, int B, int H, int D, int Tw, void* workspace, size_t workspace_bytes,
                              g2v_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Calibration probes used by bench.py to report what the box sustains next to the datasheet peaks (no counterpart in the
 * reference): g2v_probe_mfma_f32 runs `blocks` x 4 waves x `iters` x 8 independent v_mfma_f32_16x16x4_f32 (2048 flop each)
 * without memory traffic (scratch: blocks * 256 floats); g2v_probe_copy streams n floats from src to dst.
 * ------------------------------------------------------------------------------------------ */
int g2v_probe_mfma_f32(float* scratch, int blocks, int iters, g2v_stream_t stream);
int g2v_probe_copy(const float* src, float* dst, int64_t n, g2v_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Keep-mask generator: keep[i] = (philox4x32-10(seed, offset_counter, i) uniform < keep_prob).
 * Replaces the RNG draws of nn.Dropout / nn.GRU dropout on the path (e.g. :570).  offset_counter is a
 * device int64 that the call advances by 1 (so graph replays draw fresh masks).
 * ------------------------------------------------------------------------------------------ */
int g2v_keep_mask(uint8_t* keep, int64_t n, float keep_prob, uint64_t seed, int64_t* offset_counter,
                  g2v_stream_t stream);
/* The same stream at offset_counter[0] + offset_add WITHOUT advancing the counter, and the advance as its own call: several
 * masks of one step (offset_add = 0, 1, 2 ...) then cost one counter launch instead of one each. */
int g2v_keep_mask_at(uint8_t* keep, int64_t n, float keep_prob, uint64_t seed, const int64_t* offset_counter, int64_t offset_add,
                     g2v_stream_t stream);
int g2v_counter_add(int64_t* counter, int64_t n, g2v_stream_t stream);
/* g2v_keep_mask_at + g2v_mask_rows in one kernel, without the mask tensor: out[m, k] = keep(m K + k) ? x[row(m), k] * scale : 0
 * with keep(e) = element e of the stream (seed, offset_counter[0] + offset_add) -- bit for bit what the two calls produce. */
int g2v_dropout_rows(const float* x, int64_t ldx, int rows_inner, int64_t stride_outer, int64_t stride_inner, float keep_prob,
                     float scale, uint64_t seed, const int64_t* offset_counter, int64_t offset_add, float* out, int64_t ldo,
                     int M, int K, g2v_stream_t stream);

/* small helpers used by the host */
int g2v_fill_f32(float* p, float v, int64_t n, g2v_stream_t stream);
/* dst[k][i] = src[k][i] for i < n[k], k < nseg (src[k] == NULL: zero fill), all segments in one launch per 48.  src / dst /
 * n are HOST arrays (read at launch).  FlatParams.gather_grads: every parameter's .grad into the flat gradient buffer that
 * g2v_clip_adam_step consumes (torch.nn.utils.clip_grad_norm_ + Adam.step over a parameter list, train_seq2seq.py:540-546). */
int g2v_copy_segments(const float* const* src, float* const* dst, const int64_t* n, int nseg, g2v_stream_t stream);
/* out[i] = in[i] * scalar[0]   (scalar is a DEVICE float: chains an upstream autograd scalar without a host sync) */
int g2v_scale_f32(const float* in, const float* scalar, float* out, int64_t n, g2v_stream_t stream);
/* out[i] = on(i) ? in[i]*scale : 0, on(i) = keep[i] != 0 (uint8 mask) or, when keep is NULL, positive_of[i] > 0
 * (dropout / ReLU backward of the thin dense models). */
int g2v_mask_mul(const float* in, const uint8_t* keep, const float* positive_of, float scale, float* out,
                 int64_t n, g2v_stream_t stream);
/* out[m, k] = keep[m K + k] ? x[row(m), k] * scale : 0 for m < M, k < K -- the dropped input of a dense layer as a tensor of its
 * own (row addressing of x as in g2v_linear_fwd; out rows at stride ldo).  The encoder's input dropout
 * (model/Autoencoder_VQVAE_model.py:88-93: self.do(inputs) in front of in_layer) uses it once per step, so that the forward
 * product and the weight-gradient product both run on their unmasked fast kernels. */
int g2v_mask_rows(const float* x, int64_t ldx, int rows_inner, int64_t stride_outer, int64_t stride_inner, const uint8_t* keep,
                  float scale, float* out, int64_t ldo, int M, int K, g2v_stream_t stream);
int g2v_transpose(const float* in, float* out, int rows, int cols, g2v_stream_t stream); /* out[c][r] = in[r][c] */
/* out[m, 0:H] = a[m, 0:H] + b[m, 0:H] with row strides (sum of the two GRU directions, :95-97) */
int g2v_add_halves(const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int64_t ldo,
                   int64_t M, int H, g2v_stream_t stream);

/* ---- evaluation statistics (metrics.hip; gesture2vec_amd/metrics.py) ----------------------------------------------------------
 * Shifted first and second moments of the rows of x (N x E fp32, row stride ld >= E elements), ADDED to float64 accumulators:
 *   s1[E]    += sum_n (x_n - shift)
 *   s2[E][E] += sum_n (x_n - shift)(x_n - shift)^T     stored full: the upper triangle is computed (fp32 MFMA, exact fp32 products)
 *                                                       and mirrored, so s2[i][j] == s2[j][i] bit for bit.
 * x - shift is rounded once to fp32; fp32 accumulation chains are at most 1024 rows long and are folded into float64 in a fixed
 * order: no floating-point atomics, the same input gives the same bits.  The sums are additive over calls (and over ranks) that use
 * the same shift.  1 <= E <= 512 (G2V_ERR_UNSUPPORTED beyond), any N >= 1.  x is read once for E <= 400, twice for wider rows.
 * workspace: g2v_moments_workspace(N, E) bytes, 16-byte aligned; its contents are not trusted across calls. */
size_t g2v_moments_workspace(int64_t N, int E);
int g2v_moments_accumulate(const float* x, int64_t ld, const float* shift, double* s1, double* s2, int64_t N, int E,
                           void* workspace, size_t workspace_bytes, g2v_stream_t stream);
/* counts[k] += #{n : idx[n] == k} for k < K; ids outside [0, K) are counted in counts[K] and never used as an address.
 * counts: int64[K + 1].  Integer atomics only: exact and order-independent. */
int g2v_code_histogram(const int64_t* idx, int64_t N, int K, int64_t* counts, g2v_stream_t stream);
/* Clipped n-gram match counts of B independent (candidate, reference) pairs of code-id sequences (ngram.hip): the integer half of
 * BLEU over code sequences (torchtext's bleu_score with one reference per candidate, Clustering.py:1560-1609):
 *   clipped[b][n-1] = sum over the distinct n-grams g of candidate b of min(count in the candidate, count in the reference), n = 1 .. max_n
 *   (= sum((Counter(candidate n-grams) & Counter(reference n-grams)).values())).
 * Sequence b of `cand` is the cand_len[b] ids from element cand_start[b] on, the same for `ref`: one entry serves a padded (B, L)
 * tensor (start = b * row stride; what lies past a length is not read) and a ragged concatenation.  The starts are the caller's
 * addresses and are trusted; the lengths live on the device and are not read back: max_len is the caller's upper bound on all of
 * them and picks the kernel (max_len <= 64: one wavefront per pair, the rank form over LDS broadcasts; longer: one workgroup per
 * pair, both key arrays sorted in LDS, run starts matched by binary search).
 * 1 <= max_n <= 4, 1 <= K <= 65536 (an n-gram is one 64-bit key of 16-bit ids), 0 <= max_len <= 4096: G2V_ERR_UNSUPPORTED above,
 * G2V_ERR_ARG below, B < 1 or a null pointer, all before any launch (nothing is written).  A length below n gives 0 for order n.
 * A pair with a length outside [0, max_len] or an id outside [0, K) gets -1 in its max_n slots and adds 1 to bad[0] (int64[1],
 * cleared by the caller; an integer atomic); its out-of-range values are never used as an address or a key, the other pairs are
 * untouched.  clipped: int64[B][max_n].  Integer arithmetic only: exact, the same bits on every run, a pair's counts do not depend on
 * the rest of the batch.  No workspace. */
int g2v_ngram_clipped_counts(const int64_t* cand, const int64_t* cand_start, const int64_t* cand_len, const int64_t* ref,
                             const int64_t* ref_start, const int64_t* ref_len, int64_t* clipped, int64_t* bad, int64_t B, int K,
                             int max_n, int max_len, g2v_stream_t stream);

/* ---- k-means over latent rows (kmeans.hip; gesture2vec_amd/kmeans.py) -------------------------------------------------------------
 * The reference fits sklearn.cluster.KMeans on the (N, L*H) chunk latents of a quantiser-free autoencoder (Clustering.py:705-725) and
 * calls kmeanmodel.predict for Part d's cluster ids (lmdb_data_loader.py:1097-1103).  The assignment half of a Lloyd iteration is
 * g2v_vq_assign_fwd / g2v_vq_assign_packed_fwd (exact fp32 argmin, lowest index on ties); the rest is here.
 *
 * g2v_kmeans_update: x (N,E) fp32, labels (N) int64 (ids outside [0,K) are ignored), prev_labels (N) or NULL, centers_old (K,E) ->
 *   counts[K] int64, sums[K][E] float64, centers_new[K][E] = (float)(sum / count) (a cluster without rows keeps centers_old),
 *   stats[4] float64 = { inertia = sum_n |x_n - centers_old[label_n]|^2 (from the rows, not from an assign kernel's distances),
 *                        shift = sum_k |centers_new_k - centers_old_k|^2, n_changed = #{n: labels[n] != prev_labels[n]} (N when
 *                        prev_labels is NULL), n_relocated }.
 *   x is read once through an inverted index (stable counting sort of the row ids by label); lists are cut into chunks of 512 rows,
 *   one wave sums a chunk in float64 and the chunks of a cluster are added in chunk order: no floating-point atomics, the same input
 *   gives the same bits.  relocate != 0: sklearn's _relocate_empty_clusters_dense in a fixed order -- the empty clusters in ascending
 *   id take the n_empty rows with the largest |x - centers_old[label]|^2, farthest first, lowest row among equals; a chosen row leaves
 *   its cluster's sum and count and becomes the empty cluster's sum with count 1; labels are not touched.  relocated_rows (may be
 *   NULL): its first n_relocated entries receive the chosen rows.
 *   state (may be NULL): float64[8] = { done, n_iter, n_changed, shift, inertia, n_relocated, active, tol_abs }, zeroed by the caller
 *   before a fit except tol_abs.  With a state block the call is a NO-OP once done != 0 (active = 0 then); otherwise it adds 1 to
 *   n_iter, stores the scalars, sets active = 1, and sets done when prev_labels was given and no label changed, or shift <= tol_abs.
 *   g2v_kmeans_commit copies centers_new -> centers and labels_new -> labels (either labels pointer may be NULL) when active != 0:
 *   a host may enqueue several assign / update / commit rounds per read-back and what it reads is the state at convergence.
 *   Needs E % 4 == 0, E <= 512 (G2V_ERR_UNSUPPORTED otherwise), 1 <= N < 2^31 - 2048, K >= 1; x, centers_old 16-byte aligned.
 * g2v_kmeans_tolerance: out[0] = tol * mean_e Var(x_e) (population variance; float64 column moments in one pass, fixed order).
 * g2v_kmeans_pp_step: one greedy k-means++ step (sklearn _kmeans_plusplus) over ncand <= 8 candidate rows.  closest (N) float64 holds
 *   the running squared distance to the nearest chosen centre (+inf before the first).  The rows are cut into g2v_kmeans_pp_blocks(N)
 *   blocks of 1024; candidate t is the first row of block pick_block[t] at which the running sum of closest[] over that block reaches
 *   pick_resid[t] (the last row of the block if none does) -- the host finds the block from the block sums of the previous step; with
 *   pick_resid == NULL pick_block[t] is the candidate row itself.  pick_block / pick_resid are HOST arrays, read at launch.
 *   d_t[n] = min(closest[n], |x_n - x_cand(t)|^2) in float64, potential_t = sum_n d_t[n]; the candidate with the lowest potential
 *   (lowest t among equals) wins: closest = d_best, center_out[E] = its row.
 *   out: float64[blocks + 11] = { block sums of the new closest[], potential_0..7, best t, chosen row, its potential }. */
size_t g2v_kmeans_update_workspace(int64_t N, int E, int K);
int g2v_kmeans_update(const float* x, const int64_t* labels, const int64_t* prev_labels, const float* centers_old,
                      int64_t N, int E, int K, int relocate, int64_t* counts, double* sums, float* centers_new,
                      double* stats, int64_t* relocated_rows, double* state, void* workspace, size_t workspace_bytes,
                      g2v_stream_t stream);
int g2v_kmeans_commit(const double* state, const float* centers_new, float* centers, int64_t n_center_elems,
                      const int64_t* labels_new, int64_t* labels, int64_t N, g2v_stream_t stream);
size_t g2v_kmeans_tolerance_workspace(int64_t N, int E);
int g2v_kmeans_tolerance(const float* x, int64_t N, int E, double tol, double* out, void* workspace, size_t workspace_bytes,
                         g2v_stream_t stream);
int g2v_kmeans_pp_blocks(int64_t N);
size_t g2v_kmeans_pp_workspace(int64_t N, int E);
int g2v_kmeans_pp_step(const float* x, int64_t N, int E, double* closest, G2V_HOST const int64_t* pick_block,
                       G2V_HOST const double* pick_resid, int ncand, double* out, float* center_out, void* workspace,
                       size_t workspace_bytes, g2v_stream_t stream);

/* ---- silhouette coefficient of a clustering of latent rows (silhouette.hip; gesture2vec_amd/silhouette.py) ------------------------
 * The second curve of the reference's k scan (Clustering.py:608-624, sklearn.metrics.silhouette_score).  x (N,E) fp32 with row stride
 * ld >= E elements, labels (N) int64.  With c = labels[i], n_c rows in c and d the Euclidean distance (not its square):
 *   a[i] = sum_{j in c, j != i} d(i,j) / (n_c - 1)      b[i] = min over the non-empty clusters c' != c of sum_{j in c'} d(i,j) / n_c'
 *   s[i] = (b - a) / max(a, b); 0 where n_c = 1 and where a = b = 0 (sklearn's nan_to_num).  The term i = j is exactly 0 by rule.
 *   a, b, s: float64[N].  counts: int64[K + 1] = rows per cluster, and in counts[K] the rows whose label is outside [0, K): those
 *   are in no cluster, are never used as an address, and keep a = b = s = 0.  out: float64[2] = { sum_i s[i] in a fixed order,
 *   number of non-empty clusters }.  With one non-empty cluster b = +inf and s = 0.
 *   The rows are sorted by label with the counting sort of g2v_kmeans_update; the Gram products run on the exact-fp32 MFMA from LDS
 *   tiles with sqrt in the accumulator epilogue, and a row's running sum is closed at each cluster boundary: neither the N x N
 *   distances nor an N x K table of sums exist.  A pair with d^2 < (|x_i|^2 + |x_j|^2) / 8 is re-evaluated as sum (x_i - x_j)^2 in
 *   float64 (bitwise equal rows: exactly 0), so no distance carries the cancellation of |x|^2 + |y|^2 - 2 x.y.  Every sum is formed
 *   in an order fixed by (N, E, K, ld), the data and the labels: no floating-point atomics, the same input gives the same bits.
 *   Needs E % 4 == 0, E <= 512, N + 16 K + 64 < 2^31 (G2V_ERR_UNSUPPORTED otherwise), 2 <= N < 2^31 - 2048, K >= 1, ld % 4 == 0;
 *   x and workspace 16-byte aligned.  workspace: g2v_silhouette_workspace(N, E, K) bytes (0 for an unsupported shape); its
 *   contents are not trusted across calls. */
size_t g2v_silhouette_workspace(int64_t N, int E, int K);
int g2v_silhouette_samples(const float* x, int64_t ld, const int64_t* labels, int64_t N, int E, int K, double* a, double* b,
                           double* s, int64_t* counts, double* out, void* workspace, size_t workspace_bytes, g2v_stream_t stream);

/* ---- exact t-SNE into the plane (tsne.hip; gesture2vec_amd/embedding.py) ------------------------------------------------------------
 * The reference's 2-D maps of the codebook and of the chunk latents (train_autoencoder_VQVAE.py:450-505, Clustering.py:1046-1056:
 * PCA(50) + sklearn.manifold.TSNE); the math is sklearn 1.7's exact method.  N <= g2v_tsne_max_rows() = 32768 rows (the joint P is
 * dense: N x N fp32 with row stride N, 4 GiB at the limit; every offset is 64-bit), G2V_ERR_UNSUPPORTED beyond.
 *
 * g2v_tsne_affinities: x (N,d) fp32 with row stride ld >= d, ld % 4 == 0, 1 <= d <= 512; 0 < perplexity < N -> the joint P, symmetric
 *   bit for bit, diagonal 0, every other entry >= DBL_EPSILON.  Squared distances |x_i|^2 + |x_j|^2 - 2 x_i.x_j with float64 norms and
 *   Gram tiles from the exact-fp32 MFMA (chains of 32 columns, folded in float64), rounded to fp32 once; a pair with
 *   d^2 < (|x_i|^2 + |x_j|^2) / 8 is re-evaluated as sum (x_i - x_j)^2 in float64 as g2v_silhouette_samples does (bitwise equal
 *   rows: exactly 0).  Elsewhere d^2 carries ~3e-7 of the 32-column partial sums of x_i.x_j: centre rows that lie far from the
 *   origin.  Per row, sklearn's
 *   bisection of the precision in float64: beta = 1, doubled / halved while a bound is infinite, at most 100 steps, stop at
 *   |H - log(perplexity)| <= 1e-5, a row sum of exactly 0 becomes 1e-8, the term j = i left out; the conditionals are kept as fp32.
 *   P_ij = max((c_ij + c_ji) / sum(C + C^T), DBL_EPSILON), the sum in float64 in a fixed order.  P and workspace 16-byte aligned;
 *   workspace: g2v_tsne_affinities_workspace(N, d) bytes (0 for an unsupported shape); its contents are not trusted across calls.
 * g2v_tsne_gradient: P as above, y (N,2) fp32 (8-byte aligned), exaggeration > 0 -> grad (N,2) fp32 and out float64[3] =
 *   { KL, sum grad^2 (of the fp32 values), Z } with p_ij = exaggeration P_ij, q_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} q_ij,
 *     grad_i = 4 sum_j (p_ij - q_ij / Z) q_ij (y_i - y_j)      KL = sum_{i != j} p_ij log(max(p_ij, DBL_EPSILON) / (q_ij / Z))
 *   (sklearn's _kl_divergence called with P * exaggeration; its clamp of q / Z at DBL_EPSILON is left out).  One pass over P; y_i - y_j
 *   and q in fp32, the attractive and repulsive row sums, Z and the KL terms in float64, combined once Z is known.  want_kl == 0
 *   skips the logarithms and stores NaN in out[0], as sklearn does.  workspace: g2v_tsne_gradient_workspace(N) bytes.
 * g2v_tsne_update: one step of sklearn's _gradient_descent over y, velocity and gains (N,2) fp32, in its fp32 operation order:
 *   gains += 0.2 where velocity * grad < 0, *= 0.8 elsewhere, floor 0.01; velocity = momentum velocity - learning_rate (gains grad);
 *   y += velocity.  gnorm2 (may be NULL): float64[1] = sum (gains grad)^2, the norm its stop rule reads.
 * No floating-point atomics anywhere: the same input gives the same bits. */
int64_t g2v_tsne_max_rows(void);
size_t g2v_tsne_affinities_workspace(int64_t N, int d);
int g2v_tsne_affinities(const float* x, int64_t ld, int64_t N, int d, double perplexity, float* P, void* workspace,
                        size_t workspace_bytes, g2v_stream_t stream);
size_t g2v_tsne_gradient_workspace(int64_t N);
int g2v_tsne_gradient(const float* P, const float* y, int64_t N, double exaggeration, int want_kl, float* grad, double* out,
                      void* workspace, size_t workspace_bytes, g2v_stream_t stream);
int g2v_tsne_update(float* y, float* velocity, float* gains, const float* grad, int64_t N, float momentum, float learning_rate,
                    double* gnorm2, g2v_stream_t stream);

/* ---- new rows into a fitted t-SNE map (tsne_place.hip; gesture2vec_amd/embedding.py: TSNE.transform, LatentMap) --------------------
 * The reference's make_unity_scatter(latents, labels, file, pca, MyTSNE) = MyTSNE.transform(pca.transform(latents))
 * (Clustering.py:1318-1350): openTSNE's structure and transform defaults, stated exactly; bit parity with openTSNE (approximate
 * neighbours, interpolated repulsion) is not claimed.  X (N,d) fp32 are the rows the map was fitted on, Y (N,2) fp32 their map,
 * Z (M,d) fp32 the new rows.  Every new row is its own problem and Y does not move: a row's result depends on that row, X, Y and the
 * parameters, not on M or on the other rows of the call, bit for bit.  1 <= N < 2^24, 1 <= M < 2^31, 1 <= kk <= min(N, 128).
 *
 * g2v_tsne_place_neighbors: X with row stride ldx, Z with row stride ldz (both >= d and % 4 == 0), 1 <= d <= 512 -> idx int32 (M,kk) and
 *   d2 fp32 (M,kk): per new row the kk nearest reference rows in ascending (d^2, index) order, ties to the lower index.  They are
 *   SELECTED on squared distances formed exactly as g2v_tsne_affinities forms them (float64 norms, Gram tiles on the exact-fp32 MFMA
 *   in chains of 32 columns folded in float64, rounded to fp32 once; d^2 < (|z|^2 + |x|^2) / 8 re-evaluated from differences in
 *   float64), so a row that differs from the kk-th nearest by less than ~3e-7 (|z|^2 + |x|^2) may take its place.  The kk kept
 *   distances are then evaluated once more as sum (z - x)^2 in float64, rounded to fp32 once, and the list is sorted again: d2 is the
 *   correctly rounded distance (a new row bitwise equal to a reference row is at exactly 0), which the conditionals need (the Gram
 *   form's error is ~20 roundings of d^2 on centred rows).  Columns d .. ld - 1 are never read.  The M x N distances are selected
 *   from as they are formed and never stored.  Any other shape: G2V_ERR_UNSUPPORTED.  X, Z and workspace 16-byte aligned;
 *   workspace: g2v_tsne_place_neighbors_workspace(N, M, d, kk) bytes (0 for an unsupported shape), not trusted across calls.
 * g2v_tsne_place_conditionals: d2 (M,kk) as above, 1 <= k_aff <= kk, 0 < perplexity < k_aff -> p fp32 (M,k_aff): over the first
 *   k_aff neighbours, the bisection of the precision of g2v_tsne_affinities (float64, beta = 1, doubled / halved while a bound is
 *   infinite, at most 100 steps, stop at |H - log(perplexity)| <= 1e-5, a row sum of exactly 0 becomes 1e-8) with no term left out.
 *   p is the conditional: not symmetrised, each row sums to 1.
 * g2v_tsne_place_init: the start y (M,2) fp32 from idx (M,kk) (and p (M,k_aff) for mode 1).  mode 0: per coordinate the median of Y
 *   over the first k_use <= kk neighbours, numpy's rule (an even count gives (a + b) * 0.5f of the two middle values).  mode 1:
 *   sum_j p_ij Y_j over the first k_use <= k_aff neighbours in float64, rounded once.
 * g2v_tsne_place_descent: n_iter steps on y, velocity, gains (M,2) fp32 in place, all inside one launch.  With
 *   w_ij = 1 / (1 + |y_i - Y_j|^2) and Z_i = sum_{j < N} w_ij,
 *     g_i = 2 [ exaggeration sum_{j in the k_aff neighbours} p_ij w_ij (y_i - Y_j)  -  (1 / Z_i) sum_{j < N} w_ij^2 (y_i - Y_j) ]
 *   y - Y and w in fp32 as g2v_tsne_gradient takes its q, the three sums and Z in float64 over j ascending, g rounded to fp32 once.
 *   A step, in fp32 in this order: n = sqrt(gx^2 + gy^2); if max_grad_norm > 0 and n > max_grad_norm, g *= max_grad_norm / n; gains
 *   += 0.2 where velocity * g < 0, *= 0.8 elsewhere, floor 0.01; velocity = momentum velocity - learning_rate (gains g);
 *   y += velocity.  After the last step one more sweep at exaggeration 1 gives, per row, kl float64 (M) = sum_j p_ij log(p_ij /
 *   (w_ij / Z_i)) (a p of exactly 0 adds nothing), zsum float64 (M) = Z_i and grad fp32 (M,2), the unclipped gradient; each may be
 *   NULL.  n_iter == 0 moves nothing, only evaluates them at y -- grad at the exaggeration given, which a closing sweep replaces
 *   by 1 -- and reads neither velocity nor gains (both may be NULL).  An entry of idx outside [0, N) is read as 0.  Y, y, velocity, gains and grad 8-byte aligned.  No workspace.
 * No floating-point atomics anywhere: the same input gives the same bits. */
size_t g2v_tsne_place_neighbors_workspace(int64_t N, int64_t M, int d, int kk);
int g2v_tsne_place_neighbors(const float* X, int64_t ldx, int64_t N, const float* Z, int64_t ldz, int64_t M, int d, int kk,
                             int32_t* idx, float* d2, void* workspace, size_t workspace_bytes, g2v_stream_t stream);
int g2v_tsne_place_conditionals(const float* d2, int64_t M, int kk, int k_aff, double perplexity, float* p, g2v_stream_t stream);
int g2v_tsne_place_init(const float* Y, int64_t N, const int32_t* idx, const float* p, int64_t M, int kk, int k_aff, int mode,
                        int k_use, float* y, g2v_stream_t stream);
int g2v_tsne_place_descent(const float* Y, int64_t N, const int32_t* idx, const float* p, int64_t M, int kk, int k_aff, float* y,
                           float* velocity, float* gains, int n_iter, double exaggeration, float momentum, float learning_rate,
                           float max_grad_norm, double* kl, double* zsum, float* grad, g2v_stream_t stream);

/* ---- ranks of given neighbours among all rows (map_quality.hip; gesture2vec_amd/embedding.py: trustworthiness, continuity) ---------
 * What sklearn.manifold.trustworthiness (sklearn 1.7, Euclidean) takes from two N x N float64 matrices and a full argsort of each,
 * without forming either: the neighbours of one space (g2v_tsne_place_neighbors) are ranked in the other.  X (N,d) fp32 with row
 * stride ldx are the reference rows, Z (M,d) fp32 with row stride ldz the query rows (Z = X for a map scored against itself; placed
 * rows against the fitted sample otherwise), idx int32 (M,k) lists rows of X per query, self int64 (M) or NULL names the row of X
 * that IS query m (-1: none), which is left out of every count.
 *   rank[m][s] = 1 + #{ l in [0,N), l != self[m] : (D(m,l), l) < (D(m,j), j) },  j = idx[m][s], in lexicographic order: the nearest
 *   other row has rank 1 and equal distances go to the lower index.  D(m,l) = sum (z_m - x_l)^2 in float64 from the differences.
 *   An entry j outside [0,N), or equal to self[m], gives rank 0.  rank: int32 (M,k).
 * The thresholds D(m,j) of the M k listed pairs are evaluated exactly first.  Every other d^2 is formed as g2v_tsne_affinities forms
 * it (float64 norms, Gram tiles on the exact-fp32 MFMA in chains of 32 columns folded in float64, rounded to fp32 once) and compared
 * with the k thresholds of its row; a comparison with |d^2 - D(m,j)| <= 2^-18 (|z_m|^2 + |x_l|^2), twice the worst case of the Gram
 * form's error, is decided again on sum (z_m - x_l)^2 in float64, so every count is the float64 count of the fp32 rows.
 * redecided (may be NULL): int64[1] = the pairs (m,l) evaluated again (a listed pair itself is not one: it is never below itself).
 * Counts are integers, added with integer operations only: the same input gives the same bits, however the columns are shared out
 * among workgroups.  Columns d .. ld - 1 are never read; the M x N distances are never stored.
 * Served: 1 <= d <= 512, ldx and ldz multiples of 4 and >= d, 1 <= k <= 127, 1 <= N < 2^24, 1 <= M < 2^31; anything else is
 * G2V_ERR_UNSUPPORTED before any launch, with rank untouched.  g2v_neighbor_ranks_ok: 1 where (N, M, d, k) is served.  X, Z and
 * workspace 16-byte aligned; workspace: g2v_neighbor_ranks_workspace(N, M, d, k) bytes (0 for an unsupported shape), not trusted
 * across calls. */
int g2v_neighbor_ranks_ok(int64_t N, int64_t M, int d, int k);
size_t g2v_neighbor_ranks_workspace(int64_t N, int64_t M, int d, int k);
int g2v_neighbor_ranks(const float* X, int64_t ldx, int64_t N, const float* Z, int64_t ldz, int64_t M, int d, const int64_t* self,
                       const int32_t* idx, int k, int32_t* rank, int64_t* redecided, void* workspace, size_t workspace_bytes,
                       g2v_stream_t stream);

/* ---- DBSCAN over latent rows (dbscan.hip; gesture2vec_amd/dbscan.py) ----------------------------------------------------------------
 * The other branch of the reference's clustering switch (Clustering.py:742-750, sklearn.cluster.DBSCAN(eps, min_samples).fit), with
 * sklearn's labels, not merely an equivalent partition.  With adj(i,j) <=> |x_i - x_j| <= eps (a row is its own neighbour):
 * core(i) <=> #{j : adj(i,j)} >= min_samples; root(i) = the smallest index in i's connected component of the core rows under adj;
 * a component's cluster id = the rank of its root among all roots; a row that is not core gets the smallest id among its core
 * neighbours, or -1 without one.  1 <= N <= g2v_dbscan_max_rows() = 131072 (the adjacency is a bitmap of N^2 / 8 bytes: 2 GiB at
 * the limit), 1 <= E <= 512; G2V_ERR_UNSUPPORTED beyond.  Distances are formed once, in g2v_dbscan_neighbors; the other two read
 * the bitmap.  No floating-point atomics: the same input gives the same bits.
 *
 * g2v_dbscan_neighbors: x (N,E) fp32 with row stride ld >= E, ld % 4 == 0, eps >= 0 -> bitmap: N rows of W = ceil(N / 64) 64-bit
 *   words, bit (j % 64) of word j / 64 of row i = adj(i,j), bits past N zero, symmetric bit for bit; counts int64[N] = the popcount of
 *   each row.  d^2 as g2v_tsne_affinities forms it (float64 norms, Gram tiles on the exact-fp32 MFMA in chains of 32 columns folded
 *   in float64); adjacent iff d^2 <= eps * eps in float64.  A pair with |d^2 - eps^2| <= 2^-18 (|x_i|^2 + |x_j|^2), twice the
 *   worst case of the Gram form's error, is evaluated again as sum (x_i - x_j)^2 in float64 and decided on that: every bit is the
 *   float64 decision of the fp32 rows.  Columns E .. ld - 1 are never read.  x and workspace 16-byte aligned, bitmap 8-byte.
 * g2v_dbscan_propagate: `rounds` >= 1 rounds of L'[i] = min(L[i], min {L[j] : adj(i,j), core(j)}) over the core rows, each followed
 *   by pointer jumping L'[i] <- L'[L'[i]].  L, tmp: int32[N].  init != 0 first sets L[i] = i for core rows (counts[i] >= min_samples)
 *   and N for the others; with init == 0 L continues from an earlier call and counts is not read.  flags int32[rounds]: flags[r] = 1
 *   iff round r changed a row.  A round reads one array and writes the other, so neither its result nor the number of rounds
 *   depends on the order of the workgroups, and no round waits on another workgroup.  Call until a flag stays 0 (at most N rounds):
 *   then L[i] = root(i) for core rows.
 * g2v_dbscan_labels: the converged L -> labels int64[N], core uint8[N], out int64[3] = { clusters, core rows, rows labelled -1 }.
 * workspace (neighbors and labels): g2v_dbscan_workspace(N, E) bytes (0 for an unsupported shape), not trusted across calls. */
int64_t g2v_dbscan_max_rows(void);
size_t g2v_dbscan_workspace(int64_t N, int E);
int g2v_dbscan_neighbors(const float* x, int64_t ld, int64_t N, int E, double eps, uint64_t* bitmap, int64_t* counts, void* workspace,
                         size_t workspace_bytes, g2v_stream_t stream);
int g2v_dbscan_propagate(const uint64_t* bitmap, const int64_t* counts, int64_t N, int64_t min_samples, int init, int rounds,
                         int32_t* L, int32_t* tmp, int32_t* flags, g2v_stream_t stream);
int g2v_dbscan_labels(const uint64_t* bitmap, const int32_t* L, int64_t N, int64_t* labels, uint8_t* core, int64_t* out,
                      void* workspace, size_t workspace_bytes, g2v_stream_t stream);

/* ---- Ward agglomerative clustering over latent rows (ward.hip; gesture2vec_amd/agglomerative.py) ------------------------------------
 * The last sklearn branch of the reference's clustering switch (Clustering.py:751-755,
 * AgglomerativeClustering(linkage="ward", n_clusters)), with the merges of scipy.cluster.hierarchy.ward.  Ward linkage is reducible,
 * so clusters that are each other's nearest neighbour may be merged at any time: a round merges all such pairs at once.  A slot is
 * a cluster; slot k starts as row k and a merged pair lives on in its smaller slot.  1 <= N <= g2v_ward_max_rows() = 32768 (the
 * distance matrix is 8 N^2 bytes: 8 GiB at the limit), 1 <= E <= 512; G2V_ERR_UNSUPPORTED beyond, before any launch.  No
 * floating-point atomics: the same input gives the same bits, whatever the order of the workgroups.
 *
 * g2v_ward_distances: x (N,E) fp32 with row stride ld >= E, ld % 4 == 0 -> D: N x N float64, row stride N, D[i][j] = |x_i - x_j| of
 *   the rows widened to float64 (unsquared), +inf on the diagonal, D[i][j] and D[j][i] the same bits (one value, stored twice).
 *   d^2 = |x_i|^2 + |x_j|^2 - 2 x_i.x_j with float64 norms and Gram tiles on the float64 MFMA; a pair with
 *   d^2 < (|x_i|^2 + |x_j|^2) / 8 is evaluated again as sum (x_i - x_j)^2 in float64, so bitwise equal rows are 0 apart.  Columns
 *   E .. ld - 1 are never read.  x and workspace 16-byte aligned, D 8-byte.  workspace: g2v_ward_workspace(N, E) bytes (0 for an
 *   unsupported shape), not trusted across calls.
 * g2v_ward_rounds: `rounds` >= 1 rounds over D, in place.  State: size int32[N] (rows of the slot's cluster, 0 = dead), nn int32[N]
 *   (the cached nearest active slot), part int32[N] (the slot merged with in the last round, or -1); init != 0 starts them (and
 *   zeroes counters) for N clusters of one row, with init == 0 they continue from an earlier call.  One round: (a) nn of every slot
 *   that merged in the last round or whose cached nn did, ties to the smallest index (the others keep their cache, which
 *   reducibility allows); (b) every mutual pair i < j is logged in ascending i behind the earlier rounds': pairs int32[N-1][2] =
 *   (i, j), heights float64[N-1] = D[i][j], sizes int32[N-1] = rows of the union; (c) D[i][k] and D[k][i] of every surviving slot k
 *   become scipy's Ward update sqrt(((n_i+n_k) d_ik^2 + (n_j+n_k) d_jk^2 - n_k d_ij^2) / (n_i+n_j+n_k)) of unsquared distances; where
 *   k itself survives a pair of this round, its columns are merged first, then the rows, by one thread that writes both places.  j
 *   is dead from then on and never read.  counters int64[4] = { merges logged, rounds that merged, merges of the last round, where
 *   its log begins }.  A round with one active cluster changes nothing, so call until counters[0] == N - 1 (at most N - 1 rounds).
 *   The log is in round order, not in height order. */
int64_t g2v_ward_max_rows(void);
size_t g2v_ward_workspace(int64_t N, int E);
int g2v_ward_distances(const float* x, int64_t ld, int64_t N, int E, double* D, void* workspace, size_t workspace_bytes,
                       g2v_stream_t stream);
int g2v_ward_rounds(double* D, int64_t N, int32_t* size, int32_t* nn, int32_t* part, int init, int rounds, int32_t* pairs,
                    double* heights, int32_t* sizes, int64_t* counters, g2v_stream_t stream);

/* ---- Pairwise-distance statistics and temporal-neighbour distances (pair_stats.hip; gesture2vec_amd/repdist.py) --------------------
 * The reference's representation-similarity metric (Clustering.py:410-505, calculate_distances): np.mean(pdist(latents)) stores
 * N (N - 1) / 2 float64 distances.  Here the pairs are reduced as they are formed and none is stored.  1 <= N, M <=
 * g2v_pair_stats_max_rows() = 2^24 (the index width, not memory), 1 <= E <= 512, 0 <= bins <= g2v_pair_stats_max_bins() = 1024 (the
 * edges and a workgroup's counters live in LDS); G2V_ERR_UNSUPPORTED beyond, before any launch.  No floating-point atomics, and how the
 * work is split is a function of (N, M) alone: the same input gives the same bits on any device.
 *
 * g2v_pair_stats: x (N,E) fp32 with row stride ldx >= E, ldx % 4 == 0; y (M,E) with ldy likewise, or y == NULL and M == 0.  Without y
 *   the pairs are the unordered pairs i < j of x (N (N - 1) / 2 of them), with y all N M pairs (i, j).  d = sqrt(d^2) with d^2 as
 *   g2v_ward_distances forms it (float64 norms, Gram tiles on the float64 MFMA, a pair with d^2 < (|a|^2 + |b|^2) / 8 again from
 *   differences, so bitwise equal rows are 0 apart).  All outputs are written by the device:
 *     out    double[4]  = { sum d, sum d^2 (of the d^2 themselves), min d, max d }; without a pair { 0, 0, +inf, -inf }.  A NaN
 *                         distance makes the sums NaN and is passed over by min and max.
 *     counts int64[2]   = { pairs, pairs whose distance is NaN or infinite }
 *     hist   int64[bins], with bins > 0, over edges double[bins + 1] (device memory, ascending: the caller's to ensure), by
 *                         numpy.histogram's rule: bin b holds edges[b] <= d < edges[b + 1], the last bin also d == edges[bins];
 *                         anything else, NaN included, is in no bin.  bins == 0: edges and hist are not read and may be NULL.
 *   One workgroup takes 64 rows of x and g2v_pair_stats_run(N, M) consecutive 64-row tiles of the other set and writes one partial to
 *   its own slot of the workspace; a second launch folds the slots in a fixed order.  x, y and workspace 16-byte aligned, the other
 *   arrays 8-byte.  Columns E .. ld - 1 are never read.  workspace: g2v_pair_stats_workspace(N, M, E, bins) bytes (0 for an unsupported
 *   shape), not trusted across calls.
 * g2v_lag_distances: x (N,E) as above, lags: n_lags <= 8 host integers >= 1, clip_ids int64[N] or NULL -> out double[n_lags][N],
 *   out[l][i] = (|x_{i - lag} - x_i| + |x_{i + lag} - x_i|) / 2, each distance the square root of a float64 sum of squared differences;
 *   NaN where i - lag < 0, i + lag >= N, or (with clip_ids) either neighbour carries another id than row i. */
int64_t g2v_pair_stats_max_rows(void);
int g2v_pair_stats_max_bins(void);
int g2v_pair_stats_run(int64_t N, int64_t M);
size_t g2v_pair_stats_workspace(int64_t N, int64_t M, int E, int bins);
int g2v_pair_stats(const float* x, int64_t ldx, int64_t N, const float* y, int64_t ldy, int64_t M, int E, const double* edges, int bins,
                   double* out, int64_t* counts, int64_t* hist, void* workspace, size_t workspace_bytes, g2v_stream_t stream);
int g2v_lag_distances(const float* x, int64_t ld, int64_t N, int E, G2V_HOST const int32_t* lags, int n_lags, const int64_t* clip_ids,
                      double* out, g2v_stream_t stream);

/* ---- DTW k-means over chunk sequences (dtw.hip; gesture2vec_amd/timeseries.py) ------------------------------------------------------
 * The reference's other clustering space (Clustering.py:629-669, tslearn's TimeSeriesKMeans(metric="dtw")): dynamic time warping
 * between series and centres, and DTW barycentre averaging (DBA).  tslearn is not a dependency and no run of it stands behind this
 * block: the algorithm is stated here, from tslearn's definition, and tested against a float64 restatement (tests/_dtw_ref.py).
 *   Series x: fp32 (N, T, F), contiguous.  Centres / second operands y: float64 (M, S, F), contiguous (fp32 widens exactly).
 *   cost(i, j) = sum_f (a_if - b_jf)^2 from the differences in float64, never from a Gram form: every term is non-negative and
 *     identical series are exactly 0 apart.  The terms are added in ascending f, each fused into the running sum.
 *   acc(i, j) = cost(i, j) + min(acc(i-1, j-1), acc(i-1, j), acc(i, j-1)); acc(0, 0) = cost(0, 0); absent predecessors are +inf.
 *   dtw^2(a, b) = acc(T-1, S-1).
 *   The path is walked back from (T-1, S-1) to (0, 0): from each cell to the smallest of (i-1, j-1), (i-1, j), (i, j-1), on equal
 *     values the first of them in that order, on an edge the only move there is.
 * Supported: 1 <= T, S <= g2v_dtw_max_len() = 64 and 1 <= F <= 512; beyond, G2V_ERR_UNSUPPORTED before any launch.  Everything is
 * float64 (the planted test inputs decide a path cell by as little as 4e-7 relative).  No floating-point atomics: the same input
 * gives the same bits on every call, whatever the number of workgroups or CUs.
 *
 * g2v_dtw_workspace(N, M, T, S, F): bytes for either call below with M centres (0 for an unsupported shape); 16-byte aligned, not
 *   trusted across calls.
 * g2v_dtw_cdist: out double (N, M) = dtw^2(x_n, y_m) when squared != 0, its square root otherwise; may be NULL.  labels int64[N] =
 *   the argmin over m of dtw^2, the lowest index on ties; best double[N] = the minimal dtw^2; NULL together.
 * g2v_dtw_dba_accumulate: over every row n with 0 <= labels[n] < K and live[labels[n]] != 0 (live NULL: every cluster is live), with
 *   k = labels[n], the centre c_k as the first index i and the row as the second index j, over every cell (i, j) of the row's path:
 *   sums[k][i][:] += x[n][j][:] (float64 (K, S, F)), counts[k][i] += 1 (int64 (K, S)), cost[k] += dtw^2 (double[K]).  The outputs of a
 *   live cluster are overwritten, not added to (zeros for one without rows); rows with other ids are ignored; a cluster that is
 *   not live is left untouched.  The rows of a cluster are added in ascending n, in slabs of a fixed number of rows that are folded
 *   in slab order.
 * g2v_dtw_dba_update: one barycentre step per live cluster.  state = double prev_cost[K] followed by uint8 live[K] (start: +inf and
 *   1); members int64[K] = the rows of each cluster.  For a live k: centers[k][i][:] = sums[k][i][:] / counts[k][i] (every
 *   counts[k][i] of a cluster with rows is >= 1: a path visits every i); then, with c = cost[k] / members[k], the cluster stops
 *   (live = 0) if |prev - c| < tol or prev < c, otherwise prev = c.  The update is applied before the test.  A live cluster
 *   without rows keeps its centre and stops.  A cluster that is not live is a no-op in both calls, so every step of a barycentre
 *   can be enqueued without reading back: the same bits as checking after each. */
int g2v_dtw_max_len(void);
size_t g2v_dtw_workspace(int64_t N, int64_t M, int T, int S, int F);
int g2v_dtw_cdist(const float* x, int64_t N, int T, const double* y, int64_t M, int S, int F, int squared, double* out, int64_t* labels,
                  double* best, void* workspace, size_t workspace_bytes, g2v_stream_t stream);
int g2v_dtw_dba_accumulate(const float* x, int64_t N, int T, const int64_t* labels, const double* centers, int K, int S, int F,
                           const uint8_t* live, double* sums, int64_t* counts, double* cost, void* workspace, size_t workspace_bytes,
                           g2v_stream_t stream);
int g2v_dtw_dba_update(const double* sums, const int64_t* counts, const double* cost, const int64_t* members, void* state,
                       double* centers, int K, int S, int F, double tol, g2v_stream_t stream);

/* ---- Soft-DTW over chunk sequences (softdtw.hip; gesture2vec_amd/timeseries.py) ------------------------------------------------------
 * The reference's third time-series branch (Clustering.py:670-691, tslearn's TimeSeriesKMeans(metric="softdtw")): the differentiable
 * DTW of Cuturi & Blondel (2017), its soft alignment matrix, and value and gradient of a barycentre objective.  tslearn is not a
 * dependency and no run of it stands behind this block: the algorithm is stated here, from tslearn's definition, and tested against
 * a float64 restatement (tests/_softdtw_ref.py).  Everything is float64.
 *   Operands.  Series x: fp32 (N, T, F), contiguous.  A centre or second operand z: float64 (S, F), contiguous.  gamma > 0.
 *   Cost.  cost(i, j) = sum_f (z_if - x_jf)^2, formed exactly as the DTW block forms it (from differences, f ascending, each term
 *     fused into the running sum; one piece of code, csrc/dtw_tile.hpp).  Not tslearn's Gram form: the two differ by rounding only.
 *   Forward.  R(i, j) = cost(i, j) + softmin(R(i-1, j), R(i-1, j-1), R(i, j-1)); R(0, 0) = cost(0, 0); absent predecessors contribute
 *     nothing.  softmin(a, b, c) = -gamma (log(e^(a'-m) + e^(b'-m) + e^(c'-m)) + m), a' = -a / gamma and so on, m = max(a', b', c').
 *     sdtw(z, x) = R(S-1, T-1).  It can be negative.
 *   Backward.  E(S-1, T-1) = 1, otherwise E(i, j) = E(i+1, j) a + E(i, j+1) b + E(i+1, j+1) c with
 *     a = exp((R(i+1, j) - R(i, j) - cost(i+1, j)) / gamma), b = exp((R(i, j+1) - R(i, j) - cost(i, j+1)) / gamma),
 *     c = exp((R(i+1, j+1) - R(i, j) - cost(i+1, j+1)) / gamma); a term whose successor lies outside the tile is 0.  Each of a, b, c
 *     lies in (0, 1], and so does E (up to rounding).  E is tslearn's soft_dtw_alignment.
 *   Objective of a barycentre z over member rows with weights w_n (all ones when absent, not normalised):
 *     obj(z) = sum_n w_n sdtw(z, x_n),  G[i][f] = 2 (z_if sum_n w_n sum_j E_n(i, j) - sum_n w_n sum_j E_n(i, j) x_njf).
 *   softdtw_barycenter(X, gamma, weights, max_iter, tol = 1e-3, init) = scipy.optimize.minimize(f, init.ravel(), method="L-BFGS-B",
 *     jac=True, tol=tol, options=dict(maxiter=max_iter, disp=False)).x on the host, f = (obj, G) from the device; init = None starts
 *     from the weighted Euclidean mean (equal lengths only); max_iter == 0 returns the init.
 *   k-means loop (tslearn's TimeSeriesKMeans(metric="softdtw")).  Centres start as the init rows.  For it in range(max_iter):
 *     labels = argmin_k sdtw(c_k, x_n), lowest index on ties; inertia = the mean of the minimal soft-DTW values (not squared, not the
 *     DTW inertia); an empty cluster raises, or redraws with init="random"; every cluster becomes softdtw_barycenter(members, gamma,
 *     max_iter=max_iter_barycenter, init=its current centre); stop after the update if |old - inertia| < tol.  labels_ and inertia_
 *     are those of the last assignment; predict uses the final centres.
 * Supported: the DTW limits, 1 <= T, S <= g2v_dtw_max_len() and 1 <= F <= 512; beyond, G2V_ERR_UNSUPPORTED before any launch.  gamma
 * that is not finite or not > 0: G2V_ERR_ARG.  exp of a very negative argument underflows to 0; no NaN arises from finite inputs.
 * No floating-point atomics, independent workgroups only: the same input gives the same bits on every call.
 *
 * g2v_softdtw_workspace(N, M, T, S, F): bytes for any call below over N rows (for g2v_softdtw_grad: R member rows) and M centres (1
 *   for g2v_softdtw_grad); 0 for an unsupported shape; 16-byte aligned, not trusted across calls.
 * g2v_softdtw_cdist: out double (N, M) = sdtw(y_m, x_n); may be NULL.  labels int64[N] = the argmin over m, the lowest index on
 *   ties; best double[N] = the minimal value; NULL together.
 * g2v_softdtw_alignment: every row of x (R, T, F) against the one centre z -> value double[R] = sdtw(z, x_r), E double (R, S, T).
 * g2v_softdtw_grad: one evaluation of (obj, G) for the centre z over the member rows x[rows[r]], r < R: rows int64[R] on the device,
 *   ascending row ids in [0, N) (an id outside contributes nothing); weights double[R] on the device, or NULL for all ones ->
 *   value double[1], grad double (S, F).  Per (i, f) the members' sums over j (j ascending) are added in the order of `rows`, in
 *   slabs of a fixed number of members that are folded in slab order: the order of every sum is a function of `rows` alone. */
size_t g2v_softdtw_workspace(int64_t N, int64_t M, int T, int S, int F);
int g2v_softdtw_cdist(const float* x, int64_t N, int T, const double* y, int64_t M, int S, int F, double gamma, double* out,
                      int64_t* labels, double* best, void* workspace, size_t workspace_bytes, g2v_stream_t stream);
int g2v_softdtw_alignment(const float* x, int64_t R, int T, const double* z, int S, int F, double gamma, double* value, double* E,
                          g2v_stream_t stream);
int g2v_softdtw_grad(const float* x, int64_t N, int T, const int64_t* rows, int64_t R, const double* weights, const double* z, int S,
                     int F, double gamma, double* value, double* grad, void* workspace, size_t workspace_bytes, g2v_stream_t stream);

/* ---- The frame-level quantised autoencoder of Part a (VQ_Frame, reference scripts/model/DAE_model.py:118-275, :351-482):
 *   x (B,D) -> Dropout -> y = x We^T + be -> z = BatchNorm1d(y) -> id = argmin_k (|z|^2 + |e_k|^2) - 2 z.e_k (lowest k on ties),
 *   q = e_id -> out = q Wd^T + bd;  loss = mse(out, target) + commitment mse(q.detach(), z);  the quantiser's state moves by the EMA
 *   of the batch's code statistics (counts, Laplace smoothing, dw = onehot^T z), never by a gradient.  No pre_linear is applied.
 * g2v_vqframe_plan(B, D, L, K, training): host arithmetic only.  Bits 0-7: what `auto` takes, G2V_VQFRAME_FUSED (training: the
 *   one-workgroup step g2v_vqframe_step; eval, B = rows: the grid kernel g2v_vqframe_infer), G2V_VQFRAME_STAGED (the per-operator
 *   kernels: linear, batchnorm, vq_assign ...), or G2V_VQFRAME_REFUSED (0: no route, e.g. B < 2 in training).  G2V_VQFRAME_FUSED_OK
 *   is set where the fused kernel admits the shape whatever `auto` takes: training 2 <= B, L <= 256, K <= 256 and the LDS layout
 *   (vq_frame.hip) within 160 KB -- B <= 256 at D = 135, L <= 45, K <= 128 --; eval D, L <= 256, K <= 4096.  `auto` is FUSED only
 *   where it was measured faster.  g2v_vqframe_plan_reason: the same answer in words (a static string).
 * g2v_vqframe_workspace: bytes of workspace for the fused kernel of that mode (0: not admitted); g2v_vqframe_step_lds: the
 *   step's dynamic LDS in bytes (0: not admitted).
 * g2v_vqframe_step: training forward and backward of one batch in ONE workgroup.  keep: uint8 (B,D) or NULL (no dropout), kept
 *   inputs are multiplied by scale.  In place: running_mean / running_var (momentum; unbiased variance), codebook, ema_w (K,L) and
 *   ema_cluster_size (K), updated AFTER q was taken from the old codebook.  Writes the six gradients (no dx), scalars[3] = (mse,
 *   loss_vq, perplexity), ids int64[B], and, where not NULL, latent = z (B,L) and out (B,D).  No atomics: the same input gives the
 *   same bits.  G2V_ERR_UNSUPPORTED for a shape the plan does not admit.
 * g2v_vqframe_infer: the eval-mode forward of N rows (running statistics, no dropout) over independent tiles of 16 rows: ids
 *   int64[N], and, where not NULL, latent (N,L) and out (N,D) (then w_dec, b_dec).  A row's bits do not depend on the other rows. */
#define G2V_VQFRAME_REFUSED 0
#define G2V_VQFRAME_FUSED 1
#define G2V_VQFRAME_STAGED 2
#define G2V_VQFRAME_FUSED_OK 256
int g2v_vqframe_plan(int B, int D, int L, int K, int training);
const char* g2v_vqframe_plan_reason(int B, int D, int L, int K, int training);
size_t g2v_vqframe_workspace(int B, int D, int L, int K, int training);
size_t g2v_vqframe_step_lds(int B, int D, int L, int K);
int g2v_vqframe_step(const float* x, const float* target, const uint8_t* keep, float scale, const float* w_enc,
                     const float* b_enc, const float* bn_weight, const float* bn_bias, float* running_mean,
                     float* running_var, float momentum, const float* w_dec, const float* b_dec, float* codebook,
                     float* ema_w, float* ema_cluster_size, float commitment, double decay, double epsilon,
                     float* g_w_enc, float* g_b_enc, float* g_bn_weight, float* g_bn_bias, float* g_w_dec, float* g_b_dec,
                     float* scalars, int64_t* ids, float* latent, float* out, void* workspace, size_t workspace_bytes,
                     int B, int D, int L, int K, g2v_stream_t stream);
int g2v_vqframe_infer(const float* x, int64_t N, const float* w_enc, const float* b_enc, const float* bn_weight,
                      const float* bn_bias, const float* running_mean, const float* running_var, const float* codebook,
                      const float* w_dec, const float* b_dec, int64_t* ids, float* latent, float* out, void* workspace,
                      size_t workspace_bytes, int D, int L, int K, g2v_stream_t stream);

/* ---- The frame-level variational autoencoder of Part a (VAE_Network, reference scripts/model/DAE_model.py:600-725;
 * train_eval/train_seq2seq.py:161-241), autoencoder_vq "False" with autoencoder_vae "True":
 *   x (B,D) -> Dropout -> h = tanh(x We^T + be) -> mean = h Wm^T + bm, logvar = h Ws^T + bs -> z = mean + exp(logvar / 2) eps
 *   -> c = z Wf^T + bf -> out = c Wd^T + bd;  loss = mse(out, target) + kl_weight kl,  kl = mean(exp(logvar) - logvar - 1 + mean^2)
 *   over the B L elements (the reference's 5 x -2.5 mean(mean(1 + logvar - exp(logvar) - mean^2, 1)) is kl_weight = 12.5).
 * Noise, here and in g2v_reparam_fwd: eps_in (B,L) when given, else drawn from the g2v_keep_mask stream exactly as
 *   g2v_vae_latent_fwd draws it (seed, offset_counter[0]; Philox block g <-> elements 4g .. 4g+3 of the row-major (B,L) array, two
 *   Box-Muller pairs per block; one device function serves all three kernels); the counter then advances by 1 and eps_out (B,L)
 *   receives the eps used (required when drawn, else may be NULL).
 * g2v_vaeframe_plan(B, D, L, training): host arithmetic only, with the constants and bit layout of g2v_vqframe_plan
 *   (G2V_VQFRAME_FUSED / _STAGED / _REFUSED in bits 0-7, G2V_VQFRAME_FUSED_OK).  The fused step is admitted for training,
 *   2 <= B, where its LDS layout (vae_frame.hip: six (B, ld(L)) row arrays + 32 floats) stays within 160 KB -- B <= 155 at L = 40,
 *   B <= 131 at L = 45, whatever D is.  B = 1 is refused (the reference's squeeze drops the row axis of a single frame).  Eval
 *   mode has no fused kernel: STAGED.  `auto` is FUSED only where it was measured faster: admitted shapes with B <= 155,
 *   D <= 135, L <= 45.
 *   g2v_vaeframe_plan_reason: the same answer in words (a static string).  g2v_vaeframe_workspace: bytes of workspace of the
 *   fused step (0: not admitted); g2v_vaeframe_step_lds: its dynamic LDS in bytes (0: not admitted).
 * g2v_vaeframe_step: training forward and backward of one batch in ONE workgroup.  keep: uint8 (B,D) or NULL (no dropout), kept
 *   inputs are multiplied by scale.  Writes the ten gradients (no dx), scalars[3] = (mse, kl, mse + kl_weight kl), and, where not
 *   NULL, latent = h, mean, logvar (B,L) and out (B,D).  It moves no weight.  Every product is a chain of fp32 MFMAs per 16 x 16
 *   tile with k ascending, every other sum has a fixed tree, no atomics: the same input gives the same bits.
 *   G2V_ERR_UNSUPPORTED for a shape the plan does not admit.
 * The staged route's operators (the dense layers are g2v_linear_*), any n >= 1 elements:
 *   g2v_tanh_bwd     dpre[i] = dy[i] (1 - y[i]^2), y = tanh(pre).
 *   g2v_reparam_fwd  z = mean + exp(logvar / 2) eps (sample != 0; noise as above) or z = mean bit for bit (sample == 0: eps is
 *                    neither read nor written); kl[0] = mean(exp(logvar) - logvar - 1 + mean^2) by per-workgroup partials in a
 *                    fixed order and a one-workgroup finish.  workspace >= g2v_reparam_workspace(n) bytes.
 *   g2v_reparam_bwd  c = g_kl[0] / n (g_kl: device scalar d loss / d kl, NULL = 0);  dmean = dz + 2 c mean + g_mean,
 *                    dlogvar = dz 0.5 exp(logvar / 2) eps + c (exp(logvar) - 1) + g_logvar.  eps NULL: the forward had sample == 0.
 *                    dz, g_mean, g_logvar (n; NULL = 0): the gradients reaching z, mean and logvar. */
int g2v_vaeframe_plan(int B, int D, int L, int training);
const char* g2v_vaeframe_plan_reason(int B, int D, int L, int training);
size_t g2v_vaeframe_workspace(int B, int D, int L);
size_t g2v_vaeframe_step_lds(int B, int D, int L);
int g2v_vaeframe_step(const float* x, const float* target, const uint8_t* keep, float scale, const float* w_enc,
                      const float* b_enc, const float* w_mean, const float* b_mean, const float* w_std, const float* b_std,
                      const float* w_fc, const float* b_fc, const float* w_dec, const float* b_dec, float kl_weight,
                      const float* eps_in, uint64_t seed, int64_t* offset_counter, float* g_w_enc, float* g_b_enc, float* g_w_mean,
                      float* g_b_mean, float* g_w_std, float* g_b_std, float* g_w_fc, float* g_b_fc, float* g_w_dec, float* g_b_dec,
                      float* scalars, float* latent, float* mean, float* logvar, float* out, float* eps_out, void* workspace,
                      size_t workspace_bytes, int B, int D, int L, g2v_stream_t stream);
int g2v_tanh_bwd(const float* dy, const float* y, float* dpre, int64_t n, g2v_stream_t stream);
size_t g2v_reparam_workspace(int64_t n);
int g2v_reparam_fwd(const float* mean, const float* logvar, const float* eps_in, uint64_t seed, int64_t* offset_counter, int sample,
                    float* z, float* eps_out, float* kl, void* workspace, size_t workspace_bytes, int64_t n, g2v_stream_t stream);
int g2v_reparam_bwd(const float* dz, const float* g_kl, const float* g_mean, const float* g_logvar, const float* mean,
                    const float* logvar, const float* eps, float* dmean, float* dlogvar, int64_t n, g2v_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* G2V_H */
