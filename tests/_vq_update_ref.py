"""Float64 restatement of what happens to the codebook AFTER the code assignment, and the bar of every output.

Numpy float64 only, no device.  The operations (reference: scripts/model/Autoencoder_VQVAE_model.py, cited as the kernels cite it):

    stats            cnt[k] = #{n : idx[n] = k},  dw[k] = sum_{idx[n] = k} flat[n]                   (:1262-1266, :1275)
    ema_step         cs = cs d + w cnt (:1263-1265);  n = sum_k cs;  cs = (cs + eps) / (n + K eps) n (:1268-1273);
                     ema_w = ema_w d + w dw (:1276-1278);  codebook = ema_w / cs (:1280-1282);  |W_k|^2;
                     loss = beta sum(sse) / (N_loss E) (:1285-1289);  perplexity = exp(-sum p log(p + 1e-10)), p = cnt / N_cnt
                     (:1293-1294)
    vq_bwd           gz = g_quantized + g_loss 2 beta / (N E) (z - q), q = W[idx] or the dense quantised rows; either gradient
                     may be absent                                                                  (backward of :1285-1292)
    codebook_grad    gW[k] = g_loss 2 / (N E) (cnt[k] W[k] - dw[k])                                 (backward of :1158-1164)
    code_sqnorm      |W_k|^2
    ste              z + (q - z), evaluated in float32                                              (:1170, :1292, :1431)

d is (float)decay; w, the weight of the new statistics, is the float32 number the entry point really uses (ema_weights):
1.0f - (float)decay for g2v_vq_ema_update, (float)(1.0 - decay) for g2v_vq_ema_update_exact.  beta, eps and 1e-10 are the float32
values the kernels hold, widened.

BARS.  u = 2^-24, gamma(n) = n u / (1 - n u): n roundings in a chain perturb a value by at most gamma(n) of its magnitude, and
gamma(j) + gamma(k) + gamma(j) gamma(k) <= gamma(j + k).  Counts, and everything else integer-valued or copied, are compared
for equality.  Inputs are the float32 arrays the device reads, so a bar covers only the operation's own arithmetic.

  Sums.  A sum of n float32 terms in ANY order is within gamma(n + c) sum|terms| of the exact one (n - 1 additions, each term
  passing through at most n - 1 of them; adding an exact zero -- a one-hot miss, an idle lane -- rounds nothing).  c counts the
  fixed merges a partial passes through on top, read from the kernels:
      C_BLOCK = 2   four per-wave partials merged as (p0 + p1) + (p2 + p3): vq_stats_owner_kernel, vq_ema_scalars_kernel
      C_WAVE  = 6   wave_sum, six xor-shuffle additions: vq_ema_scalars_kernel, vq_ema_rows_kernel, code_sqnorm_kernel
      c_slab(splits) = ceil(splits / 16) + 3 + 2 + 2   slab_reduce_kernel: a thread's longest accumulator takes every 16th slab
                    and the up-to-three left over, (s0 + s1) + (s2 + s3), then the four groups' (r0 + r1) + (r2 + r3)
  The one-hot products 1 x and 0 x of the statistics are exact, so
      bar dw[k, e] = gamma(cnt[k] + c) sum_{idx[n] = k} |flat[n, e]|          c = C_BLOCK (tile owner), c_slab(splits) (slabs)
  and 0 for an empty code.  Shards summed in float32 (data parallelism): one merge more.

  Element-wise chains: one rounding per operation (a contracted fma only removes one).
      cs' = cs d + w cnt             two products, one addition; all terms >= 0:           gamma(2) cs'
      n = sum_k cs'                  K terms, C_WAVE + C_BLOCK merges, on perturbed terms:  gamma(K + 10) n
      cs'' = (cs' + eps) / (n + K eps) n.   As a function of the computed n the result is x n / (n + K eps), whose relative
                                     sensitivity to n is s = K eps / (n + K eps); around it: cs' (2) + eps (1), K eps and the
                                     denominator's sum (2), quotient (1), product (1):     (gamma(7) + s gamma(K + 10) / (1 - gamma(K + 10))) cs''
      ema_w' = ema_w d + w dw        signs mix:                                            gamma(2) (|ema_w d| + |w dw|)
      W = ema_w' / cs''              (bar ema_w' + |ema_w'| (rel cs'' + u)) / cs'' (1 + 2 rel cs'')
      |W_k|^2                        sum_e (2 |W| bar W + bar W^2) + gamma(E + C_WAVE + 1) sum_e (|W| + bar W)^2
      loss                           n_sse terms, C_WAVE + C_BLOCK merges, (float)N (float)E, quotient, beta:
                                                                                           gamma(n_sse + 11) beta sum|sse| / (N E)
      vq_bwd                         c = g_loss (2 beta / (N E)): 4 roundings; z - q: 1; product: 1; sum: 1
                                                                                           gamma(7) |c (z - q)| + gamma(1) |g_quantized|
                                     without g_quantized gamma(6) |c (z - q)|; without g_loss the result is g_quantized (or 0) exactly
      codebook_grad                  c = g_loss (2 / (N E)): 3; cnt W: 1; difference: 1; product: 1
                                                                                           gamma(6) |c| (|cnt W| + |dw|)
      code_sqnorm                    E squares, E - 1 additions, C_WAVE merges:             gamma(E + C_WAVE + 1) sum_e W^2
      ste                            float32 numpy evaluates z + (q - z) with the same two roundings: equality

  Perplexity.  p = cnt / N_cnt (1 rounding), x = p + 1e-10f (1), t = p logf(x) (1), ent = sum_k t (K terms, C_WAVE + C_BLOCK
  merges), perplexity = expf(-ent).  No document available to this project states the ulp error of the ROCm device library's logf
  and expf, so the SECOND rule is used for the two functions: the distance of a float32 numpy restatement from float64 ON THE SAME
  INPUTS, times four.  r_log = max_k |log32(x_k) - log64(x_k)| / (u |log64(x_k)|) over this call's x, r_exp the same of
  exp32(-ent) at this call's ent; the functions are allowed 4 r_log and 4 r_exp roundings.  Then
      d p = u p,  d x = d p + u x,  d l = d x / x + 4 r_log u |log x|,  d t = |l| d p + p d l + u |p l|
      d ent = sum_k d t + gamma(K + C_WAVE + C_BLOCK) sum_k (|t| + d t)
      bar = perplexity (expm1(d ent) + 4 r_exp u (1 + expm1(d ent)))

The propagation formulas are first order in u; what they neglect is of the order of u times a bar.

The float32 restatements (suffix _f32) use the same formulas with every sum taken strictly sequentially, the worst order the
sum bars admit; the host test shows them inside every bar and the planted defects outside."""
import numpy as np

U = 2.0 ** -24
C_BLOCK = 2
C_WAVE = 6
F32 = np.float32
TINY = float(F32(1e-10))


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def c_slab(splits):
    return -(-splits // 16) + 3 + 2 + 2


def ema_weights(decay, exact):
    """(d, w) as float32: what vq_ema_update_launch receives from the two entry points"""
    d = F32(decay)
    w = F32(1.0 - float(decay)) if exact else F32(1.0) - d
    return d, F32(w)


# ---- statistics ------------------------------------------------------------------------------------------------------------------
def _segments(idx, K):
    order = np.argsort(idx, kind="stable")
    cnt = np.bincount(idx, minlength=K).astype(np.int64)
    return order, cnt


def stats(idx, flat, K):
    """(cnt int64 (K,), dw float64 (K, E), sum of |terms| float64 (K, E))"""
    order, cnt = _segments(idx, K)
    f = np.asarray(flat, dtype=np.float64)[order]
    live = np.flatnonzero(cnt)
    starts = (np.cumsum(cnt) - cnt)[live]
    dw = np.zeros((K, f.shape[1]))
    mag = np.zeros_like(dw)
    if live.size:
        dw[live] = np.add.reduceat(f, starts, axis=0)
        mag[live] = np.add.reduceat(np.abs(f), starts, axis=0)
    return cnt, dw, mag


def stats_bar(cnt, mag, c):
    return np.where(cnt > 0, gamma(cnt + c), 0.0)[:, None] * mag


def stats_f32(idx, flat, K):
    """float32, every code's rows added one after the other in row order"""
    dw = np.zeros((K, flat.shape[1]), F32)
    cnt = np.zeros(K, F32)
    for n in range(flat.shape[0]):
        dw[idx[n]] += flat[n]
        cnt[idx[n]] += F32(1)
    return cnt, dw


# ---- EMA step --------------------------------------------------------------------------------------------------------------------
def perplexity(cnt, N_cnt):
    """(value, bar) from the float32 counts"""
    K = cnt.shape[0]
    c64 = np.asarray(cnt, dtype=np.float64)
    p32 = cnt.astype(F32) / F32(N_cnt)
    x32 = p32 + F32(1e-10)
    p = c64 / float(N_cnt)
    x = p + TINY
    l = np.log(x)
    t = p * l
    ent = float(t.sum())
    val = float(np.exp(-ent))
    # the measured error of a float32 log / exp at this call's inputs, in roundings
    lx = np.log(x32.astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(np.log(x32).astype(np.float64) - lx) / (U * np.abs(lx))
    r_log = float(np.nanmax(np.where(lx == 0.0, 0.0, r)))
    e32 = F32(-ent)
    r_exp = abs(float(np.exp(e32)) - float(np.exp(np.float64(e32)))) / (U * float(np.exp(np.float64(e32))))
    dp = U * p
    dx = dp + U * x
    dl = dx / x + 4.0 * r_log * U * np.abs(l)
    dt = np.abs(l) * dp + p * dl + U * np.abs(t)
    dent = float(dt.sum() + gamma(K + C_WAVE + C_BLOCK) * (np.abs(t) + dt).sum())
    bar = val * (np.expm1(dent) + 4.0 * r_exp * U * (1.0 + np.expm1(dent)))
    return val, float(bar)


def loss(sse, N_loss, E, beta):
    b = float(F32(beta))
    s = np.asarray(sse, dtype=np.float64)
    val = b * float(s.sum()) / (float(N_loss) * float(E))
    return val, float(gamma(s.shape[0] + C_WAVE + C_BLOCK + 3) * b * float(np.abs(s).sum()) / (float(N_loss) * float(E)))


def ema_step(cnt, dw, sse, cs, ema_w, N_loss, N_cnt, beta, decay, eps, exact, swap_weights=False, weights=None):
    """out[name] = (float64 value, bar) for cs, ema_w, codebook, wsq, loss, perplexity.  swap_weights / weights plant defects."""
    K, E = dw.shape
    d, w = ema_weights(decay, exact) if weights is None else weights
    d, w = (float(w), float(d)) if swap_weights else (float(d), float(w))
    eps = float(F32(eps))
    cnt, dw, cs, ema_w = (np.asarray(a, dtype=np.float64) for a in (cnt, dw, cs, ema_w))
    cs1 = cs * d + w * cnt
    n = float(cs1.sum())
    keps = float(K) * eps
    s = keps / (n + keps)
    cs2 = (cs1 + eps) / (n + keps) * n
    g_n = float(gamma(K + C_WAVE + C_BLOCK + 2))
    rel_cs = float(gamma(7)) + s * g_n / (1.0 - g_n)
    ew = ema_w * d + w * dw
    bar_ew = gamma(2) * (np.abs(ema_w * d) + np.abs(w * dw))
    W = ew / cs2[:, None]
    bar_W = (bar_ew + np.abs(ew) * (rel_cs + U)) / cs2[:, None] * (1.0 + 2.0 * rel_cs)
    wsq = (W * W).sum(1)
    bar_wsq = (2.0 * np.abs(W) * bar_W + bar_W ** 2).sum(1) + gamma(E + C_WAVE + 1) * ((np.abs(W) + bar_W) ** 2).sum(1)
    return dict(cs=(cs2, rel_cs * cs2), ema_w=(ew, bar_ew), codebook=(W, bar_W), wsq=(wsq, bar_wsq),
                loss=loss(sse, N_loss, E, beta), perplexity=perplexity(np.asarray(cnt, dtype=F32), N_cnt))


def _seq_sum(a):
    """float32 sum of a 1-D array, strictly left to right"""
    a = np.asarray(a, dtype=F32)
    return F32(0) if a.size == 0 else np.cumsum(a, dtype=F32)[-1]


def ema_step_f32(cnt, dw, sse, cs, ema_w, N_loss, N_cnt, beta, decay, eps, exact):
    K, E = dw.shape
    d, w = ema_weights(decay, exact)
    eps, beta = F32(eps), F32(beta)
    cs1 = cs * d + w * cnt
    n = _seq_sum(cs1)
    cs2 = (cs1 + eps) / (n + F32(K) * eps) * n
    ew = ema_w * d + w * dw
    W = ew / cs2[:, None]
    wsq = np.cumsum(W * W, axis=1, dtype=F32)[:, -1]
    p = cnt / F32(N_cnt)
    ent = _seq_sum(p * np.log(p + F32(1e-10)))
    out = dict(cs=cs2, ema_w=ew, codebook=W, wsq=wsq, loss=beta * (_seq_sum(sse) / (F32(N_loss) * F32(E))), perplexity=np.exp(-ent))
    assert all(np.asarray(v).dtype == F32 for v in out.values())
    return out


# ---- vq_bwd, codebook gradient, code norms, straight-through value -------------------------------------------------------------
def vq_bwd(gq, gl, z, q, N, E, beta):
    """gq, gl: arrays or None.  q: the (N, E) quantised rows (W[idx] for the gathered form).  (value, bar)"""
    z64, q64 = np.asarray(z, dtype=np.float64), np.asarray(q, dtype=np.float64)
    if gl is None:
        val = np.zeros_like(z64) if gq is None else np.asarray(gq, dtype=np.float64)
        return val, np.zeros_like(z64)
    c = float(gl[0]) * 2.0 * float(F32(beta)) / (float(N) * float(E))
    cd = c * (z64 - q64)
    if gq is None:
        return cd, gamma(6) * np.abs(cd)
    g64 = np.asarray(gq, dtype=np.float64)
    return g64 + cd, gamma(7) * np.abs(cd) + gamma(1) * np.abs(g64)


def vq_bwd_f32(gq, gl, z, q, N, E, beta):
    if gl is None:
        return np.zeros_like(z) if gq is None else gq.copy()
    c = gl[0] * (F32(2) * F32(beta) / (F32(N) * F32(E)))
    cd = c * (z - q)
    return cd if gq is None else gq + cd


def codebook_grad(cnt, dw, W, gl, N):
    K, E = W.shape
    c = float(gl[0]) * 2.0 / (float(N) * float(E))
    cw = np.asarray(cnt, dtype=np.float64)[:, None] * np.asarray(W, dtype=np.float64)
    d64 = np.asarray(dw, dtype=np.float64)
    return c * (cw - d64), gamma(6) * abs(c) * (np.abs(cw) + np.abs(d64))


def codebook_grad_f32(cnt, dw, W, gl, N):
    K, E = W.shape
    c = gl[0] * (F32(2) / (F32(N) * F32(E)))
    return c * (cnt[:, None] * W - dw)


def code_sqnorm(W):
    w2 = np.asarray(W, dtype=np.float64) ** 2
    return w2.sum(1), gamma(W.shape[1] + C_WAVE + 1) * w2.sum(1)


def code_sqnorm_f32(W):
    return np.cumsum(W * W, axis=1, dtype=F32)[:, -1]


def ste(z, q):
    """float32, bitwise what the reference forms"""
    out = z + (q - z)
    assert out.dtype == F32
    return out


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def fraction(got, ref, bar):
    """largest |got - ref| / bar over the elements whose bar is positive; elements with bar 0 must be equal.  Returns
    (fraction, number of elements outside)."""
    got, ref, bar = (np.asarray(a, dtype=np.float64) for a in (got, ref, bar))
    err = np.abs(got - ref)
    pos = bar > 0
    bad = int((err[~pos] != 0).sum()) + int((err[pos] > bar[pos]).sum()) + int((~np.isfinite(got)).sum())
    frac = float((err[pos] / bar[pos]).max()) if pos.any() else 0.0
    return frac, bad
