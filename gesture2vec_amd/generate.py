"""Gesture generation on the device: sequences of codes or latent rows -> pose clips.

The reference runs one decode loop at three call sites -- `Clustering.py:198-261` (`make_VQ_Centers`: one gesture per codebook row),
`inference_Autoencoder.py:124-244` with `main`'s tail `:388-404` (a whole clip, chunk after chunk) and
`inference_text2embedding.py:400-547` (the chunk decoder behind Part d's codes).  All three seed the pose decoder's hidden state
per chunk, run five discarded warm-up steps and roll out `n_poses` frames, the last input of one chunk carried in as the first
of the next; then `DAE.decoder`, a blend across the chunk boundaries and the un-normalisation.  Here that loop is `decode_chunks`
(include/g2v.h states the chain above g2v_dec_chain_fwd), behind two routes with the same results up to rounding:

* "chain":   g2v_dec_chain_fwd, the whole chain of every clip in one launch (csrc/dec_chain.hip);
* "rollout": one g2v_dec_rollout_fwd call in eval mode per chunk over warmup + T frames whose first warmup + 1 target frames
             are the carried frame -- the kernels that train the decoder, and the yardstick of the chain kernel's time.  It
             serves every shape g2v_dec_chain_ok refuses.

`AUTO_CHAIN_MIN_CLIPS` decides what route="auto" takes (DESIGN.md section 3.6d has the measured table it is set from).  Everything is
forward-only and runs the net in eval mode (BatchNorm on its running statistics; the decoder's inline Dropout(0.95) stays
active, as in the reference).

`clip_angles` is the arithmetic every make_bvh of the reference runs on such a clip in front of pymo (csrc/clip_angles.hip, DESIGN.md
section 3.6e): `rotmat_to_euler`, the per-frame Rotation.from_matrix(...).as_euler("ZXY", degrees=True), then `smoothing_spline`,
csaps' cubic smoothing spline over every channel.  BVH writing, audio and word timing are out of scope."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .pipeline import _need_cuda, chunk_latents

# route="auto", from the measured table of DESIGN.md section 3.6d (tools/bench_generate.py, profiles/generate_routes.jsonl): the
# fewest clips from which the chain kernel is taken, by whether its weights stay in registers (H = 64, D = 135: it wins or ties at
# every measured batch) or are streamed from L2 every step (every other shape: it wins at B = 4096 only; below that the rollout's
# cluster kernels spread the hidden units of a small batch over many CUs, which one workgroup per 16 clips cannot).  Fewer clips,
# and every shape g2v_dec_chain_ok refuses, take "rollout".
AUTO_CHAIN_MIN_CLIPS = {"resident": 1, "streamed": 4096}
ROUTES = ("auto", "chain", "rollout")
SAVGOL_WINDOW, SAVGOL_ORDER = 25, 5

_DEC_WEIGHTS = {
    "w_pre": "pre_linear.0.weight", "b_pre": "pre_linear.0.bias", "bn_w": "pre_linear.1.weight", "bn_b": "pre_linear.1.bias",
    "bn_running_mean": "pre_linear.1.running_mean", "bn_running_var": "pre_linear.1.running_var",
    "w_ih0": "gru.weight_ih_l0", "w_hh0": "gru.weight_hh_l0", "b_ih0": "gru.bias_ih_l0", "b_hh0": "gru.bias_hh_l0",
    "w_ih1": "gru.weight_ih_l1", "w_hh1": "gru.weight_hh_l1", "b_ih1": "gru.bias_ih_l1", "b_hh1": "gru.bias_hh_l1",
    "w_out": "out_layer.weight", "b_out": "out_layer.bias",
}


def _decoder_weights(net):
    """the pose decoder's tensors by g2v_dec_weights field, after the refusals by name"""
    dec = net.decoder.decoder
    if dec.att_use:
        raise NotImplementedError("decode_chunks: the chain is the attention-free decoder's (autoencoder_att == 'True' has no "
                                  "encoder outputs to attend over when decoding from codes or latents)")
    if dec.n_layers != 2:
        raise NotImplementedError(f"decode_chunks: the decoder kernels are built for n_layers == 2, got {dec.n_layers}")
    sd = dict(dec.named_parameters())
    sd.update(dict(dec.named_buffers()))
    return {k: sd[v].detach().to(torch.float32).contiguous() for k, v in _DEC_WEIGHTS.items()}


class _EvalMode:
    def __init__(self, *nets):
        self.nets = [n for n in nets if n is not None]

    def __enter__(self):
        self.was = [n.training for n in self.nets]
        for n in self.nets:
            n.eval()

    def __exit__(self, *exc):
        for n, was in zip(self.nets, self.was):
            n.train(was)
        return False


def _f32(t, shape, what):
    _need_cuda(t, what)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.to(torch.float32).contiguous()


def check_ids(ids, R):
    """IndexError, as nn.Embedding would raise it, where an id is outside [0, R): one reduction on the ids' device"""
    if ids.numel() > 0 and bool(((ids < 0) | (ids >= R)).any()):
        raise IndexError(f"decode_chunks: an id is outside [0, {R})")


def chain_ok(C_, T, warmup, B, D, H) -> bool:
    return bool(_lib.load().g2v_dec_chain_ok(int(C_), int(T), int(warmup), int(B), int(D), int(H)))


def dec_chain_fwd(rows, ids, start, teacher, keep95, weights, n_pre, conditioned, C_, T, warmup, B, D, H, want_hidden=False):
    """g2v_dec_chain_fwd on checked tensors -> (out (B, C T, D), h_last (2,B,H) | None)"""
    lib = _lib.load()
    dev = rows.device
    out = torch.empty((B, C_ * T, D), dtype=torch.float32, device=dev)
    h_last = torch.empty((2, B, H), dtype=torch.float32, device=dev) if want_hidden else None
    ws = ops.workspace(lib.g2v_dec_chain_workspace(D, H), dev, "decchain")
    _lib.check(lib.g2v_dec_chain_fwd(ops._p(ops._chk(rows, name="rows")), rows.shape[0], ops._p(ids), ops._p(start), ops._p(teacher),
                                     ops._p(keep95), C.byref(ops.dec_weights_struct(weights)), ops._p(out), ops._p(h_last), int(n_pre),
                                     int(conditioned), C_, T, warmup, B, D, H, ops._p(ws), ws.numel(), ops._stream()),
               "dec_chain_fwd")
    return out, h_last


def _rollout_route(rows, ids, start, teacher, keep95, weights, n_pre, conditioned, C_, T, warmup, B, D, H, want_hidden):
    """The composition: chunk c is one eval-mode rollout over T' = warmup + T frames.  Target frames 0..warmup are the carried
    frame, frames warmup + 1 .. warmup + n_pre - 1 the teacher's 1 .. n_pre - 1, n_pre' = warmup + n_pre; outputs
    warmup + 1 .. warmup + T - 1 are out[c, 1..T-1].  Copies only: every number comes from the rollout's kernels."""
    lib = _lib.load()
    dev = rows.device
    Tp = warmup + T
    if lib.g2v_dec_rollout_route(0, Tp, B, D, H, 0, -1, 0, 0) == 0:
        raise NotImplementedError(f"decode_chunks: no decoder rollout serves T' = {Tp}, B = {B}, D = {D}, H = {H}")
    wstruct = ops.dec_weights_struct(weights)
    nblk = ops.dec_rollout_blocks(B)
    saved = {"y": torch.empty((Tp, B, D), dtype=torch.float32, device=dev), "u": torch.empty((Tp - 1, B, H), dtype=torch.float32, device=dev),
             "h0": torch.empty((Tp, B, H), dtype=torch.float32, device=dev), "h1": torch.empty((Tp, B, H), dtype=torch.float32, device=dev),
             "bn_partial": torch.empty((2, nblk, 2, H), dtype=torch.float32, device=dev)}
    k_none = keep95 if keep95 is not None else torch.zeros((C_, Tp - 1, B, D), dtype=torch.uint8, device=dev)
    out = torch.empty((B, C_, T, D), dtype=torch.float32, device=dev)
    target = torch.zeros((B, Tp, D), dtype=torch.float32, device=dev)
    carry = start if start is not None else torch.zeros((B, D), dtype=torch.float32, device=dev)
    R = rows.shape[0]
    for c in range(C_):
        rc = rows.index_select(0, ids[:, c]) if ids is not None else rows[c:R:C_][:B]
        h_init = rc.reshape(B, 2, H).transpose(0, 1).contiguous()
        target[:, :warmup + 1] = carry.unsqueeze(1)
        if teacher is not None and n_pre > 1:
            target[:, warmup + 1:warmup + n_pre] = teacher[:, c, 1:n_pre]
        ops.dec_rollout_fwd(target, h_init, wstruct, saved, k_none[c], None, 0.0, warmup + n_pre, conditioned, False, Tp, B, D, H)
        out[:, c, 0] = carry
        out[:, c, 1:] = saved["y"][warmup + 1:].transpose(0, 1)
        if not conditioned:
            carry = torch.zeros_like(carry)
        elif teacher is not None and T - 1 < n_pre:
            carry = teacher[:, c, T - 1].contiguous()
        else:
            carry = saved["y"][Tp - 1].clone()
    h_last = torch.stack((saved["h0"][Tp - 1], saved["h1"][Tp - 1])) if want_hidden else None
    return out.view(B, C_ * T, D), h_last


@torch.no_grad()
def decode_chunks(net, rows, ids=None, *, chunks, start=None, teacher=None, warmup=5, keep95=None, route="auto",
                  return_hidden=False):
    """The chain of include/g2v.h (g2v_dec_chain_fwd) for B clips of `chunks` chunks -> (B, chunks * T, D) frames in the chunk
    autoencoder's input space (with return_hidden: also the last hidden state (2, B, H)).

    rows (R, 2H): the initial hidden states, [layer 0 | layer 1]; ids (B, chunks) int64 picks chunk c of clip b, without ids it
    is row b * chunks + c (R = B * chunks).  start (B, D): the first input (None: zeros).  teacher (B, chunks, T, D): with it
    the next input is teacher[b, c, t] while t < net.n_pre_poses.  warmup: discarded steps per chunk.  keep95
    (chunks, warmup + T - 1, B, D) uint8: the masks of the inline Dropout(0.95), one per step; None draws them all in one
    ops.keep_mask call from net.rng_seed.  route: "auto" (AUTO_CHAIN_MIN_CLIPS), "chain" or "rollout".
    Raises: NotImplementedError for an attention net, n_layers != 2 and shapes the chosen route does not serve; IndexError for
    an id outside [0, R), as nn.Embedding would."""
    if route not in ROUTES:
        raise ValueError(f"decode_chunks: route must be one of {ROUTES}, got {route!r}")
    weights = _decoder_weights(net)
    _need_cuda(rows, "decode_chunks")
    C_, W = int(chunks), int(warmup)
    T, D, H = int(net.n_frames), int(net.pose_dim), int(net.hidden_size)
    if C_ < 1 or W < 0 or T < 2:
        raise ValueError(f"decode_chunks: chunks >= 1, warmup >= 0 and n_frames >= 2 (got {C_}, {W}, {T})")
    if rows.dim() != 2 or rows.shape[1] != 2 * H:
        raise ValueError(f"decode_chunks: rows must be (R, {2 * H}), got {tuple(rows.shape)}")
    rows = rows.detach().to(torch.float32).contiguous()
    R = rows.shape[0]
    if ids is not None:
        _need_cuda(ids, "decode_chunks")
        if ids.dim() != 2 or ids.shape[1] != C_ or ids.dtype != torch.int64:
            raise ValueError(f"decode_chunks: ids must be (B, {C_}) int64, got {tuple(ids.shape)} {ids.dtype}")
        ids = ids.contiguous()
        B = ids.shape[0]
        check_ids(ids, R)
    else:
        if R % C_ != 0:
            raise ValueError(f"decode_chunks: without ids, rows holds B * chunks rows; {R} is no multiple of {C_}")
        B = R // C_
    if B < 1:
        raise ValueError("decode_chunks: no clips")
    S = W + T - 1
    start = None if start is None else _f32(start, (B, D), "decode_chunks: start")
    teacher = None if teacher is None else _f32(teacher, (B, C_, T, D), "decode_chunks: teacher")
    conditioned = bool(net.autoencoder_conditioned)
    if keep95 is None:
        keep95 = net._draw((C_, S, B, D), 0.05, rows.device) if conditioned else None
    else:
        _need_cuda(keep95, "decode_chunks")
        if tuple(keep95.shape) != (C_, S, B, D) or keep95.dtype != torch.uint8:
            raise ValueError(f"decode_chunks: keep95 must be {(C_, S, B, D)} uint8, got {tuple(keep95.shape)} {keep95.dtype}")
        keep95 = keep95.contiguous()
    n_pre = max(int(net.n_pre_poses), 1) if teacher is not None else 1
    ok = chain_ok(C_, T, W, B, D, H)
    if route == "auto":
        route = "chain" if ok and B >= AUTO_CHAIN_MIN_CLIPS["resident" if (H, D) == (64, 135) else "streamed"] else "rollout"
    if route == "chain" and not ok:
        raise NotImplementedError(f"decode_chunks: g2v_dec_chain_ok refuses chunks = {C_}, T = {T}, warmup = {W}, B = {B}, D = {D}, "
                                  f"H = {H}; route='rollout' serves it")
    fn = dec_chain_fwd if route == "chain" else _rollout_route
    with _EvalMode(net):
        out, h_last = fn(rows, ids, start, teacher, keep95, weights, n_pre, conditioned, C_, T, W, B, D, H, bool(return_hidden))
    return (out, h_last) if return_hidden else out


def _code_rows(net, kmeans, what):
    if getattr(net, "vq", True) and hasattr(net, "vq_layer"):
        return net.vq_layer._embedding.weight.detach()
    if kmeans is None or getattr(kmeans, "cluster_centers_", None) is None:
        raise ValueError(f"{what}: this autoencoder has no quantiser (autoencoder_vq == 'False') and no fitted k-means model "
                         "was given, so a code names no latent row")
    dev = next(net.parameters()).device
    return torch.from_numpy(np.ascontiguousarray(kmeans.cluster_centers_, dtype=np.float32)).to(dev)


@torch.no_grad()
def decode_codes(net, codes, kmeans=None, **kw):
    """codes (B, C) int64 -> (B, C * T, D).  The rows are the net's codebook (vq_layer._embedding.weight); for a quantiser-free
    net the centres of the fitted `kmeans` (gesture2vec_amd.kmeans.KMeans).  **kw: decode_chunks' keywords."""
    rows = _code_rows(net, kmeans, "decode_codes")
    _need_cuda(codes, "decode_codes")
    if codes.dim() != 2:
        raise ValueError(f"decode_codes: codes must be (B, C), got {tuple(codes.shape)}")
    return decode_chunks(net, rows, codes.to(torch.int64), chunks=codes.shape[1], **kw)


@torch.no_grad()
def decode_latents(net, latents, **kw):
    """latents (B, C, L * H), the rows chunk_latents returns (every mode, the variational one included) -> (B, C * T, D)"""
    _need_cuda(latents, "decode_latents")
    if latents.dim() != 3:
        raise ValueError(f"decode_latents: latents must be (B, C, L * H), got {tuple(latents.shape)}")
    B, C_, E = latents.shape
    return decode_chunks(net, latents.reshape(B * C_, E), None, chunks=C_, **kw)


def savgol_table(window=SAVGOL_WINDOW, order=SAVGOL_ORDER) -> np.ndarray:
    """What g2v_clip_finish filters with, in float64: `window` interior taps, then the (window // 2, window) matrices that give the
    first and the last window // 2 frames from the first / last `window` frames -- scipy.signal.savgol_filter(mode="interp"): the
    least-squares polynomial of that order through the edge window, evaluated at the edge frames.  All of it is rows of the
    projection onto polynomials over the window's positions."""
    half = window // 2
    pos = np.arange(window, dtype=np.float64) - half
    A = np.vander(pos, order + 1, increasing=True)
    P = A @ np.linalg.pinv(A)                                   # (window, window): fitted values from samples
    return np.concatenate([P[half], P[:half].reshape(-1), P[window - half:].reshape(-1)])


def clip_finish(frames, mean=None, std=None, *, n_poses, blend=10, smooth=None):
    """g2v_clip_finish on (B, F, Dr) frames: blend across the chunk boundaries, * clip(std, 0.01) + mean, optional filter"""
    _need_cuda(frames, "clip_finish")
    if smooth not in (None, "savgol"):
        raise ValueError(f"clip_finish: smooth must be None or 'savgol', got {smooth!r}")
    if frames.dim() != 3:
        raise ValueError(f"clip_finish: frames must be (B, F, Dr), got {tuple(frames.shape)}")
    B, F, Dr = frames.shape
    T, n = int(n_poses), int(blend)
    if T < 1 or F % T != 0 or n < 0:
        raise ValueError(f"clip_finish: {F} frames are no whole number of chunks of {T}, or blend < 0")
    if n > 0 and T < 2 * n - 1:
        raise ValueError(f"clip_finish: the blend over {n} frames equals the reference's in-place loop only for n_poses >= {2 * n - 1}, "
                         f"got {T}")
    if smooth and F < SAVGOL_WINDOW:
        raise ValueError(f"clip_finish: the Savitzky-Golay filter needs at least {SAVGOL_WINDOW} frames, got {F}")
    if (mean is None) != (std is None):
        raise ValueError("clip_finish: mean and std come together")
    dev = frames.device
    r = frames.detach().to(torch.float32).contiguous()

    def vec(v):
        t = torch.as_tensor(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float64).reshape(-1), dtype=torch.float32)
        if t.numel() != Dr:
            raise ValueError(f"clip_finish: mean / std must have {Dr} entries, got {t.numel()}")
        return t.to(dev)

    m, s = (vec(mean), vec(std)) if mean is not None else (None, None)
    out = torch.empty_like(r)
    table = tmp = None
    if smooth:
        table = torch.from_numpy(savgol_table().astype(np.float32)).to(dev)
        tmp = torch.empty_like(r)
    lib = _lib.load()
    _lib.check(lib.g2v_clip_finish(ops._p(r), ops._p(out), ops._p(m), ops._p(s), ops._p(table), ops._p(tmp), T, n, B, F, Dr,
                                   ops._stream()), "clip_finish")
    return out


def _is_identity(dae):
    return dae is None or getattr(dae, "decoder", None) is None


@torch.no_grad()
def finish_clips(dae, frames, mean, std, *, n_poses, blend=10, smooth=None):
    """(B, F, D) decoded frames -> DAE.decode -> g2v_clip_finish -> (B, F, D_raw).  dae None or an identity DAE skips the decode;
    mean = std = None skips the un-normalisation; smooth: None or "savgol" (window 25, order 5, along time)."""
    _need_cuda(frames, "finish_clips")
    B, F, D = frames.shape
    if not _is_identity(dae):
        with _EvalMode(dae):
            frames = dae.decode(frames.reshape(B * F, D).to(torch.float32).contiguous()).view(B, F, -1)
    return clip_finish(frames, mean, std, n_poses=n_poses, blend=blend, smooth=smooth)


@torch.no_grad()
def codebook_gestures(net, dae=None, mean=None, std=None, **kw):
    """make_VQ_Centers (Clustering.py:198-261): one gesture per codebook row from a zero first frame -> (K, T, D_raw).
    B = K clips of one chunk; no chunk boundary, so nothing is blended."""
    rows = _code_rows(net, kw.pop("kmeans", None), "codebook_gestures")
    K = rows.shape[0]
    ids = torch.arange(K, dtype=torch.int64, device=rows.device).view(K, 1)
    frames = decode_chunks(net, rows, ids, chunks=1, **kw)
    return finish_clips(dae, frames, mean, std, n_poses=int(net.n_frames), blend=0)


@torch.no_grad()
def reconstruct_clips(dae, net, poses, mean, std, *, blend=10, smooth=None, **kw):
    """inference_Autoencoder.generate_gestures (:124-244) plus main's tail (:388-404) for B clips: poses (B, F, D_raw) raw ->
    normalise -> DAE encoder -> chunks -> encoder -> the mode's latent (the codebook row after `assign`, `latent_code` of a
    variational net, else the plain hidden state) -> the chain with teacher = the encoded chunks, start = encoded frame 0 and
    the net's n_pre_poses -> finish_clips.  Returns (B, C * T, D_raw).

    The chunks start at range(0, F - T, T), as in the reference: with F a multiple of T that DROPS the trailing full chunk
    (F = 3 T gives C = 2), and a remainder shorter than T is dropped too.
    The normalisation (x - mean) / clip(std, 0.01) is the data loader's input preparation and is done with torch."""
    _need_cuda(poses, "reconstruct_clips")
    B, F, Draw = poses.shape
    T = int(net.n_frames)
    starts = range(0, F - T, T)
    C_ = len(starts)
    if C_ < 1:
        raise ValueError(f"reconstruct_clips: {F} frames hold no chunk (range(0, F - T, T) with T = {T} is empty)")
    if getattr(net, "vq", True) and getattr(net, "VAE", False):
        raise NotImplementedError("reconstruct_clips: a net with both a quantiser and a variational block is out of scope")
    dev = poses.device
    x = poses.to(torch.float32)
    if mean is not None:
        m = torch.as_tensor(np.asarray(mean, dtype=np.float32).reshape(-1)).to(dev)
        s = torch.as_tensor(np.clip(np.asarray(std, dtype=np.float32).reshape(-1), 0.01, None)).to(dev)
        x = (x - m) / s
    with _EvalMode(dae, net):
        enc = x if _is_identity(dae) else dae.encode(x.reshape(B * F, Draw).contiguous()).view(B, F, -1)
        chunks = enc[:, :C_ * T].reshape(B, C_, T, -1).contiguous()
        lat = chunk_latents(net, chunks.view(B * C_, T, -1))
        if getattr(net, "vq", True):
            rows, ids = net.vq_layer._embedding.weight.detach(), net.vq_layer.assign(lat).view(B, C_)
        else:
            rows, ids = lat, None
        frames = decode_chunks(net, rows, ids, chunks=C_, start=enc[:, 0].contiguous(), teacher=chunks, **kw)
    return finish_clips(dae, frames, mean, std, n_poses=T, blend=blend, smooth=smooth)


NEAREST = tuple(ops.ROT_METHODS)
SPLINE_SMOOTH = 0.5                  # the reference's smooth_f (smoothing_function("spline", .) of every make_bvh)


def rotmat_to_euler(frames, *, nearest="markley"):
    """(..., 9 J) un-normalised row-major 3x3 matrices, joint-major -> (..., 3 J) joint angles in degrees, per joint (Z, X, Y) with
    R = Rz(Z) Rx(X) Ry(Y): Rotation.from_matrix(frame.reshape(J, 3, 3)).as_euler("ZXY", degrees=True) of the reference's make_bvh
    (inference_Autoencoder.py:584-592) for every frame in one launch (g2v_rotmat_to_euler).  The matrices are not orthogonal and
    scipy's from_matrix is two functions: nearest="markley" is scipy 1.10.1's, the reference's pin (Markley's quaternion from the raw
    entries), nearest="procrustes" scipy 1.15.3's (the nearest rotation first).  They agree on exact rotations only.
    Raises ValueError, as scipy 1.15.3 does, when a matrix has a non-positive determinant, naming how many (one read-back)."""
    _need_cuda(frames, "rotmat_to_euler")
    if nearest not in NEAREST:
        raise ValueError(f"rotmat_to_euler: nearest must be one of {NEAREST}, got {nearest!r}")
    if frames.dim() < 1 or frames.shape[-1] == 0 or frames.shape[-1] % 9 != 0:
        raise ValueError(f"rotmat_to_euler: the last dimension holds 9 entries per joint, got {tuple(frames.shape)}")
    J = frames.shape[-1] // 9
    lead = tuple(frames.shape[:-1])
    flat = frames.detach().to(torch.float32).reshape(-1, 9 * J).contiguous()
    if flat.shape[0] == 0:
        return torch.empty(lead + (3 * J,), dtype=torch.float32, device=frames.device)
    angles, bad = ops.rotmat_to_euler(flat, J, ops.ROT_METHODS[nearest])
    n_bad = int(bad.item())
    if n_bad:
        raise ValueError(f"rotmat_to_euler: {n_bad} of {flat.shape[0] * J} matrices have a non-positive determinant (a zero matrix "
                         "or a reflection): no rotation is nearest to them")
    return angles.view(lead + (3 * J,))


def smoothing_spline(y, smooth=SPLINE_SMOOTH):
    """(B, F, Cn) -> (B, F, Cn): the cubic smoothing spline of every (clip, channel) along time at the frames themselves
    (g2v_smoothing_spline): csaps.csaps(x, channel, x, smooth=smooth) of the reference's smoothing_function("spline", .), one
    factorisation and B Cn solves in two launches.  smooth = 1 returns y, smooth = 0 the least-squares straight line."""
    _need_cuda(y, "smoothing_spline")
    if y.dim() != 3:
        raise ValueError(f"smoothing_spline: y must be (B, F, Cn), got {tuple(y.shape)}")
    p = float(smooth)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"smoothing_spline: smooth must lie in [0, 1], got {smooth!r}")
    B, F, Cn = y.shape
    if B < 1 or F < 2 or Cn < 1:
        raise ValueError(f"smoothing_spline: needs B >= 1, F >= 2 and Cn >= 1, got {tuple(y.shape)}")
    return ops.smoothing_spline(y.detach().to(torch.float32).contiguous(), p)


def clip_angles(frames, *, nearest="markley", spline=SPLINE_SMOOTH):
    """The tail of the reference's make_bvh in front of pymo's inverse_transform: frames (B, F, 9 J), as finish_clips returns them ->
    (B, F, 3 J) joint angles, converted (rotmat_to_euler) and then smoothed along time (smoothing_spline with smooth = spline;
    None: not smoothed).  As in the reference the angles are not unwrapped across +-180 degrees before the spline."""
    _need_cuda(frames, "clip_angles")
    if frames.dim() != 3:
        raise ValueError(f"clip_angles: frames must be (B, F, 9 J), got {tuple(frames.shape)}")
    if spline is not None and not 0.0 <= float(spline) <= 1.0:
        raise ValueError(f"clip_angles: spline must be None or lie in [0, 1], got {spline!r}")
    angles = rotmat_to_euler(frames, nearest=nearest)
    return angles if spline is None else smoothing_spline(angles, spline)


@torch.no_grad()
def text_to_codes(t2e_net, windows):
    """The loop of inference_text2embedding.py:351-374 over sentence windows [(ids (B, Tw), lengths), ...] -> (B, C) codes,
    C = windows * slots per window.  The model runs in eval mode with pre_seq and vid_indices = cheat: the argmax of the last
    n_pre_poses slots of a window is carried into the first n_pre_poses slots of the next pre_seq, and cheat is the window's last
    code (None for the first window).  Discrete mode only (text2_embedding_discrete == "True")."""
    if not getattr(t2e_net, "text2_embedding_discrete", False):
        raise NotImplementedError("text_to_codes: text2_embedding_discrete == 'False' produces latent rows, not codes")
    S = t2e_net.sentence_frame_length // t2e_net.n_frames
    n_pre = int(t2e_net.n_pre_poses)
    pre_seq = cheat = None
    out = []
    with _EvalMode(t2e_net):
        for ids, lengths in windows:
            _need_cuda(ids, "text_to_codes")
            B = ids.shape[0]
            if pre_seq is None:
                pre_seq = torch.zeros((B, S), dtype=torch.int64, device=ids.device)
            logits, _ = t2e_net(ids, lengths, None, pre_seq, None, cheat)
            K = logits.shape[2]
            best = ops.argmax_rows(logits.detach().reshape(B * S, K).contiguous()).view(B, S)
            pre_seq = pre_seq.clone()
            pre_seq[:, :n_pre] = best[:, S - n_pre:]
            cheat = best[:, -1].contiguous()
            out.append(best)
    if not out:
        raise ValueError("text_to_codes: no windows")
    return torch.cat(out, dim=1)
