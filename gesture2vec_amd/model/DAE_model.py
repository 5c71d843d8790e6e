"""Part a: frame-level denoising autoencoder -- mirror of `scripts/model/DAE_model.py::DAE_Network` (:22-114) on the
MI355X dense-layer kernels.  Dropout(0.2) -> Linear(motion_dim, latent) + ReLU -> Linear(latent, motion_dim).
state_dict keys `encoder.0.*`, `decoder.0.*` as in the reference.  Sentinels: latent_dim == -1 is the identity
(:52-55), latent_dim == -2 is a linear 200-d bottleneck with 30 % dropout (:58-66).

`VQ_Frame` (:118-275) with its own `VQ_Payam_EMA` (:351-482) is the frame-level QUANTISED autoencoder (autoencoder_vq "True"):
Dropout(0.5) -> Linear -> BatchNorm1d (`bachnorm`, the reference's spelling) -> nearest of K codes (EMA codebook) -> Linear.

`VAE_Network` (:600-725) is the frame-level VARIATIONAL autoencoder (autoencoder_vq "False", autoencoder_vae "True"):
Dropout(0.5) -> tanh(Linear) -> mean, logvar -> z = mean + exp(logvar / 2) eps -> Linear -> Linear."""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import functional as Fn
from .. import ops
from .Autoencoder_VQVAE_model import _VQFn


class _FramePlumbing:
    """What the three frame models share besides their layers: the keep mask (given or drawn), the Philox offset counter, the input
    checks and the route resolver.  A plain mixin in front of nn.Module: it adds no child, buffer or parameter, so no state_dict
    moves.  A class names itself in `_name` (error messages), says what `_batch` answers a wrong batch with in `_batch_msg`
    ({} = the shape), and, if it has routes, provides `_plan(rows, training)` and a dict `_routes`."""

    _name = ""
    _batch_msg = ""
    _refuses_when_staged = False      # VAE_Network: a shape the plan refuses raises on every route, "staged" included
    _explicit_keep = None
    _rng_counter = None
    rng_seed = 0

    def set_dropout_mask(self, keep):
        """Explicit uint8 keep mask for the next training forwards (parity tests)."""
        self._explicit_keep = keep

    def _counter(self, device):
        if self._rng_counter is None or self._rng_counter.device != device:
            self._rng_counter = torch.zeros(1, dtype=torch.int64, device=device)
        return self._rng_counter

    def _keep(self, inp: torch.Tensor):
        if self._explicit_keep is not None:
            return self._explicit_keep
        return ops.keep_mask(torch.empty(inp.shape, dtype=torch.uint8, device=inp.device), 1.0 - self.dropout.p, self.rng_seed,
                             self._counter(inp.device))

    def _on_device(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            raise RuntimeError(f"{self._name} runs on the MI355X kernels only (no CPU fallback)")
        return x

    def _batch(self, x: torch.Tensor) -> torch.Tensor:
        """(B,D,1) or (B,D) -> contiguous (B,D) with B >= 2"""
        inp = torch.squeeze(x)
        if inp.dim() != 2 or inp.shape[0] < 2:
            raise ValueError(self._batch_msg.format(tuple(x.shape)))
        return self._on_device(inp).contiguous()

    def _rows(self, x: torch.Tensor, width: int) -> torch.Tensor:
        return self._on_device(x).reshape(-1, width).contiguous()

    def resolve(self, rows: int, training: bool) -> str:
        """"fused" or "staged" for a call of `rows` frames; `auto` takes the plan's answer.  An explicit "fused" that the kernel does
        not admit raises with the plan's reason."""
        if self.route not in ("auto", "fused", "staged"):
            raise ValueError(f"{self._name}.route must be 'auto', 'fused' or 'staged', got {self.route!r}")
        if self.route == "staged" and not self._refuses_when_staged:
            return "staged"
        key = (rows, training)
        if key not in self._routes:
            self._routes[key] = self._plan(rows, training)
        auto, fused_ok, reason = self._routes[key]
        if auto == "" and (self._refuses_when_staged or self.route == "auto"):
            raise ValueError(f"{self._name}: {reason}")
        if self.route == "fused" and not fused_ok:
            raise ValueError(f"{self._name}.route = 'fused': {reason}")
        return auto if self.route == "auto" else self.route


class DAE_Network(_FramePlumbing, nn.Module):
    _name = "DAE_Network"

    def __init__(self, motion_dim: int, latent_dim: int):
        super().__init__()
        self.dropout = nn.Dropout(0.2)             # container for p only; masks come from the Philox kernel
        self._relu = True
        if latent_dim == -1:
            self.encoder = None
            self.decoder = None
            return
        if latent_dim == -2:
            self.encoder = nn.Sequential(nn.Linear(motion_dim, 200))
            self.decoder = nn.Sequential(nn.Linear(200, motion_dim))
            self.dropout = nn.Dropout(0.3)
            self._relu = False
            return
        self.encoder = nn.Sequential(nn.Linear(motion_dim, latent_dim), nn.ReLU())
        self.decoder = nn.Sequential(nn.Linear(latent_dim, motion_dim))

    def encode(self, x: torch.Tensor) -> torch.Tensor:
        """`rep_model.encoder(x)` as the datasets call it (lmdb_data_loader.py:649-653): Linear(+ReLU), no dropout."""
        e = self.encoder[0]
        return Fn.linear(x, e.weight, e.bias, act=1 if self._relu else 0)

    def decode(self, lat: torch.Tensor) -> torch.Tensor:
        d = self.decoder[0]
        return Fn.linear(lat, d.weight, d.bias)

    def forward(self, x: torch.Tensor, get_latent: bool = False):
        if self.encoder is None:
            return (x, x) if get_latent else x
        inp = self._on_device(torch.squeeze(x))
        keep, scale = None, 1.0
        if self.training:
            keep, scale = self._keep(inp), 1.0 / (1.0 - self.dropout.p)
        e = self.encoder[0]
        lat = Fn.linear(inp, e.weight, e.bias, keep=keep, scale=scale, act=1 if self._relu else 0)
        out = self.decode(lat)
        out = torch.unsqueeze(out, 2)
        return (out, lat.detach().clone()) if get_latent else out


class VQ_Payam_EMA(nn.Module):
    """The frame-level EMA quantiser (reference DAE_model.py:351-482).  It is not Part b's class: the codebook starts
    uniform(-1/K, 1/K), and `pre_linear` is part of the state_dict but NOT applied -- distances, loss and straight-through all act
    on the input rows.  forward(inputs) -> (loss, quantized, perplexity, encodings).  `_ema_w`, `_embedding.weight` and
    `pre_linear.*` never receive a gradient (the reference re-creates the first two every training forward, so its optimiser never
    moves them either); here they are updated in place by the kernels."""

    def __init__(self, num_embeddings: int, embedding_dim: int, commitment_cost: float, decay: float, epsilon: float = 1e-5):
        super().__init__()
        self._embedding_dim, self._num_embeddings = embedding_dim, num_embeddings
        self.pre_linear = nn.Linear(embedding_dim, embedding_dim)
        self._embedding = nn.Embedding(num_embeddings, embedding_dim)
        self._embedding.weight.data.uniform_(-1 / num_embeddings, 1 / num_embeddings)      # :383-385
        self._commitment_cost = commitment_cost
        self.register_buffer("_ema_cluster_size", torch.zeros(num_embeddings))
        self._ema_w = nn.Parameter(torch.Tensor(num_embeddings, embedding_dim))
        self._ema_w.data.normal_()
        self._decay, self._epsilon = decay, epsilon
        # 1 - decay as torch forms the Python scalar (in double): a cluster size that starts from ZERO is (1 - decay) count after the
        # first update, so the 9.3e-7 between that and 1.0f - 0.99f reaches the second step's codebook and loss undiluted
        self._exact_decay = True
        for p in (self._ema_w, self._embedding.weight, self.pre_linear.weight, self.pre_linear.bias):
            p.requires_grad_(False)

    def forward(self, inputs: torch.Tensor):
        return _VQFn.apply(inputs, self, False)


class VQ_Frame(_FramePlumbing, nn.Module):
    """forward(x) -> (out (B,D,1), loss_vq, perplexity); forward(x, Inference=True) -> (out, latent, encodings (N,K) one-hot).

    Two routes behind one forward, chosen by the attribute `route` = "auto" | "fused" | "staged":
      staged  the per-operator kernels under autograd (linear, batchnorm, the quantiser node, linear): every shape, eval mode,
              `skip_vq`; the yardstick of the fused kernel.
      fused   training: g2v_vqframe_step, forward AND backward of the batch in one launch.  The backward needs the target, so the
              launch is driven by `fused_step` (train_iter_DAE calls it); a training `forward` on route "fused" says so.
              eval: g2v_vqframe_infer serves `codes`, `encode` and `forward(x, Inference=True)`.
      auto    asks g2v_vqframe_plan (ops.vqframe_plan) -- here, in `resolve`, and nowhere else."""

    route = "auto"
    _name = "VQ_Frame"
    _batch_msg = ("VQ_Frame in training needs a batch of at least 2 frames (BatchNorm1d on batch statistics; squeeze drops the row "
                  "axis of a single frame), got {}")

    def __init__(self, motion_dim: int, latent_dim: int, vae: bool, vq_components: int):
        super().__init__()
        if vae:
            raise NotImplementedError("VQ_Frame(vae=True) (the frame-level variational block, VAE_fc_mean / VAE_fc_std / "
                                      "VAE_fc_decoder) is out of scope; vae=False is served")
        self.encoder = nn.Sequential(nn.Linear(motion_dim, latent_dim))
        nn.init.xavier_normal_(self.encoder[0].weight)
        self.bachnorm = nn.BatchNorm1d(latent_dim)
        self.skip_vq = False
        self.vq_components = vq_components
        self.commitment_cost = 0.25
        self.vq_layer = VQ_Payam_EMA(self.vq_components, latent_dim, self.commitment_cost, 0.99)
        self.gs_soft = False
        self.decoder = nn.Sequential(nn.Linear(latent_dim, motion_dim))
        nn.init.xavier_normal_(self.decoder[0].weight)
        self.dropout = nn.Dropout()                # p = 0.5; container for p only, masks come from the Philox kernel
        self.vae = vae
        self._pending_batches = 0                  # training forwards not yet added to bachnorm.num_batches_tracked
        self._routes = {}

    # ---- bookkeeping -------------------------------------------------------------------------------------------------------
    def state_dict(self, *args, **kwargs):
        # num_batches_tracked counts training forwards; they are counted on the host and added here, not by a launch per iteration
        if self._pending_batches:
            self.bachnorm.num_batches_tracked += self._pending_batches
            self._pending_batches = 0
        return super().state_dict(*args, **kwargs)

    def _load_from_state_dict(self, *args, **kwargs):
        self._pending_batches = 0
        return super()._load_from_state_dict(*args, **kwargs)

    def _dims(self):
        e = self.encoder[0]
        return e.in_features, e.out_features, self.vq_components

    def _plan(self, rows: int, training: bool):
        return ops.vqframe_plan(rows, *self._dims(), training)

    def _infer_args(self):
        e, bn, q = self.encoder[0], self.bachnorm, self.vq_layer
        return (e.weight.data, e.bias.data, bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var, q._embedding.weight.data)

    # ---- eval-mode entry points ----------------------------------------------------------------------------------------------
    def _encode_staged(self, rows: torch.Tensor) -> torch.Tensor:
        e, bn = self.encoder[0], self.bachnorm
        y = ops.linear_fwd(rows, e.weight.data, e.bias.data)
        return ops.batchnorm_fwd(y, bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var, False, False)[0]

    def encode(self, x: torch.Tensor) -> torch.Tensor:
        """The eval-mode z = bachnorm(encoder(x)) of any number of frames, (N,D) or (N,D,1) -> (N,L): what the datasets would call."""
        rows = self._rows(x, self.encoder[0].in_features)
        if self.resolve(rows.shape[0], False) == "fused":
            return ops.vqframe_infer(rows, *self._infer_args(), want_latent=True)[1]
        return self._encode_staged(rows)

    def codes(self, x: torch.Tensor) -> torch.Tensor:
        """int64 code ids (N,) of any number of frames in eval mode; the (N,K) one-hot is never formed."""
        rows = self._rows(x, self.encoder[0].in_features)
        if self.resolve(rows.shape[0], False) == "fused":
            return ops.vqframe_infer(rows, *self._infer_args())[0]
        z, W = self._encode_staged(rows), self.vq_layer._embedding.weight.data
        return ops.vq_assign(z, z, W, ops.vq_code_sqnorm(W))[0]

    # ---- the fused training step ---------------------------------------------------------------------------------------------
    def trainable(self):
        e, bn, d = self.encoder[0], self.bachnorm, self.decoder[0]
        return [e.weight, e.bias, bn.weight, bn.bias, d.weight, d.bias]

    def fused_step(self, x: torch.Tensor, target: torch.Tensor, grads, want_latent: bool = False, want_out: bool = False):
        """One launch: forward and backward of the batch (g2v_vqframe_step).  `grads`: six buffers for the gradients of
        `trainable()`.  The running statistics and the quantiser's state are updated in place.
        -> (scalars (3,) = reconstruction mse, loss_vq, perplexity; ids (B,); latent or None; out (B,D) or None)"""
        if not self.training or self.skip_vq:
            raise RuntimeError("VQ_Frame.fused_step is the training step with the quantiser on")
        inp = self._batch(x)
        tgt = torch.squeeze(target).contiguous()
        e, bn, d, q = self.encoder[0], self.bachnorm, self.decoder[0], self.vq_layer
        momentum = 0.1 if bn.momentum is None else bn.momentum
        keep = self._keep(inp)
        res = ops.vqframe_step(inp, tgt, keep, 1.0 / (1.0 - self.dropout.p), e.weight.data, e.bias.data, bn.weight.data,
                               bn.bias.data, bn.running_mean, bn.running_var, momentum, d.weight.data, d.bias.data,
                               q._embedding.weight.data, q._ema_w.data, q._ema_cluster_size, q._commitment_cost, q._decay,
                               q._epsilon, grads, want_latent=want_latent, want_out=want_out)
        self._pending_batches += 1
        return res

    # ---- forward -------------------------------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, Inference: bool = False):
        if self.training:
            inp = self._batch(x)
            if self.route == "fused" and not self.skip_vq:
                raise RuntimeError("VQ_Frame.route = 'fused': the fused training step computes forward and backward in one launch and "
                                   "needs the target; call fused_step(x, target, grads) or train_iter_DAE, or set route = 'staged'")
            keep, scale = self._keep(inp), 1.0 / (1.0 - self.dropout.p)
            self._pending_batches += 1
        else:
            inp = self._on_device(torch.squeeze(x))
            if inp.dim() != 2:
                raise ValueError(f"VQ_Frame.forward expects (B, motion_dim, 1) frames with B >= 2, got {tuple(x.shape)}; "
                                 "codes(x) / encode(x) take any number of frames")
            inp = inp.contiguous()
            keep, scale = None, 1.0
            if Inference and not self.skip_vq and self.resolve(inp.shape[0], False) == "fused":
                d = self.decoder[0]
                ids, latent, out = ops.vqframe_infer(inp, *self._infer_args(), w_dec=d.weight.data, b_dec=d.bias.data,
                                                     want_latent=True, want_out=True)
                encodings = torch.zeros((inp.shape[0], self.vq_components), dtype=torch.float32, device=inp.device)
                encodings.scatter_(1, ids.unsqueeze(1), 1.0)       # layout glue: the one-hot the reference's callers argmax over
                return out.unsqueeze(2), latent, encodings
        e, bn, d = self.encoder[0], self.bachnorm, self.decoder[0]
        y = Fn.linear(inp, e.weight, e.bias, keep=keep, scale=scale)
        z = Fn.BatchNormReluFn.apply(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, self.training, False)
        latent = z.detach().clone()
        encodings = None
        if not self.skip_vq:
            loss_vq, z, perplexity_vq, encodings = self.vq_layer(z)
        else:
            loss_vq, perplexity_vq = torch.tensor(0), torch.tensor(0)
        out = torch.unsqueeze(Fn.linear(z, d.weight, d.bias), 2)
        if Inference:
            return out, latent, encodings
        return out, loss_vq, perplexity_vq


class VAE_Network(_FramePlumbing, nn.Module):
    """The frame-level VARIATIONAL autoencoder (reference DAE_model.py:600-725; autoencoder_vq "False", autoencoder_vae "True"):
    Dropout(0.5) -> tanh(Linear(D, L)) = h -> mean = VAE_fc_mean(h), logvar = VAE_fc_std(h) -> z = mean + exp(logvar / 2) eps ->
    VAE_fc_decoder -> Linear(L, D).  forward(x) -> (out (B,D,1), logvar, mean) -- logvar first, as the reference returns them;
    forward(x, get_latent=True) -> (out, latent = h.detach()).  The noise is added in eval mode too (the reference calls
    reparameterize with its default train=True); `reconstruct(x, sample=False)` is the deterministic z = mean path.

    Two routes behind one model, chosen by the attribute `route` = "auto" | "fused" | "staged":
      staged  the per-operator kernels under autograd (five dense layers, tanh, the reparameterisation node): every shape, eval mode.
      fused   training: g2v_vaeframe_step, forward AND backward of the batch in one launch.  The backward needs the target, so the
              launch is driven by `fused_step` (train_iter_DAE calls it); a training `forward` on route "fused" says so.
      auto    asks g2v_vaeframe_plan (ops.vaeframe_plan) -- here, in `resolve`, and nowhere else."""

    route = "auto"
    _name = "VAE_Network"
    _batch_msg = ("VAE_Network needs a batch of at least 2 frames (the reference's squeeze drops the row axis of a single frame and "
                  "its unsqueeze(2) then fails), got {}; encode(x) takes any number of frames")
    _refuses_when_staged = True
    KL_WEIGHT = 12.5            # train_seq2seq.py:224-230: 5 x (-2.5 mean(mean(1 + logvar - exp(logvar) - mean^2, 1)))

    def __init__(self, motion_dim: int, latent_dim: int):
        super().__init__()
        self.encoder = nn.Sequential(nn.Linear(motion_dim, latent_dim), nn.Tanh())
        self.decoder = nn.Sequential(nn.Linear(latent_dim, motion_dim))
        self.dropout = nn.Dropout()                # p = 0.5; container for p only, masks come from the Philox kernel
        self.vae = True
        self.VAE_fc_mean = nn.Linear(latent_dim, latent_dim)
        self.VAE_fc_std = nn.Linear(latent_dim, latent_dim)
        self.VAE_fc_decoder = nn.Linear(latent_dim, latent_dim)
        self._explicit_eps = None
        self._routes = {}
        self.last_kl = None                        # the KL mean of the last staged forward (part of its autograd graph)

    # ---- bookkeeping -------------------------------------------------------------------------------------------------------
    def set_latent_noise(self, eps):
        """Explicit eps (B, L) for the next forwards, training or eval (parity tests); None draws again."""
        self._explicit_eps = eps

    def _dims(self):
        e = self.encoder[0]
        return e.in_features, e.out_features

    def _plan(self, rows: int, training: bool):
        return ops.vaeframe_plan(rows, *self._dims(), training)

    def trainable(self):
        """the ten tensors in state_dict order: what FlatClipAdam(net.parameters()) holds and g2v_vaeframe_step writes gradients for"""
        e, d = self.encoder[0], self.decoder[0]
        return [e.weight, e.bias, d.weight, d.bias, self.VAE_fc_mean.weight, self.VAE_fc_mean.bias, self.VAE_fc_std.weight,
                self.VAE_fc_std.bias, self.VAE_fc_decoder.weight, self.VAE_fc_decoder.bias]

    @staticmethod
    def _kernel_order(ten):
        """trainable() order -> the kernel's (enc, mean, std, fc, dec)"""
        return [ten[0], ten[1], ten[4], ten[5], ten[6], ten[7], ten[8], ten[9], ten[2], ten[3]]

    # ---- the row-wise pieces the datasets and the generators call ----------------------------------------------------------------
    def encode(self, x: torch.Tensor) -> torch.Tensor:
        """h = tanh(Linear(x)) of any number of frames, (N,D) or (N,D,1) -> (N,L), no dropout: `rep_model.encoder(x)`."""
        e = self.encoder[0]
        return ops.linear_fwd(self._rows(x, e.in_features), e.weight.data, e.bias.data, act=2)

    def decode(self, lat: torch.Tensor) -> torch.Tensor:
        """the last Linear on (N,L) rows -> (N,D), as generate.finish_clips uses `dae.decode`"""
        d = self.decoder[0]
        return Fn.linear(lat, d.weight, d.bias)

    def generate(self, z: torch.Tensor) -> torch.Tensor:
        """decoder(VAE_fc_decoder(z)) for latents z (N,L) drawn from the prior -> (N,D)"""
        f = self.VAE_fc_decoder
        return self.decode(Fn.linear(self._rows(z, f.in_features), f.weight, f.bias))

    def reconstruct(self, x: torch.Tensor, sample: bool = True) -> torch.Tensor:
        """the eval-mode forward (no dropout) of (B,D,1) frames -> (B,D,1); sample=False: z = mean, no noise"""
        with torch.no_grad():
            return self._staged(self._batch(x), None, 1.0, sample)[0]

    # ---- the fused training step ---------------------------------------------------------------------------------------------
    def fused_step(self, x: torch.Tensor, target: torch.Tensor, grads, want_latent: bool = False, want_stats: bool = False,
                   want_out: bool = False):
        """One launch: forward and backward of the batch (g2v_vaeframe_step).  `grads`: ten buffers for the gradients of
        `trainable()`, in its order.  -> ops.vaeframe_step's dict: scalars (3,) = mse, kl, mse + 12.5 kl; eps; latent, mean,
        logvar, out where asked for."""
        if not self.training:
            raise RuntimeError("VAE_Network.fused_step is the training step")
        inp = self._batch(x)
        tgt = torch.squeeze(target).contiguous()
        keep = self._keep(inp)
        return ops.vaeframe_step(inp, tgt, keep, 1.0 / (1.0 - self.dropout.p), self._kernel_order([p.data for p in self.trainable()]),
                                 self.KL_WEIGHT, self._kernel_order(list(grads)), eps=self._explicit_eps, seed=self.rng_seed,
                                 offset_counter=self._counter(inp.device), want_latent=want_latent, want_stats=want_stats,
                                 want_out=want_out)

    # ---- forward -------------------------------------------------------------------------------------------------------------
    def _staged(self, inp, keep, scale, sample=True):
        e, d = self.encoder[0], self.decoder[0]
        h = Fn.linear(inp, e.weight, e.bias, keep=keep, scale=scale, act=2)
        mean = Fn.linear(h, self.VAE_fc_mean.weight, self.VAE_fc_mean.bias)
        logvar = Fn.linear(h, self.VAE_fc_std.weight, self.VAE_fc_std.bias)
        z, kl = Fn.reparam(mean, logvar, self._explicit_eps if sample else None, self.rng_seed, self._counter(inp.device), sample)
        c = Fn.linear(z, self.VAE_fc_decoder.weight, self.VAE_fc_decoder.bias)
        out = torch.unsqueeze(Fn.linear(c, d.weight, d.bias), 2)
        return out, logvar, mean, h, kl

    def forward(self, x: torch.Tensor, get_latent: bool = False):
        inp = self._batch(x)
        keep, scale = None, 1.0
        if self.training:
            if self.route == "fused":
                raise RuntimeError("VAE_Network.route = 'fused': the fused training step computes forward and backward in one launch "
                                   "and needs the target; call fused_step(x, target, grads) or train_iter_DAE, or set route = 'staged'")
            keep, scale = self._keep(inp), 1.0 / (1.0 - self.dropout.p)
        out, logvar, mean, h, kl = self._staged(inp, keep, scale)
        self.last_kl = kl
        if get_latent:
            return out, h.detach().clone()
        return out, logvar, mean
