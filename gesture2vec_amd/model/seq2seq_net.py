"""The end-to-end text -> pose baseline -- mirror of `scripts/model/seq2seq_net.py` (reference :14-257) on the MI355X kernels:
`EncoderRNN` (word Embedding -> length-packed bi-GRU -> sum of directions), `Attn`, `BahdanauAttnDecoderRNN` (Bahdanau attention
-> cat(pose, context) -> Linear + BatchNorm1d + ReLU -> GRU(2) -> Linear(H -> D)), `Generator`, `Seq2SeqNet` (n_frames - 1 decode
steps; after n_pre_poses frames the decoder's own output is fed back WITH its gradient, :252-255).  Same class names, constructor
signatures and state_dict keys as the reference, so a reference `gen_dict` loads with strict=True and the other way round.

The encoder is Part d's text encoder and the decoder is the continuous, attention-on form of Part d's decoder: both classes ARE
the ones of text2embedding_model.py / Autoencoder_VQVAE_model.py (the decoder under the reference's own constructor signature).

Two routes behind one forward (`Seq2SeqNet.route`):
  per_operator  one autograd node per operator and step: every shape, eval mode, and the yardstick of the tests;
  fused         rollout_t2e.PoseAttnRollout on the step kernels of csrc/pose_attn.hip: the training forward only;
  auto          the library's plan decides (g2v_pose_attn_rollout_plan with rollout_t2e.POSE_FUSED_MIN_ROWS).
Refused by name: `speaker_model`, `discrete_representation=True`, `z is not None`."""
from __future__ import annotations

from types import SimpleNamespace
from typing import List

import torch
import torch.nn as nn

from .. import ops
from .. import rollout_t2e as R
from .Autoencoder_VQVAE_model import Attn
from .text2embedding_model import BahdanauAttnDecoderRNN as _T2EDecoder
from .text2embedding_model import EncoderRNN

__all__ = ["EncoderRNN", "Attn", "BahdanauAttnDecoderRNN", "Generator", "Seq2SeqNet"]


class BahdanauAttnDecoderRNN(_T2EDecoder):
    """Reference :92-190: Part d's decoder in its continuous form with attention always on, under the reference's signature."""

    def __init__(self, input_size: int, hidden_size: int, output_size: int, n_layers: int = 1, dropout_p: float = 0.1,
                 discrete_representation: bool = False, speaker_model=None):
        if speaker_model:
            raise NotImplementedError("speaker_model: the speaker embedding of the baseline is not built")
        if discrete_representation:
            raise NotImplementedError("discrete_representation=True: the baseline regresses poses; code ids belong to Part d "
                                      "(text2embedding_model)")
        super().__init__(SimpleNamespace(autoencoder_att="True"), input_size, hidden_size, output_size, n_layers, dropout_p,
                         False, None)


class Generator(nn.Module):
    def __init__(self, args, motion_dim: int, discrete_representation: bool = False, speaker_model=None):
        super().__init__()
        self.output_size = motion_dim
        self.n_layers = args.n_layers
        self.discrete_representation = discrete_representation
        self.decoder = BahdanauAttnDecoderRNN(input_size=motion_dim, hidden_size=args.hidden_size, output_size=self.output_size,
                                              n_layers=self.n_layers, dropout_p=args.dropout_prob,
                                              discrete_representation=discrete_representation, speaker_model=speaker_model)

    def freeze_attn(self) -> None:
        self.decoder.freeze_attn()

    def forward(self, z, motion_input, last_hidden, encoder_output, vid_indices=None, **kw):
        if z is not None:
            raise NotImplementedError("z is not None: the noise input of the GAN family is not built")
        return self.decoder(motion_input, last_hidden, encoder_output, vid_indices, **kw)


class Seq2SeqNet(nn.Module):
    ROUTES = ("auto", "per_operator", "fused")

    def __init__(self, args, pose_dim: int, n_frames: int, n_words: int, word_embed_size: int, word_embeddings, speaker_model=None):
        super().__init__()
        if speaker_model:
            raise NotImplementedError("speaker_model: the speaker embedding of the baseline is not built")
        self.encoder = EncoderRNN(n_words, word_embed_size, args.hidden_size, args.n_layers, dropout=args.dropout_prob,
                                  pre_trained_embedding=word_embeddings)
        self.decoder = Generator(args, pose_dim, speaker_model=speaker_model)
        self.n_frames, self.n_pre_poses, self.pose_dim = n_frames, args.n_pre_poses, pose_dim
        self.n_layers = args.n_layers
        self.dropout_prob = float(args.dropout_prob)
        self.route = "auto"
        self.last_route = None          # the route the last forward took
        self._masks = None
        self._rng_counter = None
        self.rng_seed = 0
        # Trainers set this to a list for the duration of their forward (train_iter_seq2seq): the decoder then leaves BatchNorm's
        # running statistics alone and `commit_bn_running_stats()` -- called behind the backward -- applies them from the saved
        # batch statistics.  None (a plain forward in train mode): committed step by step, as nn.BatchNorm1d does.
        self.deferred_bn = None

    def commit_bn_running_stats(self) -> None:
        """Apply the decoder BatchNorm's running-statistics updates that the forward passes since `deferred_bn = []` held back
        (the pattern of text2embedding_model.commit_bn_running_stats)."""
        pend, self.deferred_bn = self.deferred_bn, None
        if not pend:
            return
        bn = self.decoder.decoder.pre_linear[1]
        for sm, si, stride, steps, B, H in pend:
            ops.bn_running_update_invstd(sm, si, stride, bn.running_mean, bn.running_var, steps, H, B)

    def set_dropout_masks(self, mask_dec_l0, mask_enc_l0=None):
        """Explicit keep masks for the next training forwards (parity tests): (n_frames-1,B,H) uint8 for the decoder GRU's
        inter-layer dropout, (Tw,B,2H) for the encoder GRU's.  None, None: back to the project's Philox masks."""
        self._masks = None if (mask_dec_l0 is None and mask_enc_l0 is None) else (mask_dec_l0, mask_enc_l0)

    def _draw_many(self, want, dev):
        if self._rng_counter is None or self._rng_counter.device != dev:
            self._rng_counter = torch.zeros(1, dtype=torch.int64, device=dev)
        masks = [ops.keep_mask_at(torch.empty(shape, dtype=torch.uint8, device=dev), kp, self.rng_seed, self._rng_counter, k)
                 for k, (shape, kp) in enumerate(want)]
        ops.counter_add(self._rng_counter, len(want))
        return masks

    def forward(self, in_text, in_lengths, poses, vid_indices):
        """in_text (B,Tw) word ids, in_lengths (B) sorted descending, poses (B, >= n_frames, D) -> outputs (B, n_frames, D) with
        outputs[:, 0] = poses[:, 0] bit for bit."""
        if not in_text.is_cuda:
            raise RuntimeError("Seq2SeqNet runs on the MI355X kernels only (no CPU fallback)")
        if vid_indices is not None:
            raise NotImplementedError("vid_indices feeds the speaker embedding (speaker_model), which is not built")
        if self.route not in self.ROUTES:
            raise ValueError(f"route: one of {self.ROUTES}, got {self.route!r}")
        dev = in_text.device
        ids = in_text.transpose(0, 1).contiguous()                                       # (Tw,B)
        S = self.n_frames
        D, H, L = self.pose_dim, self.encoder.hidden_size, self.n_layers
        if poses.dim() != 3 or poses.shape[1] < S or poses.shape[2] != D:
            raise ValueError(f"poses: expected (B, >= {S}, {D}), got {tuple(poses.shape)}")
        tgt = poses[:, :S].transpose(0, 1).to(torch.float32).contiguous()                # (S,B,D)
        B, Tw = tgt.shape[1], ids.shape[0]
        training = self.training
        dec = self.decoder.decoder
        mask_l0 = mask_enc = None
        if training:
            if self._masks is not None:
                mask_l0, mask_enc = self._masks
            elif self.dropout_prob > 0 and L > 1:
                mask_l0, mask_enc = self._draw_many([((S - 1, B, H), 1.0 - self.dropout_prob),
                                                     ((Tw, B, 2 * H), 1.0 - self.dropout_prob)], dev)
        enc_out, enc_hidden = self.encoder(ids, in_lengths, None, keep_inter=mask_enc)
        enc_proj = dec.attn.project_encoder(enc_out)
        hidden = enc_hidden[:L] if enc_hidden.shape[0] != L else enc_hidden
        bn = dec.pre_linear[1]
        fused = False
        if training and S > 1 and self.route != "per_operator":
            fused = bool(R.pose_plan(B, H, D, Tw, S - 1, L)) if self.route == "auto" else True
        if self.route == "fused" and not (training and S > 1):
            raise RuntimeError("route 'fused' is the training forward only (eval mode and n_frames == 1 go per_operator)")
        if fused:
            if L != 2 or not ops.pose_attn_rollout_ok(S - 1, B, H, D, Tw):
                raise RuntimeError(f"route 'fused': shape not served by g2v_pose_attn_rollout_ok (B={B}, H={H}, D={D}, Tw={Tw}, "
                                   f"n_layers={L})")
            spec = R.RolloutSpec(tgt, S - 1, self.n_pre_poses, L, True, self.dropout_prob, None, mask_l0, bn.running_mean,
                                 bn.running_var, defer_bn=self.deferred_bn)
            full, _ = R.PoseAttnRollout.apply(hidden, enc_out, enc_proj, spec, *R.pose_decoder_params(dec))      # (S,B,D)
            bn.num_batches_tracked += S - 1
        else:
            outs: List[torch.Tensor] = [tgt[0]]
            dec_in = tgt[0]
            for t in range(1, S):
                kl = mask_l0[t - 1].contiguous() if (training and mask_l0 is not None) else None
                y, hidden, _ = self.decoder(None, dec_in, hidden, enc_out, None, keep_l0=kl, enc_proj=enc_proj,
                                            bn_defer=self.deferred_bn if training else None)
                outs.append(y)
                dec_in = tgt[t] if t < self.n_pre_poses else y                           # :252-255: the output, not detached
            full = torch.stack(outs)
        self.last_route = "fused" if fused else "per_operator"
        outputs = full.transpose(0, 1)                                                    # (B,S,D), a view of the step-major array
        return outputs
