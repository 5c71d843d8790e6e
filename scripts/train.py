#!/usr/bin/env python3
"""Trainer of the end-to-end text -> pose baseline (Seq2SeqNet) -- drop-in for the reference's `scripts/train.py` on the MI355X
kernels.

    python train.py --config=../config/baseline_synthetic.yml --synthetic

Same surface: `init_model(args, lang_model, pose_dim, _device)` (lang_model needs `.n_words` and `.word_embedding_weights`) ->
(Seq2SeqNet, MSE loss function), `train_epochs`, `evaluate_testset` (MSE of the eval-mode outputs over all frames, the
`[VAL] loss:` line), `main`; Adam(lr, betas=(0.5, 0.999)), evaluation in front of every epoch, a checkpoint every 20 epochs
(`--save_every N` overrides) with the keys `args, epoch, lang_model, pose_dim, gen_dict`, the `EP ... | ... samples/s | loss:` line.
`--synthetic` feeds batches of the collate function's 5-tuple shape (in_text, text_lengths, target_vec, in_audio, aux_info) made on
the spot: random word ids and lengths (sorted descending), smooth random pose clips of n_poses frames; pose_dim is 135 otherwise.
The real data side (the reference's TwhDataset over its LMDB cache with a fastText vocabulary) is not built: without `--synthetic`
the script says so."""
from __future__ import annotations

import logging
import os
import pprint
import random
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_HERE, _ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from config.parse_args import parse_args  # noqa: E402
from model.seq2seq_net import Seq2SeqNet  # noqa: E402
from train_eval.train_seq2seq import train_iter_seq2seq  # noqa: E402
import utils.train_utils  # noqa: E402
from utils.average_meter import AverageMeter  # noqa: E402
from gesture2vec_amd import ops  # noqa: E402
from gesture2vec_amd.flat import FlatClipAdam  # noqa: E402

device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
POSE_DIM = 135


def _mse(output: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    loss, _ = ops.mse_fwd_bwd(output.contiguous(), target.to(torch.float32).contiguous(), want_grad=False)
    return loss[0]


def init_model(args, lang_model, pose_dim: int, _device):
    generator = Seq2SeqNet(args, pose_dim, args.n_poses, lang_model.n_words, args.wordembed_dim,
                           lang_model.word_embedding_weights).to(_device)
    return generator, _mse


class SyntheticClips:
    """Batches shaped like the reference collate function's 5-tuple; only ids, lengths and poses carry information.  A clip is a
    random walk in pose space, tanh-squashed, so that consecutive frames are close (what custom_loss's continuity term expects)."""

    def __init__(self, args, n_words: int, pose_dim: int, n_batches: int, seed: int, max_len: int = 12):
        self.B, self.T, self.D = args.batch_size, args.n_poses, pose_dim
        self.n_words, self.n_batches, self.seed, self.max_len = n_words, n_batches, seed, max_len

    def __len__(self):
        return self.n_batches

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed)
        for _ in range(self.n_batches):
            lengths = torch.randint(4, self.max_len + 1, (self.B,), generator=g).sort(descending=True).values
            Tw = int(lengths[0])
            ids = torch.zeros(self.B, Tw, dtype=torch.int64)                       # PAD = 0
            for b in range(self.B):
                ids[b, : lengths[b]] = torch.randint(4, self.n_words, (int(lengths[b]),), generator=g)
            start = torch.randn(self.B, 1, self.D, generator=g)
            steps = 0.1 * torch.randn(self.B, self.T, self.D, generator=g)
            poses = torch.tanh(start + steps.cumsum(1))
            yield ids, lengths, poses, torch.zeros(self.B, 1), {}


def evaluate_testset(test_data_loader, generator, loss_fn, args):
    """-> the mean MSE of the eval-mode outputs against the target clips, over all frames."""
    generator.train(False)
    losses = AverageMeter("loss")
    start = time.time()
    with torch.no_grad():
        for data in test_data_loader:
            in_text, text_lengths, target_vec, in_audio, aux_info = data
            in_text, target = in_text.to(device), target_vec.to(device).float()
            out_poses = generator(in_text, text_lengths, target, None)
            losses.update(float(loss_fn(out_poses, target)), target_vec.size(0))
    generator.train(True)
    logging.info("[VAL] loss: {:.3f} / {:.1f}s".format(losses.avg, time.time() - start))
    return losses.avg


def train_epochs(args, train_data_loader, test_data_loader, lang_model, pose_dim, trial_id=None):
    start = time.time()
    loss_meters = [AverageMeter("loss"), AverageMeter("var_loss")]
    print_interval = max(1, int(len(train_data_loader) / 5))
    save_model_epoch_interval = int(getattr(args, "save_every", 0)) or 20
    generator, loss_fn = init_model(args, lang_model, pose_dim, device)
    gen_optimizer = FlatClipAdam(generator.parameters(), lr=args.learning_rate, betas=(0.5, 0.999))
    val_metrics_list, loss_list = [], []
    for epoch in range(1, args.epochs + 1):
        val_metrics_list.append(evaluate_testset(test_data_loader, generator, loss_fn, args))
        if epoch % save_model_epoch_interval == 0 and epoch > 0:
            save_name = "{}/{}_checkpoint_{:03d}.bin".format(args.model_save_path, args.name, epoch)
            utils.train_utils.save_checkpoint(
                {"args": args, "epoch": epoch, "lang_model": lang_model, "pose_dim": pose_dim,
                 "gen_dict": generator.state_dict()}, save_name)
        iter_start_time = time.time()
        loss_epoch = AverageMeter("loss")
        for iter_idx, data in enumerate(train_data_loader, 0):
            in_text, text_lengths, target_vec, in_audio, aux_info = data
            batch_size = target_vec.size(0)
            in_text, target_vec = in_text.to(device), target_vec.to(device).float()
            loss = train_iter_seq2seq(args, epoch, in_text, text_lengths, target_vec, generator, gen_optimizer)
            loss_epoch.update(loss["loss"], batch_size)
            for m in loss_meters:
                if m.name in loss:
                    m.update(loss[m.name], batch_size)
            if (iter_idx + 1) % print_interval == 0:
                summary = "EP {} ({:3d}) | {:>8s}, {:.0f} samples/s | ".format(
                    epoch, iter_idx + 1, utils.train_utils.time_since(start), batch_size / (time.time() - iter_start_time))
                for m in loss_meters:
                    if m.count > 0:
                        summary += "{}: {:.3f}, ".format(m.name, m.avg)
                        m.reset()
                logging.info(summary)
            iter_start_time = time.time()
        loss_list.append(loss_epoch.avg)
    return generator, val_metrics_list, loss_list


def main(config: dict):
    args = config["args"]
    if args.random_seed >= 0:
        torch.manual_seed(args.random_seed)
        np.random.seed(args.random_seed)
        random.seed(args.random_seed)
    utils.train_utils.set_logger(args.model_save_path, os.path.basename(__file__).replace(".py", ".log"))
    logging.info(pprint.pformat(vars(args)))
    if not getattr(args, "synthetic", False):
        raise SystemExit("train.py: the baseline's data side (the pose-clip LMDB cache with a fastText vocabulary) is not built; "
                         "run with --synthetic")
    n_words = 3863
    g = torch.Generator().manual_seed(7)
    lang_model = SimpleNamespace(n_words=n_words,
                                 word_embedding_weights=torch.randn(n_words, args.wordembed_dim, generator=g).numpy())
    nb = getattr(args, "synthetic_batches", 8)
    train_loader = SyntheticClips(args, n_words, POSE_DIM, nb, seed=1234)
    test_loader = SyntheticClips(args, n_words, POSE_DIM, max(1, nb // 4), seed=4321)
    return train_epochs(args, train_loader, test_loader, lang_model, pose_dim=POSE_DIM)


if __name__ == "__main__":
    _args = parse_args()
    os.makedirs(_args.model_save_path, exist_ok=True)
    main({"args": _args})
