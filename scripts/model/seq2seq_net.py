"""`model.seq2seq_net` -- drop-in module path of the reference (scripts/model/seq2seq_net.py);
implementation in gesture2vec_amd.model.seq2seq_net."""
import os as _os
import sys as _sys

_ROOT = _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
if _ROOT not in _sys.path:
    _sys.path.insert(0, _ROOT)

from gesture2vec_amd.model.seq2seq_net import (  # noqa: E402,F401
    Attn, BahdanauAttnDecoderRNN, EncoderRNN, Generator, Seq2SeqNet)
