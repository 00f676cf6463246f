"""PositionalEncoding and PositionwiseFeedForward with the class surface of the reference's transformer/module.py."""
import math

import torch
import torch.nn as nn

from ._env import ops


class PositionalEncoding(nn.Module):
    """Sinusoidal position table as a buffer 'pe' of shape (1, max_len, d_model): column 2i holds sin(pos * w_i),
    column 2i+1 holds cos(pos * w_i), with w_i = 10000^(-2i/d_model) evaluated as exp(2i * -ln(10000)/d_model) in
    fp32 (the reference's rounding; the angle is one fp32 product).  Built once on the host at construction."""

    def __init__(self, d_model, max_len=5000):
        super(PositionalEncoding, self).__init__()
        freq = torch.exp(torch.arange(0, d_model, 2, dtype=torch.float32) * -(math.log(10000.0) / d_model))
        angle = torch.outer(torch.arange(max_len, dtype=torch.float32), freq)          # (max_len, d_model / 2)
        table = torch.stack((angle.sin(), angle.cos()), dim=-1).flatten(1)            # sin, cos interleaved
        self.register_buffer('pe', table.unsqueeze(0))

    def forward(self, input):
        """The first input.size(1) rows of the table, (1, T, d_model)."""
        return self.pe[:, :input.size(1)]


class PositionwiseFeedForward(nn.Module):
    """FFN(x) = LayerNorm(dropout(max(0, xW1 + b1)W2 + b2) + x) — module.py:35-52, one fused tape node."""

    def __init__(self, d_model, d_ff, dropout=0.1):
        super(PositionwiseFeedForward, self).__init__()
        self.w_1 = nn.Linear(d_model, d_ff)
        self.w_2 = nn.Linear(d_ff, d_model)
        self.dropout = nn.Dropout(dropout)
        self.layer_norm = nn.LayerNorm(d_model)

    def _params(self):
        """The arguments of ops.ffn_handle, which are also those of ops.FFNFn after x."""
        return (self.w_1.weight, self.w_1.bias, self.w_2.weight, self.w_2.bias, self.layer_norm.weight, self.layer_norm.bias,
                self.dropout.p if self.training else 0.0, self.layer_norm.eps)

    def handle(self):
        """This sub-layer's parameter handle for the ops.ffn_* functions."""
        return ops.ffn_handle(*self._params())

    def forward(self, x):
        return ops.FFNFn.apply(x, *self._params())


def mask_rows(x, non_pad_mask):
    """x * non_pad_mask (zeroes the padded positions) as one tape node; x itself when there is no mask."""
    return x if non_pad_mask is None else ops.RowScaleFn.apply(x, non_pad_mask)
