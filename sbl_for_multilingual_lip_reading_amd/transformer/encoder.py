"""Encoder and EncoderLayer with the constructor / forward signatures and state-dict keys of the reference's
transformer/encoder.py."""
import torch
import torch.nn as nn

from ._env import ops
from .attention import MultiHeadAttention
from .module import PositionalEncoding, PositionwiseFeedForward, mask_rows
from .utils import get_non_pad_mask, get_attn_pad_mask


class Encoder(nn.Module):
    """Frame features (N, T, d_input) -> dropout(LayerNorm(linear_in(x)) + PE) -> n_layers post-norm
    self-attention + FFN layers -> (N, T, d_model).  Positions past input_lengths[n] are masked out as keys and
    zeroed after every sub-layer.  With gradients disabled a ragged batch takes the key-count attention kernels
    (sbl_attention_seg_len_fwd: no mask tensor, the padded frames' K/V rows are never read); with gradients enabled
    the explicit (N, T, T) mask."""

    def __init__(self, d_input, n_layers, n_head, d_k, d_v,
                 d_model, d_inner, dropout=0.1, pe_maxlen=5000):
        super(Encoder, self).__init__()
        self.d_input = d_input
        self.n_layers = n_layers
        self.n_head = n_head
        self.d_k = d_k
        self.d_v = d_v
        self.d_model = d_model
        self.d_inner = d_inner
        self.dropout_rate = dropout
        self.pe_maxlen = pe_maxlen

        self.linear_in = nn.Linear(d_input, d_model)
        self.layer_norm_in = nn.LayerNorm(d_model)
        self.positional_encoding = PositionalEncoding(d_model, max_len=pe_maxlen)
        self.dropout = nn.Dropout(dropout)
        self.layer_stack = nn.ModuleList(EncoderLayer(d_model, d_inner, n_head, d_k, d_v, dropout)
                                         for _ in range(n_layers))

    def forward(self, padded_input, input_lengths, return_attns=False):
        """padded_input (N, T, d_input); input_lengths: N ints on the host (ragged when one is < T), or a CUDA int32 (N,)
        tensor, which is never read on the host and always counts as ragged.  Returns (out,) or, with return_attns,
        (out, [per-layer attention (n_head*N, T, T)])."""
        N, T, _ = padded_input.shape
        on_device = isinstance(input_lengths, torch.Tensor) and input_lengths.is_cuda
        kv_len = None
        if not on_device and all(int(l) >= T for l in input_lengths):
            # full-length batch (what Transformer passes without lengths): every mask would be a no-op
            non_pad_mask, slf_attn_mask = None, None
        elif torch.is_grad_enabled() or return_attns:
            non_pad_mask = get_non_pad_mask(padded_input, input_lengths)
            slf_attn_mask = get_attn_pad_mask(padded_input, input_lengths, T)
        else:
            kv_len = input_lengths if on_device else torch.as_tensor([int(l) for l in input_lengths], dtype=torch.int32)
            kv_len = kv_len.to(device=padded_input.device, dtype=torch.int32).contiguous().view(N)
            non_pad_mask, slf_attn_mask = get_non_pad_mask(padded_input, kv_len), None

        # the layers' weight gradients are deferred and issued as one grouped launch when backward reaches the
        # encoder input (second stream, under the frontend backward) or at the end of backward, whichever is first
        if torch.is_grad_enabled() and padded_input.requires_grad:
            padded_input.register_hook(lambda g: ops.flush_deferred())
        with ops.deferring():
            h = ops.linear(padded_input, self.linear_in.weight, self.linear_in.bias)
            h = ops.add_layernorm(h, None, self.layer_norm_in.weight, self.layer_norm_in.bias, self.layer_norm_in.eps)
            h = ops.AddPEFn.apply(h, self.positional_encoding.pe[0, :T])
            h = ops.dropout(h, self.dropout.p, self.training)

            attns = [] if return_attns else None
            for layer in self.layer_stack:
                h, attn = layer(h, non_pad_mask=non_pad_mask, slf_attn_mask=slf_attn_mask, kv_len=kv_len)
                if attns is not None:
                    attns.append(attn)
        return (h,) if attns is None else (h, attns)


class EncoderLayer(nn.Module):
    """Self-attention sub-layer, then position-wise FFN sub-layer (each post-norm with its own residual)."""

    def __init__(self, d_model, d_inner, n_head, d_k, d_v, dropout=0.1):
        super(EncoderLayer, self).__init__()
        self.slf_attn = MultiHeadAttention(n_head, d_model, d_k, d_v, dropout=dropout)
        self.pos_ffn = PositionwiseFeedForward(d_model, d_inner, dropout=dropout)

    def forward(self, enc_input, non_pad_mask=None, slf_attn_mask=None, kv_len=None):
        """kv_len (no_grad only, instead of slf_attn_mask): device int32 (N,), the keys t < kv_len[n] are attended to."""
        if kv_len is not None:
            N, T, D = enc_input.shape
            h, attn = self.slf_attn.forward_rows(enc_input.reshape(N * T, D), N, (T,), kv_len=kv_len)
            h = h.view(N, T, D)
        else:
            h, attn = self.slf_attn(enc_input, enc_input, enc_input, mask=slf_attn_mask)
        h = mask_rows(h, non_pad_mask)
        return mask_rows(self.pos_ffn(h), non_pad_mask), attn
