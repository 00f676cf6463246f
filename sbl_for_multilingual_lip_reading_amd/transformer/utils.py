"""Host-side mask and padding helpers with the names, dtypes and shapes of the reference's
SBL_Multilingual_Lip_reading/transformer/utils.py (:1-9, :98-147), built batch-at-once (no per-sample loop).
Of these, the encoder uses the two length masks (and only for ragged batches); the decoder builds its masks on the
device.  The rest are kept for code written against the reference."""
import torch

from ._env import _lib

_PAD_LEN = 16      # pad_list pads to a fixed length (the decoder's 16 steps), not to the longest sequence


def pad_list(xs, pad_value):
    """Stack 1-d (or (L, ...)) tensors of lengths <= 16 into (len(xs), 16, ...) of xs[0]'s dtype, filled with
    pad_value past each length."""
    packed = torch.nn.utils.rnn.pad_sequence(xs, batch_first=True, padding_value=pad_value)
    out = xs[0].new_full((len(xs), _PAD_LEN) + tuple(xs[0].shape[1:]), pad_value)
    out[:, :packed.size(1)] = packed
    return out


def _valid_positions(padded_input, input_lengths):
    """Bool (N, T, ...) over padded_input.shape[:-1]: True at time steps t < input_lengths[n]."""
    n, t = padded_input.shape[:2]
    lengths = torch.as_tensor(input_lengths, device=padded_input.device).view(n, 1)
    valid = torch.arange(t, device=padded_input.device) < lengths
    return valid.view(n, t, *(1,) * (padded_input.dim() - 3)).expand(padded_input.shape[:-1])


def get_non_pad_mask(padded_input, input_lengths=None, pad_idx=None):
    """(..., 1) mask that is 1 on real positions and 0 on padding, from per-sample lengths (in padded_input's dtype)
    or from the token id pad_idx of a 2-d id tensor (float32); pad_idx wins when both are given."""
    if pad_idx is None:
        assert input_lengths is not None, "get_non_pad_mask needs input_lengths or pad_idx"
        return _valid_positions(padded_input, input_lengths).to(padded_input.dtype).unsqueeze(-1)
    assert padded_input.ndim == 2, "a pad_idx mask is built from (N, T) token ids"
    return padded_input.ne(pad_idx).float().unsqueeze(-1)


def get_subsequent_mask(seq):
    """Causal mask for ids seq (N, L): uint8 (N, L, L), 1 above the diagonal (the future keys), one shared (L, L)
    table expanded over the batch."""
    n, length = seq.shape
    future = torch.ones((length, length), dtype=torch.uint8, device=seq.device).triu(1)
    return future.expand(n, length, length)


def get_attn_key_pad_mask(seq_k, seq_q, pad_idx):
    """Bool (N, Lq, Lk), True where key id seq_k[n, j] == pad_idx; a view expanded over the query length."""
    return seq_k.eq(pad_idx).unsqueeze(1).expand(-1, seq_q.size(1), -1)


def get_attn_pad_mask(padded_input, input_lengths, expand_length):
    """Bool (N, expand_length, T), True on padded key positions; a view expanded over the query length."""
    padded = ~_valid_positions(padded_input, input_lengths)
    return padded.unsqueeze(1).expand(-1, expand_length, -1)


def device_lengths(encoder_input_lengths, encoder_outputs):
    """The cross-attention key counts of a decode (the `_kv_len` of both decoders): None, or the clips' frame counts as the
    device int32 (N,) tensor the `_len` kernels read.  A host sequence is copied once; a CUDA int32 tensor is used as it is and
    never read on the host."""
    lens = encoder_input_lengths
    if lens is None:
        return None
    if not (isinstance(lens, torch.Tensor) and lens.is_cuda):
        lens = torch.as_tensor(lens, dtype=torch.int32).to(encoder_outputs.device)
    if lens.dtype != torch.int32 or lens.shape != (encoder_outputs.size(0),) or not lens.is_contiguous():
        raise _lib.SblHipError("encoder_input_lengths: a contiguous int32 (%d,) tensor, got %s %s"
                               % (encoder_outputs.size(0), lens.dtype, tuple(lens.shape)))
    return lens
