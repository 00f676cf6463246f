"""MultiHeadAttention and ScaledDotProductAttention with the class names, constructor and forward signatures and
state-dict keys of the reference's transformer/attention.py; compute is libsbl_hip.so."""
import math

import numpy as np
import torch
import torch.nn as nn

from ._env import ops


def _as_mask(mask, B, Lq, Lk):
    return ops._mask_args(mask, B, Lq, Lk)


class MultiHeadAttention(nn.Module):
    ''' Multi-Head Attention module (attention.py:6-60).

    forward(q, k, v, mask=None) -> (output, attn), attn shaped (n_head*B, Lq, Lk) like the reference.
    Extra, optional: mask='causal' (device-side triu, no mask tensor); kv_proj = pre-projected [K|V] of `k`
    (the decoder hoists it out of its 16-step loop).  The three projection weights are kept as adjacent rows of
    one fused (3*n_head*d_k, d_model) buffer so q/k/v come from a single MFMA GEMM; state-dict keys and shapes
    are unchanged (w_qs/w_ks/w_vs .weight/.bias).
    '''

    def __init__(self, n_head, d_model, d_k, d_v, dropout=0.1):
        super().__init__()
        if d_k != 64 or d_v != 64:
            raise ValueError("the HIP attention kernel is built for d_k = d_v = 64 (SBL/utils.py:94-97)")
        self.n_head = n_head
        self.d_k = d_k
        self.d_v = d_v

        self.w_qs = nn.Linear(d_model, n_head * d_k)
        self.w_ks = nn.Linear(d_model, n_head * d_k)
        self.w_vs = nn.Linear(d_model, n_head * d_v)
        for proj, d_head in ((self.w_qs, d_k), (self.w_ks, d_k), (self.w_vs, d_v)):     # N(0, 2 / (d_model + d_head))
            nn.init.normal_(proj.weight, std=math.sqrt(2.0 / (d_model + d_head)))

        self.attention = ScaledDotProductAttention(temperature=np.power(d_k, 0.5), attn_dropout=dropout)
        self.layer_norm = nn.LayerNorm(d_model)

        self.fc = nn.Linear(n_head * d_v, d_model)
        # Xavier-normal: N(0, 2 / (fan_in + fan_out))
        nn.init.normal_(self.fc.weight, std=math.sqrt(2.0 / (n_head * d_v + d_model)))

        self.dropout = nn.Dropout(dropout)
        # True when an owner keeps this module's (w_ks, w_vs) inside a block it lays out itself (the seq2seq decoder's
        # all-layers cross-attention K/V block): _fuse then leaves the parameters where they are
        self.kv_in_block = False

    def _fuse(self):
        """Re-point w_qs/w_ks/w_vs parameters at adjacent rows of one buffer (idempotent, cheap pointer check).
        Needed after construction, .to(device) or any external re-allocation of the parameters."""
        ws = (self.w_qs.weight, self.w_ks.weight, self.w_vs.weight)
        bs = (self.w_qs.bias, self.w_ks.bias, self.w_vs.bias)
        if ops._adjacent(*ws) and ops._adjacent(*bs):
            return
        if getattr(ws[0], "_sbl_flat", None) is not None or self.kv_in_block:
            # parameters of a dp.FlatModel are never re-allocated here.  Its layout keeps self-attention triples adjacent;
            # the decoder's cross-attention modules have (w_ks, w_vs) adjacent inside the all-layers K/V block instead,
            # which is all the cross-attention path (KVProjectFn / decoder_stages) needs
            assert ops._adjacent(*ws[1:]) and ops._adjacent(*bs[1:]), "flat model: K/V projection weights are not adjacent"
            return
        ops.fuse_rows(ws, bs)

    def _params(self, cross):
        """The leading arguments of ops.attn_handle, which are also those of ops.MHAFn after (x, kv)."""
        self._fuse()
        kv = (None,) * 4 if cross else (self.w_ks.weight, self.w_ks.bias, self.w_vs.weight, self.w_vs.bias)
        return (self.w_qs.weight, self.w_qs.bias) + kv + (self.fc.weight, self.fc.bias, self.layer_norm.weight, self.layer_norm.bias)

    def handle(self, cross=False):
        """This sub-layer's parameter handle for the ops.attn_* functions; cross: [K|V] come pre-projected."""
        return ops.attn_handle(*self._params(cross), self.n_head, self.dropout.p if self.training else 0.0, self.layer_norm.eps)

    def project_kv(self, k):
        """[K | V] = k [W_k; W_v]^T + [b_k; b_v], shape (B*Lk, 2*n_head*64) — attention.py:42-43 for both at once."""
        self._fuse()
        return ops.KVProjectFn.apply(k.reshape(-1, k.size(-1)), self.w_ks.weight, self.w_ks.bias,
                                     self.w_vs.weight, self.w_vs.bias)

    def forward_rows(self, x2, B, segL, mask=None, kv_proj=None, kv_group=None, kv_len=None):
        """Sub-layer on a ragged batch of rows: x2 (B*sum(segL), d_model); segment s holds B sequences of length
        segL[s] (the SBL decoder batches the steps of one teacher-forced run this way).  kv_proj=None: self-attention
        inside each segment; else cross-attention to the pre-projected [K|V] rows (B*Lk, 2*n_head*64).
        mask: None | 'causal' (| a (B,Lq,Lk) tensor when there is a single segment).  Returns (out rows, attn flat).
        kv_group = W (beam search; no_grad only, no mask): kv_proj holds B / W entries, sequence b attends to entry b // W,
        and no probabilities come back (attn is None).
        kv_len (no_grad only, no mask): device int32 key counts, one per kv_proj entry or - self-attention of one segment -
        per sequence; keys at or behind the count are not attended to (ops.attn_fwd); attn is None."""
        drop_p = self.dropout.p if self.training else 0.0
        if kv_group is not None or kv_len is not None:
            assert mask is None and not torch.is_grad_enabled() and (kv_proj is not None or kv_group is None)
            ops._need_cuda(x2, kv_proj, kv_len)
            seed, off_a, off_o = None, 0, 0
            if drop_p > 0:
                st = ops.dropout_state(x2.device)
                seed, off_a, off_o = st.seed, st.next_offset(), st.next_offset()
            y, _ = ops.attn_fwd(self.handle(cross=kv_proj is not None), x2.contiguous(), B, tuple(segL), kv_proj, 0, None, seed,
                                off_a, off_o, kv_group=kv_group, kv_len=kv_len)
            return y, None
        if isinstance(mask, str) or mask is None:
            mask_kind, mask_t = (1, None) if mask == "causal" else (0, None)
        else:
            assert len(segL) == 1
            Lk = segL[0] if kv_proj is None else kv_proj.size(0) // B
            mask_kind, mask_t = _as_mask(mask, B, segL[0], Lk)
        return ops.MHAFn.apply(x2, kv_proj, *self._params(kv_proj is not None), self.n_head, mask_kind, mask_t, drop_p,
                               self.layer_norm.eps, B, tuple(segL))

    def forward(self, q, k, v, mask=None, kv_proj=None):
        sz_b, len_q, d = q.size()
        len_k = k.size(1)
        if kv_proj is None and not (q is k and k is v):
            self._fuse()
            if k is v:
                kv_proj = self.project_kv(k)
            else:
                kk = ops.linear(k, self.w_ks.weight, self.w_ks.bias).reshape(-1, self.n_head * self.d_k)
                vv = ops.linear(v, self.w_vs.weight, self.w_vs.bias).reshape(-1, self.n_head * self.d_v)
                kv_proj = torch.cat([kk, vv], 1)
        out, attn = self.forward_rows(q.reshape(sz_b * len_q, d), sz_b, (len_q,), mask=mask, kv_proj=kv_proj)
        return out.view(sz_b, len_q, d), attn.view(self.n_head * sz_b, len_q, len_k)


class ScaledDotProductAttention(nn.Module):
    ''' Scaled Dot-Product Attention (attention.py:63-83).  q,k,v: (n_head*B, L, 64) as in the reference. '''

    def __init__(self, temperature, attn_dropout=0.1):
        super().__init__()
        self.temperature = temperature
        self.dropout = nn.Dropout(attn_dropout)
        self.softmax = nn.Softmax(dim=2)

    def forward(self, q, k, v, mask=None):
        G, Lq, d = q.shape
        Lk = k.size(1)
        if d != 64:
            raise ValueError("the HIP attention kernel is built for head dim 64")
        mask_kind, mask_t = _as_mask(mask, G, Lq, Lk)
        drop_p = self.dropout.p if self.training else 0.0
        # every (group) row is its own single-head "batch" entry for the kernel
        out, attn = ops.SDPAFn.apply(q.contiguous(), k.contiguous(), v.contiguous(), 1, 1.0 / float(self.temperature),
                                     mask_kind, mask_t, drop_p)
        return out, attn
