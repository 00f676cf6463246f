"""Plain-torch CPU restatement of the single-direction seq2seq model (the reference's
VSR_seq2seq_Transformer_with_phonemes_LRW/, "LRW/"), used by the tests only and pinned to tests/golden/s2s_*.npz (written
from the reference itself by tools/make_seq2seq_goldens.py) by test_seq2seq_cpu.py.  Built on the primitives of
oracle.sbl_oracle (frontend, encoder, attention and feed-forward sub-layers are the same modules in both models)."""
import json

import numpy as np
import torch
import torch.nn.functional as F

from oracle import sbl_oracle as O
from sbl_for_multilingual_lip_reading_amd import detfill

MAXLEN = 14          # LRW/transformer/utils.py:5


def preprocess(padded, sos_id=0, eos_id=1, ignore_id=-1):
    """LRW/transformer/decoder.py:64-79: (ys_in, ys_out), both (N, 14)."""
    N = padded.size(0)
    ys_in = torch.full((N, MAXLEN), eos_id, dtype=torch.long)
    ys_out = torch.full((N, MAXLEN), ignore_id, dtype=torch.long)
    for n in range(N):
        y = padded[n][padded[n] != ignore_id]
        ys_in[n, 0] = sos_id
        ys_in[n, 1:1 + len(y)] = y
        ys_out[n, :len(y)] = y
        ys_out[n, len(y)] = eos_id
    return ys_in, ys_out


def _layers(sd, x, enc, n_layers, slf_mask, cross_mask, non_pad, drop=0.0):
    for n in range(n_layers):
        p = "decoder.layer_stack.%d" % n
        x, _ = O.mha(sd, p + ".slf_attn", x, x, slf_mask, drop=drop)
        if non_pad is not None:
            x = x * non_pad
        x, _ = O.mha(sd, p + ".enc_attn", x, enc, cross_mask, drop=drop)
        if non_pad is not None:
            x = x * non_pad
        x = O.ffn(sd, p + ".pos_ffn", x, drop)
        if non_pad is not None:
            x = x * non_pad
    return x


def decoder_forward(sd, tgt, enc, n_layers, scale, enc_lengths=None, sos_id=0, eos_id=1, drop=0.0):
    """decoder.py:81-136 -> (pred (N, 14, V), gold (N, 14)).  drop > 0: train mode, every dropout decision through
    O._dropout in the order embedding, then per layer the self-attention probabilities and output, the cross-attention
    probabilities and output, the feed-forward output."""
    ys_in, ys_out = preprocess(tgt, sos_id, eos_id)
    N, L = ys_in.shape
    pad = ys_in.eq(eos_id)
    slf_mask = pad.unsqueeze(1) | torch.ones(L, L, dtype=torch.bool).triu(1).unsqueeze(0)
    cross_mask = None
    if enc_lengths is not None:
        cross_mask = (torch.arange(enc.size(1)).unsqueeze(0) >= torch.as_tensor(enc_lengths).unsqueeze(1)).unsqueeze(1).expand(-1, L, -1)
    x = O._dropout(sd["decoder.tgt_word_emb.weight"][ys_in] * scale + O.positional_encoding(L).unsqueeze(0), drop, drop > 0)
    x = _layers(sd, x, enc, n_layers, slf_mask, cross_mask, (~pad).to(x.dtype).unsqueeze(-1), drop)
    return F.linear(x, sd["decoder.tgt_word_prj.weight"]), ys_out


def recognize_beam(sd, enc, n_layers, scale, sos_id=0):
    """decoder.py:138-176: greedy, the whole prefix re-run at every step.  Returns (ys (N, T+1), logits (N, T, V))."""
    N, T, _ = enc.shape
    ys = torch.full((N, 1), sos_id, dtype=torch.long)
    logits = []
    for i in range(T):
        L = ys.size(1)
        x = sd["decoder.tgt_word_emb.weight"][ys] * scale + O.positional_encoding(L).unsqueeze(0)
        causal = torch.ones(L, L, dtype=torch.bool).triu(1).unsqueeze(0).expand(N, -1, -1)
        x = _layers(sd, x, enc, n_layers, causal, None, None)
        logits.append(F.linear(x[:, -1], sd["decoder.tgt_word_prj.weight"]))
        ys = torch.cat([ys, logits[-1].argmax(-1, keepdim=True)], 1)
    return ys, torch.stack(logits, 1)


def encode(sd, x, n_layers_enc, training):
    """LRW/transformer/transformer.py:26-37 (frontend dropout neutralised).  x: (N, T, H, W)."""
    N, T = x.shape[:2]
    y = O.stem(sd, x.unsqueeze(1), training, prefix="lipreading.frontend3D")
    y = y.transpose(1, 2).contiguous().view(-1, 64, y.size(3), y.size(4))
    feats = O.trunk(sd, y, training, prefix="lipreading.resnet18").view(N, T, 512)
    return O.encoder(sd, feats, n_layers_enc)


# --------------------------------------------------------------------------- fixtures
def case_config(g):
    ne, nd, vocab, share, B, T, H, W, salt = (int(v) for v in g["meta"])
    gains = str(g["gains"])
    return dict(ne=ne, nd=nd, vocab=vocab, share=bool(share), B=B, T=T, H=H, W=W, salt=salt,
                gains=json.loads(gains) if gains.startswith("{") else gains,
                scale=512 ** -0.5 if share else 1.0)


def case_state(g, requires_grad=False):
    """The deterministically filled state dict of a fixture (its key list and shapes come from the reference)."""
    c = case_config(g)
    sd = {}
    for k, shp in zip(g["keys"], g["shapes"]):
        k = str(k)
        if k.endswith(".pe"):
            continue
        shape = tuple(int(d) for d in str(shp).split(",") if d)
        t = torch.from_numpy(detfill.fill_value(k, shape, c["salt"], c["gains"]).copy())
        sd[k] = t.requires_grad_(True) if requires_grad and t.is_floating_point() and "running_" not in k else t
    if c["share"]:
        sd["decoder.tgt_word_prj.weight"] = sd["decoder.tgt_word_emb.weight"]
    return sd


def case_inputs(g):
    c = case_config(g)
    x = torch.from_numpy(detfill.normal("clips", (c["B"], c["T"], c["H"], c["W"]), c["salt"]))
    return x, torch.from_numpy(np.asarray(g["tgt"]))


def sub(a):
    """The generator stores large matrices as every 4th row / column."""
    return a[::4, ::4] if a.dim() == 2 and a.numel() > 65536 else a
