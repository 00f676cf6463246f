#!/usr/bin/env python3
"""Writes tests/golden/s2s_*.npz: what the REFERENCE single-direction seq2seq model (its
VSR_seq2seq_Transformer_with_phonemes_LRW/ package, imported at generation time from --reference) computes for
deterministic inputs and weights (detfill): preprocess, teacher-forced logits, loss, n_correct, gradients of a few named
parameters (the tied weight among them), greedy tokens and, per (row, step), the top-2 logit margin of the greedy decode.

    python tools/make_seq2seq_goldens.py --reference /path/to/VSR_seq2seq_Transformer_with_phonemes_LRW

The reference's decoder module unpickles 'bigram_freq.pkl' from the working directory at import (the file is not shipped and
nothing in forward / recognize_beam reads it), so the script runs from a temporary directory holding a pickled empty dict.
Its frontend's always-on F.dropout(p=0.5) and every nn.Dropout are switched off (parity mode, as for the SBL fixtures).

Token comparisons in the tests are exact and exclude no rows; that is sound only when no arg-max is a near tie, so the
script asserts that the smallest top-2 margin of every case is at least 10x the project's 1e-3 logit tolerance.  A case
that fails the assert gets another salt."""
import argparse
import json
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sbl_for_multilingual_lip_reading_amd import detfill  # noqa: E402

MIN_MARGIN = 10 * 1e-3
# gains of detfill.fill_value as a JSON object or the name of a detfill.GAIN_SETS entry.  With a tied weight the embedding gain
# also scales the logits, so it is kept moderate there.  The small and varied cases boost the cross-attention output
# projection, so that the greedy tokens depend on the clip (rows of a batch decode to different sequences) and a wrong
# cross-attention or a stale replay input shows in the tokens; gains and salts were picked for that and for the margin assert
TIED_GAINS = '{"tgt_word_emb": 6.0, "attn.fc.weight": 0.3, "w_2.weight": 0.3}'
SMALL_GAINS = '{"tgt_word_emb": 2.0, "enc_attn.fc.weight": 4.0, "w_2.weight": 0.3}'
VARIED_GAINS = '{"tgt_word_emb": 30.0, "enc_attn.fc.weight": 6.0, "slf_attn.fc.weight": 0.3, "w_2.weight": 0.3}'
# name: (encoder layers, decoder layers, vocab, weight sharing, B, T, H, W, salt, gains)
CASES = {
    "s2s_small": (1, 1, 42, True, 4, 6, 32, 32, 9, SMALL_GAINS),
    "s2s_varied": (1, 2, 48, False, 4, 8, 32, 32, 7, VARIED_GAINS),
    "s2s_full": (6, 6, 42, True, 2, 6, 32, 32, 7, TIED_GAINS),
}
GRAD_KEYS = ("decoder.tgt_word_emb.weight", "decoder.tgt_word_prj.weight", "decoder.layer_stack.0.slf_attn.w_qs.weight",
             "decoder.layer_stack.0.enc_attn.w_ks.weight", "decoder.layer_stack.0.pos_ffn.w_2.bias",
             "encoder.layer_stack.0.slf_attn.fc.weight", "lipreading.frontend3D.0.weight")


def targets(B, vocab, salt):
    """(B, 13) IGNORE_ID-padded targets of varied lengths; row 0 has length 1 and row 1 length 13."""
    _, tgt, _ = detfill.synthetic_batch(B, 1, 1, 1, salt, max_tgt=13, vocab=vocab)
    tgt[0, 1:] = -1
    ids = ((detfill.uniform("tgt_full", (13,), salt).astype(np.float64) + 1.0) * 0.5 * (vocab - 2)).astype(np.int64) + 2
    tgt[1] = np.clip(ids, 2, vocab - 1)
    return tgt


def sub(a):
    """Large matrices are stored as every 4th row / column."""
    return a[::4, ::4] if a.ndim == 2 and a.size > 65536 else a


def run_case(name, ref, out_dir):
    ne, nd, vocab, share, B, T, H, W, salt, gains = CASES[name]
    enc = ref["Encoder"](512, ne, 8, 64, 64, 512, 2048, dropout=0.0)
    dec = ref["Decoder"](0, 1, vocab, 512, nd, 8, 64, 64, 512, 2048, dropout=0.0, tgt_emb_prj_weight_sharing=share)
    model = ref["Transformer"](enc, dec)
    sd = model.state_dict()
    keys = list(sd.keys())
    fill = {}
    for k, v in sd.items():
        if k.endswith(".pe"):
            fill[k] = v
        elif share and k == "decoder.tgt_word_prj.weight":
            continue
        else:
            fill[k] = torch.from_numpy(detfill.fill_value(k, tuple(v.shape), salt, json.loads(gains) if gains.startswith("{") else gains).copy())
    if share:
        fill["decoder.tgt_word_prj.weight"] = fill["decoder.tgt_word_emb.weight"]
    model.load_state_dict(fill)
    x = torch.from_numpy(detfill.normal("clips", (B, T, H, W), salt))
    tgt = torch.from_numpy(targets(B, vocab, salt))

    # greedy decode (eval mode: BatchNorm running statistics), logits of every step through a hook on the projection
    model.eval()
    step_logits = []
    hook = dec.tgt_word_prj.register_forward_hook(lambda m, i, o: step_logits.append(o.detach().clone()))
    with torch.no_grad():
        ys = model.recognize(x.unsqueeze(-1), None, None)
    hook.remove()
    top2 = torch.stack(step_logits, 1).topk(2, dim=-1).values          # (B, T, 2)
    margins = (top2[..., 0] - top2[..., 1]).numpy()
    assert margins.shape == (B, T) and margins.min() >= MIN_MARGIN, (name, float(margins.min()))

    # teacher-forced step (train mode: batch statistics), loss as in train.py (label smoothing 0.1)
    model.train()
    ys_in, ys_out = dec.preprocess(tgt)
    pred, gold = model(x, tgt)
    loss, n_correct = ref["cal_performance"](pred, gold, smoothing=0.1)
    loss.backward()
    named = dict(model.named_parameters())
    out = {
        "meta": np.array([ne, nd, vocab, int(share), B, T, H, W, salt], dtype=np.int64), "gains": np.array(gains),
        "keys": np.array(keys), "shapes": np.array([",".join(str(d) for d in sd[k].shape) for k in keys]),
        "param_names": np.array([n for n, _ in model.named_parameters()]),
        "tgt": tgt.numpy(), "ys_in": ys_in.numpy(), "ys_out": ys_out.numpy(), "pred": pred.detach().numpy(),
        "gold": gold.numpy(), "loss": np.float64(loss.item()), "n_correct": np.int64(n_correct),
        "tokens": ys.numpy(), "margins": margins.astype(np.float32),
    }
    for k in GRAD_KEYS:
        p = named.get(k, named["decoder.tgt_word_emb.weight"] if share and k == "decoder.tgt_word_prj.weight" else None)
        out["grad:" + k] = sub(p.grad.numpy())
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **out)
    if B > 2:
        assert len({tuple(r) for r in ys.tolist()}) > 1, (name, "every clip decodes to the same tokens")
    print("%s: %d bytes, min margin %.4f, loss %.6f, n_correct %d, tokens row0 %s" % (
        path, os.path.getsize(path), margins.min(), loss.item(), n_correct, ys[0].tolist()))
    assert os.path.getsize(path) < (1 << 20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's VSR_seq2seq_Transformer_with_phonemes_LRW directory")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("cases", nargs="*", default=list(CASES))
    args = ap.parse_args()
    ref_dir = os.path.abspath(args.reference)
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "bigram_freq.pkl"), "wb") as f:
            pickle.dump({}, f)
        os.chdir(tmp)
        sys.path.insert(0, ref_dir)
        for m in [m for m in sys.modules if m == "config" or m.split(".")[0] == "transformer"]:
            del sys.modules[m]
        import torch.nn.functional as F
        F.dropout = lambda x, p=0.5, training=True, inplace=False: x        # the frontend's always-on dropout: parity mode
        from transformer.decoder import Decoder
        from transformer.encoder import Encoder
        from transformer.loss import cal_performance
        from transformer.transformer import Transformer
        ref = {"Decoder": Decoder, "Encoder": Encoder, "Transformer": Transformer, "cal_performance": cal_performance}
        torch.manual_seed(0)
        for name in args.cases:
            run_case(name, ref, args.out)
        os.chdir(ROOT)


if __name__ == "__main__":
    main()
