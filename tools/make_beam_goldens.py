#!/usr/bin/env python3
"""Writes tests/golden/beam_*.npz: what the REFERENCE's LRW1000 beam search (Decoder.recognize_beam of its
VSR_seq2seq_Transformer_with_phonemes_LRW1000/ package, imported at generation time from --reference) returns for
deterministic inputs and weights (detfill), clip by clip: the n-best token sequences, their lengths and scores; and, from the
in-repo restatement tests/beam_oracle.py - after asserting that its n-best equals the reference's - the tokens, parents,
scores and flags kept at every (clip, step, rank), which is what lets a failing GPU test name the first diverging step.

    python tools/make_beam_goldens.py --reference /path/to/VSR_seq2seq_Transformer_with_phonemes_LRW1000

How the reference is driven:
  * its decoder module reads an undefined global `bigram_freq` (decoder.py:163); the script sets it to the case's table
    (an all-ones table, log = 0, for the cases without a prior);
  * its Transformer loads a pretrained frontend from a path at construction and its recognize() names an attribute that
    class does not have, so frontend, encoder and decoder are built on their own, held under the attribute names of the LRW
    model (whose state-dict keys seq2seq.Seq2SeqTransformer keeps), and recognize_beam is called on each clip's encoder output;
  * the frontend's always-on F.dropout(p=0.5) and every nn.Dropout are switched off (parity mode, as for the s2s fixtures);
  * its attention passes a uint8 mask to masked_fill, which current torch refuses: the mask is cast to bool on the way in.

Token comparisons in the tests are exact and leave nothing out; that is sound only when no decision is a near tie, so the
script asserts that every decision gap (rank W against rank W+1 among the finite candidates and adjacent kept ranks at every
step, adjacent final ranks, rank nbest against the next) is at least 10x the score tolerance of 1e-3 per accumulated step.
A case that fails an assert gets another salt or other gains; the ones below were picked on the CPU with this script."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from sbl_for_multilingual_lip_reading_amd import detfill  # noqa: E402

# gains of detfill.fill_value (see tools/make_seq2seq_goldens.py); the untied case also scales the output projection
SMALL_GAINS = '{"tgt_word_emb": 6.0, "enc_attn.fc.weight": 4.0, "w_2.weight": 0.3}'
VARIED_GAINS = '{"tgt_word_emb": 30.0, "tgt_word_prj": 4.0, "enc_attn.fc.weight": 6.0, "slf_attn.fc.weight": 0.3, "w_2.weight": 0.3}'
TIED_GAINS = '{"tgt_word_emb": 6.0, "attn.fc.weight": 0.3, "w_2.weight": 0.3}'
# name: (encoder layers, decoder layers, vocab, weight sharing, B, T, H, W, salt, gains, beam, nbest, decode_max_len, prior)
CASES = {
    "beam_small": (1, 1, 42, True, 4, 6, 32, 32, 68, SMALL_GAINS, 3, 3, 0, False),
    "beam_varied": (1, 2, 48, False, 4, 8, 32, 32, 79, VARIED_GAINS, 5, 2, 0, True),
    "beam_varied_len5": (1, 2, 48, False, 4, 8, 32, 32, 42, VARIED_GAINS, 5, 2, 5, True),
    "beam_full": (6, 6, 42, True, 2, 6, 32, 32, 14, TIED_GAINS, 4, 1, 0, False),
}


class Holder(torch.nn.Module):
    """The reference's three parts under the LRW model's attribute names and registration order."""

    def __init__(self, encoder, decoder, lipreading):
        super().__init__()
        self.encoder = encoder
        self.decoder = decoder
        self.lipreading = lipreading


def run_case(name, ref, out_dir):
    import beam_oracle as B
    import seq2seq_oracle as S
    ne, nd, vocab, share, Bsz, T, H, W, salt, gains, beam, nbest, dml, prior = CASES[name]
    model = Holder(ref["Encoder"](512, ne, 8, 64, 64, 512, 2048, dropout=0.0),
                   ref["Decoder"](0, 1, vocab, 512, nd, 8, 64, 64, 512, 2048, dropout=0.0, tgt_emb_prj_weight_sharing=share),
                   ref["Lipreading"](hiddenDim=512, embedSize=256))
    sd = model.state_dict()
    keys = list(sd.keys())
    gd = json.loads(gains)
    fill = {}
    for k, v in sd.items():
        if k.endswith(".pe"):
            fill[k] = v
        elif share and k == "decoder.tgt_word_prj.weight":
            continue
        else:
            fill[k] = torch.from_numpy(detfill.fill_value(k, tuple(v.shape), salt, gd).copy())
    if share:
        fill["decoder.tgt_word_prj.weight"] = fill["decoder.tgt_word_emb.weight"]
    model.load_state_dict(fill)
    model.eval()
    freq = B.make_freq(vocab, salt) if prior else np.ones((vocab, vocab), dtype=np.float32)
    ref["decoder_module"].bigram_freq = freq
    x = torch.from_numpy(detfill.normal("clips", (Bsz, T, H, W), salt))
    args = types.SimpleNamespace(beam_size=beam, nbest=nbest, decode_max_len=dml)
    maxlen = dml or T
    with torch.no_grad():
        feats = model.lipreading(x.unsqueeze(1))
        enc, *_ = model.encoder(feats, [T] * Bsz)
        hyps = [model.decoder.recognize_beam(enc[b], None, args) for b in range(Bsz)]
    hyps = [[h for h in hs if float(h["score"]) > -np.inf] for hs in hyps]       # the oracle never keeps a score of -inf
    yseq = np.full((Bsz, nbest, maxlen + 2), 1, dtype=np.int64)
    lengths = np.zeros((Bsz, nbest), dtype=np.int32)
    scores = np.full((Bsz, nbest), -np.inf, dtype=np.float32)
    for b, hs in enumerate(hyps):
        for k, h in enumerate(hs):
            yseq[b, k, :len(h["yseq"])], lengths[b, k], scores[b, k] = h["yseq"], len(h["yseq"]), float(h["score"])
    n_hyps = np.array([len(hs) for hs in hyps], dtype=np.int32)

    g = {"meta": np.array([ne, nd, vocab, int(share), Bsz, T, H, W, salt], dtype=np.int64), "gains": np.array(gains),
         "keys": np.array(keys), "shapes": np.array([",".join(str(d) for d in sd[k].shape) for k in keys]),
         "beam": np.array([beam, nbest, dml], dtype=np.int64)}
    if prior:
        g["freq"] = freq
    c = B.beam_config(g)
    osd = S.case_state(g)
    with torch.no_grad():
        o = B.beam_search(osd, S.encode(osd, x, ne, training=False), nd, c["scale"], beam, nbest, dml, B.log_prior(g))
    assert np.array_equal(o["yseq"], yseq) and np.array_equal(o["lengths"], lengths) and np.array_equal(o["n_hyps"], n_hyps), (
        name, "the oracle's n-best differs from the reference's", o["yseq"].tolist(), yseq.tolist())
    assert float(np.abs(o["scores"] - scores).max()) < 1e-4, (name, o["scores"], scores)
    assert o["margin"] >= B.margin_floor(maxlen), (name, "margin", o["margin"], B.margin_floor(maxlen))
    # a clip read through another clip's cross-attention cache has to show: every two clips differ in their 1-best tokens or by
    # more than the margin floor in a score
    for a in range(Bsz):
        for b in range(a):
            assert not np.array_equal(yseq[a, 0], yseq[b, 0]) or np.abs(scores[a] - scores[b]).max() > B.margin_floor(maxlen), (name, a, b)
    if prior:
        with np.errstate(divide="ignore"):
            lp = np.log(freq)
        assert np.isinf(lp).any() and (np.isfinite(lp).sum(1) >= beam).all()
        assert (o["early"] > 0).any(), (name, "no hypothesis ends before the last step")
        assert (o["min_live"] < beam).any(), (name, "the live count never falls below the beam")
        assert (o["early"] < nbest).any() or (o["min_live"] == 0).any(), (name, o["early"], o["min_live"])
    g.update(yseq=yseq, lengths=lengths, scores=scores, n_hyps=n_hyps, margin=np.float32(o["margin"]),
             **{k: o[k] for k in ("hist_tok", "hist_par", "hist_score", "hist_flag")})
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **g)
    print("%s: %d bytes, margin %.4f (floor %.3f), early %s, min live %s, 1-best of clip 0 %s" % (
        path, os.path.getsize(path), o["margin"], B.margin_floor(maxlen), o["early"].tolist(), o["min_live"].tolist(),
        yseq[0, 0, :lengths[0, 0]].tolist()))
    assert os.path.getsize(path) < (1 << 20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's VSR_seq2seq_Transformer_with_phonemes_LRW1000 directory")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("cases", nargs="*", default=list(CASES))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    for m in [m for m in sys.modules if m == "config" or m.split(".")[0] == "transformer"]:
        del sys.modules[m]
    import torch.nn.functional as F
    F.dropout = lambda x, p=0.5, training=True, inplace=False: x        # the frontend's always-on dropout: parity mode
    masked_fill = torch.Tensor.masked_fill
    torch.Tensor.masked_fill = lambda self, mask, value: masked_fill(self, mask.bool(), value)
    import transformer.decoder as decoder_module
    from transformer.encoder import Encoder
    from transformer.video_frontend import Lipreading
    ref = {"Decoder": decoder_module.Decoder, "Encoder": Encoder, "Lipreading": Lipreading, "decoder_module": decoder_module}
    torch.manual_seed(0)
    for name in args.cases:
        run_case(name, ref, args.out)


if __name__ == "__main__":
    main()
