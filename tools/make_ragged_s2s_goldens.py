#!/usr/bin/env python3
"""Writes tests/golden/ragged_s2s_*.npz: what the REFERENCE's single-direction models decode for every clip of a ragged batch
when the clip is given to them ALONE, cut to its own frame count - the oracle of Seq2SeqTransformer.recognize(x,
input_lengths=) and of the beam search with lengths.

    python tools/make_ragged_s2s_goldens.py --lrw /path/to/VSR_seq2seq_Transformer_with_phonemes_LRW \\
                                            --lrw1000 /path/to/VSR_seq2seq_Transformer_with_phonemes_LRW1000

  * ragged_s2s_small: the LRW model's greedy decode (Transformer.recognize, maxlen = the clip's frame count), driven as
    tools/make_seq2seq_goldens.py drives it: the padded clips, the lengths, the encoder rows, every step's logits and tokens and
    the top-2 margins; rows / steps behind a clip's length are zero, tokens there are <eos>.
  * ragged_s2s_beam: the LRW1000 decoder's beam search (Decoder.recognize_beam per clip, decode_max_len = 0, so maxlen = the
    clip's frame count), driven as tools/make_beam_goldens.py drives it: the n-best sequences, lengths and scores, and - from
    the restatement tests/ragged_s2s_oracle.py, once its n-best equals the reference's - the per-step history.

The models are in eval mode with every dropout off, so a clip's features do not depend on its batch.  The script asserts the
margin floors the project uses (10 x 1e-3 for the greedy logits, beam_oracle.margin_floor(T) for every beam decision), that no
two clips decode alike, and that the padded batch decoded at full length gives another result for a short clip.  A case that
fails an assert gets another salt, picked here on the CPU."""
import argparse
import json
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from sbl_for_multilingual_lip_reading_amd import detfill  # noqa: E402
import beam_oracle as Bo  # noqa: E402  (the restatements are imported before any reference directory joins sys.path)
import ragged_s2s_oracle as R  # noqa: E402
import seq2seq_oracle as S  # noqa: E402

SMALL_GAINS = '{"tgt_word_emb": 2.0, "enc_attn.fc.weight": 4.0, "w_2.weight": 0.3}'
VARIED_GAINS = '{"tgt_word_emb": 30.0, "tgt_word_prj": 4.0, "enc_attn.fc.weight": 6.0, "slf_attn.fc.weight": 0.3, "w_2.weight": 0.3}'
# name: (encoder layers, decoder layers, vocab, weight sharing, B, T, H, W, lengths, salt, gains[, beam, nbest])
CASES = {
    "ragged_s2s_small": (1, 1, 42, True, 4, 8, 32, 32, (8, 5, 1, 3), 9, SMALL_GAINS),
    "ragged_s2s_beam": (1, 2, 48, False, 4, 8, 32, 32, (8, 5, 2, 3), 581, VARIED_GAINS, 5, 2),
}


class Holder(torch.nn.Module):
    """The LRW1000 reference's three parts under the LRW model's attribute names and registration order."""

    def __init__(self, encoder, decoder, lipreading):
        super().__init__()
        self.encoder = encoder
        self.decoder = decoder
        self.lipreading = lipreading


def fill(model, share, salt, gains):
    sd = model.state_dict()
    out = {}
    for k, v in sd.items():
        if k.endswith(".pe"):
            out[k] = v
        elif share and k == "decoder.tgt_word_prj.weight":
            continue
        else:
            out[k] = torch.from_numpy(detfill.fill_value(k, tuple(v.shape), salt, json.loads(gains)).copy())
    if share:
        out["decoder.tgt_word_prj.weight"] = out["decoder.tgt_word_emb.weight"]
    model.load_state_dict(out)
    model.eval()
    return {"keys": np.array(list(sd.keys())), "shapes": np.array([",".join(str(d) for d in sd[k].shape) for k in sd])}


def import_reference(ref_dir):
    sys.path.insert(0, os.path.abspath(ref_dir))
    for m in [m for m in sys.modules if m == "config" or m.split(".")[0] == "transformer"]:
        del sys.modules[m]
    import transformer.decoder as decoder_module
    from transformer.encoder import Encoder
    from transformer.video_frontend import Lipreading
    mods = {"decoder_module": decoder_module, "Decoder": decoder_module.Decoder, "Encoder": Encoder, "Lipreading": Lipreading}
    sys.path.pop(0)
    return mods


def run_greedy(name, ref, out_dir, salt=None):
    ne, nd, vocab, share, B, T, H, W, lengths, salt0, gains = CASES[name]
    salt = salt0 if salt is None else salt
    from transformer.transformer import Transformer          # the LRW package is the one imported last
    model = Transformer(ref["Encoder"](512, ne, 8, 64, 64, 512, 2048, dropout=0.0),
                        ref["Decoder"](0, 1, vocab, 512, nd, 8, 64, 64, 512, 2048, dropout=0.0, tgt_emb_prj_weight_sharing=share))
    g = fill(model, share, salt, gains)
    g.update(meta=np.array([ne, nd, vocab, int(share), B, T, H, W, salt], dtype=np.int64), gains=np.array(gains),
             lengths=np.array(lengths, dtype=np.int32))
    x = R.clips(R.config(g), lengths)
    grabbed = {"logits": []}
    model.encoder.register_forward_hook(lambda m, i, o: grabbed.__setitem__("enc", o[0].detach().clone()))
    model.decoder.tgt_word_prj.register_forward_hook(lambda m, i, o: grabbed["logits"].append(o.detach().clone()))
    enc = np.zeros((B, T, 512), dtype=np.float32)
    logits = np.zeros((B, T, vocab), dtype=np.float32)
    tokens = np.full((B, T + 1), 1, dtype=np.int64)
    margins = np.full((B, T), np.inf, dtype=np.float32)
    for n, l in enumerate(lengths):
        grabbed["logits"] = []
        with torch.no_grad():
            ys = model.recognize(x[n:n + 1, :l].unsqueeze(-1), None, None)          # the clip alone, cut to its length
        assert grabbed["enc"].shape == (1, l, 512) and len(grabbed["logits"]) == l and ys.shape == (1, l + 1)
        enc[n, :l] = grabbed["enc"][0].numpy()
        logits[n, :l] = torch.cat(grabbed["logits"], 0).numpy()
        tokens[n, :l + 1] = ys[0].numpy()
        top2 = np.sort(logits[n, :l], -1)[:, -2:]
        margins[n, :l] = top2[:, 1] - top2[:, 0]
    assert np.array_equal(np.where(np.isfinite(margins), logits.argmax(-1), 1), tokens[:, 1:])
    assert margins.min() >= R.MIN_MARGIN, (name, float(margins.min()))
    assert len({tuple(t.tolist()) for t in tokens}) == B, (name, "two clips decode alike")
    with torch.no_grad():
        padded = model.recognize(x.unsqueeze(-1), None, None).numpy()               # the padding attended to, all T steps
    assert any(l < T and not np.array_equal(padded[n, :l + 1], tokens[n, :l + 1]) for n, l in enumerate(lengths)), (name, "padding changes no tokens")
    # the restatement equals the reference
    sd = S.case_state(g)
    with torch.no_grad():
        oenc = R.encode_cut(sd, x, lengths, ne)
        otok, olog, _ = R.greedy(sd, oenc, lengths, nd, R.config(g)["scale"])
    assert np.array_equal(otok, tokens) and float(np.abs(olog - logits).max()) < 1e-3 and float(np.abs(oenc.numpy() - enc).max()) < 1e-3
    g.update(clips=x.numpy(), enc=enc, logits=logits, tokens=tokens, margins=margins, tokens_padded=padded)
    save(name, g, out_dir, "min margin %.4f, tokens %s" % (margins.min(), tokens[:, 1:4].tolist()))


def run_beam(name, ref, out_dir, salt=None):
    ne, nd, vocab, share, B, T, H, W, lengths, salt0, gains, beam, nbest = CASES[name]
    salt = salt0 if salt is None else salt
    model = Holder(ref["Encoder"](512, ne, 8, 64, 64, 512, 2048, dropout=0.0),
                   ref["Decoder"](0, 1, vocab, 512, nd, 8, 64, 64, 512, 2048, dropout=0.0, tgt_emb_prj_weight_sharing=share),
                   ref["Lipreading"](hiddenDim=512, embedSize=256))
    g = fill(model, share, salt, gains)
    freq = Bo.make_freq(vocab, salt)
    ref["decoder_module"].bigram_freq = freq
    g.update(meta=np.array([ne, nd, vocab, int(share), B, T, H, W, salt], dtype=np.int64), gains=np.array(gains),
             lengths=np.array(lengths, dtype=np.int32), beam=np.array([beam, nbest, 0], dtype=np.int64), freq=freq)
    x = R.clips(R.config(g), lengths)
    args = types.SimpleNamespace(beam_size=beam, nbest=nbest, decode_max_len=0)

    def reference(clips_, lens):
        """n-best of every clip alone, cut to lens[n] frames, in the batched layout for maxlen = T."""
        yseq = np.full((B, nbest, T + 2), 1, dtype=np.int64)
        lengths_ = np.zeros((B, nbest), dtype=np.int32)
        scores = np.full((B, nbest), -np.inf, dtype=np.float32)
        n_hyps = np.zeros(B, dtype=np.int32)
        for n, l in enumerate(lens):
            with torch.no_grad():
                feats = model.lipreading(clips_[n:n + 1, :l].unsqueeze(1))
                enc, *_ = model.encoder(feats, [l])
                hyps = model.decoder.recognize_beam(enc[0], None, args)
            hyps = [h for h in hyps if float(h["score"]) > -np.inf]           # the oracle never keeps a score of -inf
            n_hyps[n] = len(hyps)
            for k, h in enumerate(hyps):
                yseq[n, k, :len(h["yseq"])], lengths_[n, k], scores[n, k] = h["yseq"], len(h["yseq"]), float(h["score"])
        return yseq, lengths_, scores, n_hyps

    yseq, hyp_len, scores, n_hyps = reference(x, lengths)
    sd = S.case_state(g)
    with torch.no_grad():
        oenc = R.encode_cut(sd, x, lengths, ne)
        o = R.beam(sd, oenc, lengths, nd, R.config(g)["scale"], beam, nbest, Bo.log_prior(g))
    assert np.array_equal(o["yseq"], yseq) and np.array_equal(o["lengths"], hyp_len) and np.array_equal(o["n_hyps"], n_hyps), (
        name, "the restatement's n-best differs from the reference's", o["yseq"].tolist(), yseq.tolist())
    assert float(np.abs(o["scores"] - scores).max()) < 1e-4, (name, o["scores"], scores)
    assert o["margin"] >= Bo.margin_floor(T), (name, "margin", o["margin"], Bo.margin_floor(T))
    for a in range(B):
        for b in range(a):
            assert not np.array_equal(yseq[a, 0], yseq[b, 0]) or np.abs(scores[a] - scores[b]).max() > Bo.margin_floor(T), (name, "clips decode alike", a, b)
    pad = reference(x, [T] * B)                                                    # the padding encoded and attended to
    assert any(l < T and not np.array_equal(pad[0][n, 0], yseq[n, 0]) for n, l in enumerate(lengths)), (name, "padding changes no 1-best")
    assert all(hyp_len[n, 0] <= l + 2 for n, l in enumerate(lengths))
    g.update(clips=x.numpy(), enc=oenc.numpy(), yseq=yseq, hyp_lengths=hyp_len, scores=scores, n_hyps=n_hyps,
             margin=np.float32(o["margin"]), yseq_padded=pad[0][:, 0], **{k: o[k] for k in ("hist_tok", "hist_par", "hist_score", "hist_flag")})
    save(name, g, out_dir, "margin %.4f (floor %.3f), 1-best %s" % (o["margin"], Bo.margin_floor(T), [yseq[n, 0, :hyp_len[n, 0]].tolist() for n in range(B)]))


def save(name, g, out_dir, note):
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **g)
    print("%s: %d bytes, %s" % (path, os.path.getsize(path), note))
    assert os.path.getsize(path) < (1 << 20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lrw", required=True, help="the reference's VSR_seq2seq_Transformer_with_phonemes_LRW directory")
    ap.add_argument("--lrw1000", required=True, help="the reference's VSR_seq2seq_Transformer_with_phonemes_LRW1000 directory")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--salt", type=int, default=None, help="try another salt (for picking one; the cases name theirs)")
    ap.add_argument("cases", nargs="*", default=list(CASES))
    args = ap.parse_args()
    import torch.nn.functional as F
    F.dropout = lambda x, p=0.5, training=True, inplace=False: x        # the frontend's always-on dropout: parity mode
    masked_fill = torch.Tensor.masked_fill
    torch.Tensor.masked_fill = lambda self, mask, value: masked_fill(self, mask.bool(), value)
    torch.manual_seed(0)
    out, lrw, lrw1000 = (os.path.abspath(p) for p in (args.out, args.lrw, args.lrw1000))
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "bigram_freq.pkl"), "wb") as f:       # the LRW decoder module unpickles it at import
            pickle.dump({}, f)
        os.chdir(tmp)
        for name in args.cases:
            beam = len(CASES[name]) > 11
            ref_dir = lrw1000 if beam else lrw
            ref = import_reference(ref_dir)
            sys.path.insert(0, ref_dir)
            (run_beam if beam else run_greedy)(name, ref, out, args.salt)
            sys.path.remove(ref_dir)
        os.chdir(ROOT)


if __name__ == "__main__":
    main()
