#!/usr/bin/env python3
"""Writes tests/golden/ragged_*.npz: what the REFERENCE SBL model (its SBL_Multilingual_Lip_reading/ package, imported at
generation time from --reference) decodes for every clip of a ragged batch when the clip is given to it ALONE, cut to its
own frame count - the oracle of Transformer.recognize(x, input_lengths).

    python tools/make_ragged_goldens.py --reference /path/to/SBL_Multilingual_Lip_reading

The model is filled with detfill weights (as the recognize_varied fixture is; the gains boost the token embedding and the
cross-attention output projection, so that the greedy tokens depend on the clip and on how many of its frames are attended
to), every dropout is switched off (parity mode) and the model is in eval mode (BatchNorm running statistics: a clip's
features do not depend on its batch).  Per clip n of length l the file holds the encoder output rows < l (rows >= l zero), the
logits of every greedy step and direction, the tokens and every step's top-2 margin, next to the full padded clips (frames
>= l all zero, what the loader pads with) and the lengths.

Token comparisons in the tests are exact and exclude no rows; that is sound only when no arg-max is a near tie, so the
script asserts that the smallest top-2 margin of every case is at least 10x the project's 1e-3 logit tolerance, that no two
clips decode alike, and that the padded batch decoded at full length gives other tokens for a short clip.  A case that fails an assert gets another salt."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sbl_for_multilingual_lip_reading_amd import detfill  # noqa: E402
from oracle.make_goldens import det_load, neutralise_dropout  # noqa: E402

MIN_MARGIN = 10 * 1e-3
GAINS = '{"tgt_word_emb": 30.0, "enc_attn.fc.weight": 6.0, "slf_attn.fc.weight": 0.3, "w_2.weight": 0.3}'
# name: (encoder layers, decoder layers (per direction), B, T, H, W, lengths, salt)
CASES = {
    "ragged_small": (1, 1, 4, 8, 32, 32, (8, 5, 1, 3), 23),
    "ragged_full": (6, 6, 3, 8, 32, 32, (8, 2, 6), 13),
}


def clips(B, T, H, W, lengths, salt):
    """(B, T, H, W) float32 clips whose frames t >= lengths[n] are all zero."""
    x = detfill.normal("clips", (B, T, H, W), salt)
    for n, l in enumerate(lengths):
        x[n, l:] = 0.0
    return x


def run_case(name, ref, out_dir):
    ne, nd, B, T, H, W, lengths, salt = CASES[name]
    model = ref["Transformer"](ref["Encoder"](512, ne, 8, 64, 64, 512, 2048), ref["Decoder"](0, 1, 58, 512, nd, 8, 64, 64, 512, 2048), None)
    neutralise_dropout(model)
    det_load(model, salt, json.loads(GAINS))
    model.eval()
    x = clips(B, T, H, W, lengths, salt)
    grabbed = {}
    model.encoder.register_forward_hook(lambda m, i, o: grabbed.__setitem__("enc", o[0].detach().clone()))
    model.decoder.tgt_word_prj_l2r.register_forward_hook(lambda m, i, o: grabbed["l2r"].append(o.detach().clone()))
    model.decoder.tgt_word_prj_r2l.register_forward_hook(lambda m, i, o: grabbed["r2l"].append(o.detach().clone()))
    enc = np.zeros((B, T, 512), dtype=np.float32)
    logits = np.zeros((B, 2, 16, 58), dtype=np.float32)
    tokens = np.zeros((B, 2, 17), dtype=np.int64)
    for n, l in enumerate(lengths):
        grabbed["l2r"], grabbed["r2l"] = [], []
        with torch.no_grad():
            ys_l, ys_r = model.recognize(torch.from_numpy(x[n:n + 1, :l].copy()))      # the clip alone, cut to its length
        assert grabbed["enc"].shape == (1, l, 512) and len(grabbed["l2r"]) == 16 and len(grabbed["r2l"]) == 16
        enc[n, :l] = grabbed["enc"][0].numpy()
        logits[n, 0] = torch.cat(grabbed["l2r"], 0).numpy()
        logits[n, 1] = torch.cat(grabbed["r2l"], 0).numpy()
        tokens[n, 0], tokens[n, 1] = ys_l[0].numpy(), ys_r[0].numpy()
    top2 = np.sort(logits, -1)[..., -2:]
    margins = (top2[..., 1] - top2[..., 0]).astype(np.float32)                             # (B, 2, 16)
    assert np.array_equal(logits.argmax(-1), tokens[:, :, 1:])
    assert margins.min() >= MIN_MARGIN, (name, float(margins.min()))
    assert len({tuple(t.reshape(-1).tolist()) for t in tokens}) == B, (name, "two clips decode alike")
    # what the padded batch decodes to when the padding is attended to (all lengths T): it must differ for a short clip, or the
    # fixture could not tell a decode that ignores the lengths from one that honours them
    with torch.no_grad():
        pad_l, pad_r = model.recognize(torch.from_numpy(x))
    padded = np.stack([pad_l.numpy(), pad_r.numpy()], 1)
    assert any(l < T and not np.array_equal(padded[n], tokens[n]) for n, l in enumerate(lengths)), (name, "padding changes no tokens")
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, meta=np.array([ne, nd, B, T, H, W, salt], dtype=np.int64), gains=np.array(GAINS),
                        lengths=np.array(lengths, dtype=np.int32), clips=x, enc=enc, logits=logits, tokens=tokens, margins=margins,
                        tokens_padded=padded)
    print("%s: %d bytes, min margin %.4f, tokens l2r %s" % (path, os.path.getsize(path), margins.min(), tokens[:, 0, 1:6].tolist()))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "e2e_varied.npz"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's SBL_Multilingual_Lip_reading directory")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("cases", nargs="*", default=list(CASES))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    for m in [m for m in sys.modules if m == "config" or m.split(".")[0] == "transformer"]:
        del sys.modules[m]
    from transformer.decoder import Decoder
    from transformer.encoder import Encoder
    from transformer.transformer import Transformer
    ref = {"Decoder": Decoder, "Encoder": Encoder, "Transformer": Transformer}
    torch.manual_seed(0)
    for name in args.cases:
        run_case(name, ref, args.out)


if __name__ == "__main__":
    main()
