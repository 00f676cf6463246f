"""Plain-torch CPU restatement of ragged clips in the single-direction baseline, used by the tests only and
pinned to tests/golden/ragged_s2s_*.npz (written from the reference itself by tools/make_ragged_s2s_goldens.py) by
test_ragged_s2s_cpu.py.  The oracle: clip n of a padded batch decodes as the reference decodes it ALONE, cut to its first
l_n frames - so everything here runs clip by clip on the cut clip with the primitives of seq2seq_oracle.py / beam_oracle.py
and packs the results into the layout of the batched call: T = the padded length, eos / -inf / flag 0 behind a clip's end."""
import functools

import numpy as np
import torch

import beam_oracle as B
import seq2seq_oracle as S
from conftest import load_golden

CASES = ("ragged_s2s_small", "ragged_s2s_beam")
MIN_MARGIN = 10 * 1e-3            # greedy: 10x the project's logit tolerance
# one unseen salt per fixture for the GPU tests (weights AND clips re-drawn); test_ragged_s2s_cpu.py shows that each meets its
# margin floor, so no GPU case is ever skipped.  Picked on the CPU like the fixtures' own salts.
UNSEEN_SALTS = {"ragged_s2s_small": 31, "ragged_s2s_beam": 1352}


def clips(c, lengths):
    """(B, T, H, W) float32 clips whose frames t >= lengths[n] are all zero (what the loader pads with)."""
    from sbl_for_multilingual_lip_reading_amd import detfill
    x = detfill.normal("clips", (c["B"], c["T"], c["H"], c["W"]), c["salt"])
    for n, l in enumerate(lengths):
        x[n, l:] = 0.0
    return torch.from_numpy(x)


def encode_cut(sd, x, lengths, ne):
    """Every clip alone, cut to its length -> (B, T, 512) with zero rows behind the length."""
    enc = torch.zeros(x.size(0), x.size(1), 512)
    for n, l in enumerate(lengths):
        enc[n, :l] = S.encode(sd, x[n:n + 1, :l], ne, training=False)[0]
    return enc


def greedy(sd, enc, lengths, nd, scale, eos_id=1):
    """Per clip S.recognize_beam on the cut rows -> tokens (B, T+1) eos behind l_n, logits (B, T, V) zero behind, margins
    (B, T) +inf behind."""
    Bn, T, _ = enc.shape
    V = sd["decoder.tgt_word_prj.weight"].size(0)
    tokens = np.full((Bn, T + 1), eos_id, dtype=np.int64)
    logits = np.zeros((Bn, T, V), dtype=np.float32)
    margins = np.full((Bn, T), np.inf, dtype=np.float32)
    for n, l in enumerate(lengths):
        ys, lg = S.recognize_beam(sd, enc[n:n + 1, :l], nd, scale)
        tokens[n, :l + 1], logits[n, :l] = ys[0].numpy(), lg[0].numpy()
        top2 = lg[0].topk(2, dim=-1).values
        margins[n, :l] = (top2[:, 0] - top2[:, 1]).numpy()
    return tokens, logits, margins


def beam(sd, enc, lengths, nd, scale, W, nbest, log_prior, eos_id=1):
    """Per clip B.beam_clip(..., maxlen = l_n) on the cut rows, packed for maxlen = T: a hypothesis that ended at the clip's
    last step has length l_n + 2; history rows behind l_n: token eos, parent = rank, score -inf, flag 0."""
    T = enc.size(1)
    per = [B.beam_clip(sd, enc[n, :l], nd, scale, W, nbest, l, log_prior, eos_id=eos_id) for n, l in enumerate(lengths)]
    for c, l in zip(per, lengths):
        pad = T - l
        c["tok"] = np.concatenate([c["tok"], np.full((pad, W), eos_id, dtype=np.int32)])
        c["par"] = np.concatenate([c["par"], np.tile(np.arange(W, dtype=np.int32), (pad, 1))])
        c["score"] = np.concatenate([c["score"], np.full((pad, W), -np.inf, dtype=np.float32)])
        c["flag"] = np.concatenate([c["flag"], np.zeros((pad, W), dtype=np.int32)])
    return B.pack(per, nbest, T, eos_id)      # "margin": the smallest decision gap of any clip; floor B.margin_floor(T)


def config(g):
    c = S.case_config(g)
    c["lengths"] = tuple(int(l) for l in g["lengths"])
    if "beam" in g:
        W, nbest, dml = (int(v) for v in g["beam"])
        c.update(beam_size=W, nbest=nbest, decode_max_len=dml)      # (c["W"] stays the frame width)
    return c


def with_salt(g, salt):
    d = {k: g[k] for k in ("meta", "gains", "keys", "shapes", "lengths") if k in g}
    for k in ("beam", "freq"):
        if k in g:
            d[k] = g[k]
    d["meta"] = np.array(list(g["meta"][:8]) + [salt], dtype=np.int64)
    return d


@functools.lru_cache(maxsize=None)
def oracle_case(case, salt=None):
    """(fixture or its re-salted view, clips, dict of the restatement's results), computed once per process."""
    g = load_golden(case + ".npz")
    if salt is not None:
        g = with_salt(g, salt)
    c = config(g)
    sd = S.case_state(g)
    x = clips(c, c["lengths"])
    with torch.no_grad():
        enc = encode_cut(sd, x, c["lengths"], c["ne"])
        if "beam" in g:
            o = beam(sd, enc, c["lengths"], c["nd"], c["scale"], c["beam_size"], c["nbest"], B.log_prior(g))
        else:
            tokens, logits, margins = greedy(sd, enc, c["lengths"], c["nd"], c["scale"])
            o = dict(tokens=tokens, logits=logits, margins=margins)
    o["enc"] = enc.numpy()
    return g, x, o
