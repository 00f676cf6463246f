"""Plain-torch CPU restatement of the LRW1000 beam search (the reference's
VSR_seq2seq_Transformer_with_phonemes_LRW1000/transformer/decoder.py:131-245, "LRW1000/" below) on the primitives of
tests/seq2seq_oracle.py, used by the tests only and pinned to tests/golden/beam_*.npz (written from the reference itself by
tools/make_beam_goldens.py) by test_beam_cpu.py.

Per clip, with W = beam_size: one hypothesis [sos] of score 0; at step i < maxlen every live hypothesis offers
score + log_softmax(logits) + log_prior[last token] (fp32) for every class, the best W of the clip's candidates are kept
(the reference's per-hypothesis top-W followed by a stable sort truncated to W is the same set and order, except at exact
ties), at the last step every kept hypothesis gets an <eos> appended at no score (one that ends in <eos> too), the kept ones
that end in <eos> move to the ended list in kept order, and the ended list, stably sorted by score, is cut to nbest.
Exact ties, which the reference leaves to torch.topk: lower parent slot first, then lower token id.  A candidate of score
-inf is never kept (the reference would carry it along behind every finite one).

A kept hypothesis of rank r lives in SLOT r of its clip at the next step (ended ones leave their slot empty), so "parent" in
the history is the rank the parent had one step earlier.  Flags: 0 nothing kept at this rank, 1 live, 2 ended."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from conftest import load_golden
from oracle import sbl_oracle as O
import seq2seq_oracle as S

CASES = ("beam_small", "beam_varied", "beam_varied_len5", "beam_full")
# one unseen salt per fixture shape for the GPU tests (weights AND clips are re-drawn); test_beam_cpu.py checks that each
# meets the margin floor, so no GPU case is ever skipped.  Picked on the CPU like the fixtures' own salts.
UNSEEN_SALTS = {"beam_small": 41, "beam_varied": 501, "beam_full": 51}
SCORE_TOL_PER_STEP = 1e-3          # the project's logit tolerance, once per accumulated step


def score_tol(maxlen):
    return SCORE_TOL_PER_STEP * maxlen


def margin_floor(maxlen):
    """Token comparisons are exact and leave nothing out, so every decision gap has to be 10x the score tolerance."""
    return 10 * score_tol(maxlen)


def make_freq(V, salt, eos_id=1, eos_rows=3, eos_boost=4.0, power=6.0):
    """A synthetic bigram-frequency table (the reference ships none): about half of the entries are zero (log -> -inf),
    the others are spread over several units of log-frequency (u ** power: the prior then tells permutations of the same
    tokens apart, which a randomly filled decoder barely does), and every eos_rows-th row is eos-heavy, so that hypotheses
    end before the last step.  fp32 (V, V), rows sum to 1."""
    from sbl_for_multilingual_lip_reading_amd import detfill
    u = detfill.uniform("bigram", (V, V), salt).astype(np.float64)
    f = np.where(u > 0, u ** power, 0.0)
    f[::eos_rows, eos_id] = eos_boost
    f[:, 0] = 0.0                                     # nothing is followed by <sos>
    return (f / f.sum(1, keepdims=True)).astype(np.float32)


def beam_clip(sd, enc, n_layers, scale, W, nbest, maxlen, log_prior, sos_id=0, eos_id=1):
    """enc (T, 512) of one clip -> dict(nbest=[(score, yseq list)], tok/par/score/flag (maxlen, W), margin)."""
    emb, prj = sd["decoder.tgt_word_emb.weight"], sd["decoder.tgt_word_prj.weight"]
    V = emb.size(0)
    live = [(0, torch.zeros((), dtype=torch.float32), [sos_id])]          # (slot, score, yseq)
    ended = []
    h_tok = np.full((maxlen, W), eos_id, dtype=np.int32)
    h_par = np.tile(np.arange(W, dtype=np.int32), (maxlen, 1))
    h_score = np.full((maxlen, W), -np.inf, dtype=np.float32)
    h_flag = np.zeros((maxlen, W), dtype=np.int32)
    margin = math.inf
    for i in range(maxlen):
        if not live:
            continue
        ys = torch.tensor([y for _, _, y in live], dtype=torch.long)
        n, L = ys.shape
        x = emb[ys] * scale + O.positional_encoding(L).unsqueeze(0)
        causal = torch.ones(L, L, dtype=torch.bool).triu(1).unsqueeze(0).expand(n, -1, -1)
        x = S._layers(sd, x, enc.unsqueeze(0).expand(n, -1, -1), n_layers, causal, None, None)
        local = F.log_softmax(F.linear(x[:, -1], prj), dim=1)
        if log_prior is not None:
            local = local + log_prior[ys[:, -1]]
        cand = torch.stack([sc for _, sc, _ in live]).unsqueeze(1) + local          # (n, V) fp32
        flat = [(float(cand[a, v]), live[a][0], v, a) for a in range(n) for v in range(V) if float(cand[a, v]) > -math.inf]
        flat.sort(key=lambda c: (-c[0], c[1], c[2]))
        kept = flat[:W]
        for a, b in zip(flat[:W], flat[1:W + 1]):          # adjacent kept ranks, and rank W against rank W + 1
            margin = min(margin, a[0] - b[0])
        nxt = []
        for r, (_, slot, v, a) in enumerate(kept):
            sc, yseq = cand[a, v], live[a][2] + [v]
            if i == maxlen - 1:
                yseq = yseq + [eos_id]
            end = yseq[-1] == eos_id
            h_tok[i, r], h_par[i, r], h_score[i, r], h_flag[i, r] = v, slot, float(sc), 2 if end else 1
            (ended if end else nxt).append((r, sc, yseq))
        live = nxt
    order = sorted(ended, key=lambda e: -float(e[1]))          # stable
    for a, b in zip(order[:nbest], order[1:nbest + 1]):       # adjacent final ranks, and rank nbest against the next one
        margin = min(margin, float(a[1]) - float(b[1]))
    return dict(nbest=[(float(sc), y) for _, sc, y in order[:nbest]], tok=h_tok, par=h_par, score=h_score, flag=h_flag,
                margin=margin, n_ended=len(ended), early=sum(1 for _, _, y in ended if len(y) < maxlen + 2),
                min_live=int((h_flag == 1).sum(1)[:-1].min()) if maxlen > 1 else W)


def pack(clips, nbest, maxlen, eos_id=1):
    """The device's result layout from beam_clip's dicts: yseq (N, nbest, maxlen+2), lengths, scores, n_hyps + history."""
    N = len(clips)
    yseq = np.full((N, nbest, maxlen + 2), eos_id, dtype=np.int64)
    lengths = np.zeros((N, nbest), dtype=np.int32)
    scores = np.full((N, nbest), -np.inf, dtype=np.float32)
    n_hyps = np.zeros(N, dtype=np.int32)
    for n, c in enumerate(clips):
        n_hyps[n] = len(c["nbest"])
        for k, (sc, y) in enumerate(c["nbest"]):
            yseq[n, k, :len(y)], lengths[n, k], scores[n, k] = y, len(y), sc
    out = dict(yseq=yseq, lengths=lengths, scores=scores, n_hyps=n_hyps, margin=min(c["margin"] for c in clips))
    for k in ("tok", "par", "score", "flag"):
        out["hist_" + k] = np.stack([c[k] for c in clips])
    for k in ("n_ended", "early", "min_live"):
        out[k] = np.array([c[k] for c in clips])
    return out


def beam_search(sd, enc, n_layers, scale, W, nbest, maxlen=0, log_prior=None, sos_id=0, eos_id=1):
    maxlen = maxlen or enc.size(1)
    with torch.no_grad():
        return pack([beam_clip(sd, e, n_layers, scale, W, nbest, maxlen, log_prior, sos_id, eos_id) for e in enc], nbest, maxlen, eos_id)


# --------------------------------------------------------------------------- fixtures
def beam_config(g):
    """meta is seq2seq_oracle.case_config's; beam = (beam_size, nbest, decode_max_len)."""
    c = S.case_config(g)
    W, nbest, dml = (int(v) for v in g["beam"])
    c.update(W=W, nbest=nbest, decode_max_len=dml, maxlen=dml or c["T"])
    return c


def log_prior(g):
    """The (V, V) fp32 table the reference forms with torch.log(torch.from_numpy(freq)).float(), or None."""
    return torch.log(torch.from_numpy(np.asarray(g["freq"]))).float() if "freq" in g else None


def with_salt(g, salt):
    """The fixture's shape and gains with other weights and clips."""
    d = {k: g[k] for k in ("meta", "gains", "keys", "shapes", "beam")}
    if "freq" in g:
        d["freq"] = g["freq"]
    d["meta"] = np.array(list(g["meta"][:8]) + [salt], dtype=np.int64)
    return d


@functools.lru_cache(maxsize=None)
def oracle_case(case, salt=None):
    """(fixture or its re-salted view, oracle result), computed once per process."""
    g = load_golden(case + ".npz")
    if salt is not None:
        g = with_salt(g, salt)
    c = beam_config(g)
    sd = S.case_state(g)
    with torch.no_grad():
        enc = S.encode(sd, case_clips(g), c["ne"], training=False)
    return g, beam_search(sd, enc, c["nd"], c["scale"], c["W"], c["nbest"], c["decode_max_len"], log_prior(g))


def case_clips(g):
    from sbl_for_multilingual_lip_reading_amd import detfill
    c = S.case_config(g)
    return torch.from_numpy(detfill.normal("clips", (c["B"], c["T"], c["H"], c["W"]), c["salt"]))


def first_divergence(got, ref):
    """'(clip n, step i)' of the first history entry where the kept tokens / parents / flags differ, for assert messages."""
    for i in range(ref["hist_tok"].shape[1]):
        for n in range(ref["hist_tok"].shape[0]):
            for k in ("tok", "par", "flag"):
                a, b = np.asarray(got["hist_" + k][n, i]), ref["hist_" + k][n, i]
                live = ref["hist_flag"][n, i] != 0
                if not np.array_equal(np.where(live, a, 0), np.where(live, b, 0)) or (k == "flag" and not np.array_equal(a, b)):
                    return "first divergence at (clip %d, step %d): %s got %s, expected %s; scores got %s, expected %s" % (
                        n, i, k, a.tolist(), b.tolist(), np.asarray(got["hist_score"][n, i]).tolist(), ref["hist_score"][n, i].tolist())
    return "the histories agree"
