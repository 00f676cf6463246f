"""Plain Python / torch restatement of the closed-vocabulary word decode (include/sbl_hip.h: sbl_lexicon_shortlist,
sbl_pair_score_tail; Decoder.recognize_words).

(a) strip / lev / distances / shortlist: the definitions, by brute force over every (hypothesis, word).
(b) pair_scores: the pair score of given token rows on tests/sbl_beam_oracle.stage_logprobs, one decoder pass per prefix
    length (no ragged batch, no shared K/V), summed in fp32 in the stated order.
"""
import numpy as np
import torch

import sbl_beam_oracle as PB

WIDTH = 17


def strip(row, sos=0, eos=1, ignore=-1):
    """Entries 1..16 of a 17-wide row, cut before the first eos, without the entries equal to sos or ignore."""
    out = []
    for t in list(row)[1:WIDTH]:
        t = int(t)
        if t == eos:
            break
        if t != sos and t != ignore:
            out.append(t)
    return out


def lev(a, b):
    """Levenshtein distance with unit costs, the textbook table."""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[len(b)]


def distances(p_l, p_r, words):
    """D(w) = lev(p_l, w) + lev(p_r, reversed(w)) for every word."""
    return [lev(p_l, w) + lev(p_r, w[::-1]) for w in words]


def distances_table(p_l, p_r, words):
    """distances(...) for a large lexicon: the same table as lev, filled for all words at once (numpy over the words, one
    table per direction, read at every word's own length).  tests/test_lexicon_cpu.py holds it to distances."""
    n = len(words)
    lens = np.array([len(w) for w in words])
    tok = np.full((2, n, 15), -1, np.int64)
    for i, w in enumerate(words):
        tok[0, i, :len(w)], tok[1, i, :len(w)] = w, w[::-1]
    total = np.zeros(n, np.int64)
    for d, p in enumerate((p_l, p_r)):
        prev = np.tile(np.arange(16), (n, 1))
        for i, x in enumerate(p, 1):
            cur = np.empty_like(prev)
            cur[:, 0] = i
            for j in range(1, 16):
                cur[:, j] = np.minimum(np.minimum(prev[:, j] + 1, cur[:, j - 1] + 1), prev[:, j - 1] + (tok[d, :, j - 1] != x))
            prev = cur
        total += prev[np.arange(n), lens]
    return total.tolist()


def shortlist(ys_l2r, ys_r2l, words, K, sos=0, eos=1, ignore=-1):
    """ys_l2r / ys_r2l (N, H, 17) integer arrays, words a list of token lists.  Returns a dict of numpy arrays: cand, cand_dist,
    cand_hyp (N, K) int32, cand_ys_l2r / cand_ys_r2l (N*K, 17) int64, n_pos (N*K) int32."""
    ys_l2r, ys_r2l = np.asarray(ys_l2r), np.asarray(ys_r2l)
    N, H, _ = ys_l2r.shape
    words = [list(w) for w in words]
    out = dict(cand=np.zeros((N, K), np.int32), cand_dist=np.zeros((N, K), np.int32), cand_hyp=np.zeros((N, K), np.int32),
               cand_ys_l2r=np.full((N * K, WIDTH), eos, np.int64), cand_ys_r2l=np.full((N * K, WIDTH), eos, np.int64),
               n_pos=np.zeros(N * K, np.int32))
    for n in range(N):
        dist = distances if len(words) < 2000 else distances_table
        per_h = [dist(strip(ys_l2r[n, h], sos, eos, ignore), strip(ys_r2l[n, h], sos, eos, ignore), words) for h in range(H)]
        keys = sorted(min((per_h[h][w], h) for h in range(H)) + (w,) for w in range(len(words)))
        for r, (d, h, w) in enumerate(keys[:K]):
            s, c = n * K + r, len(words[w])
            out["cand"][n, r], out["cand_dist"][n, r], out["cand_hyp"][n, r] = w, d, h
            out["cand_ys_l2r"][s, 0] = out["cand_ys_r2l"][s, 0] = sos
            out["cand_ys_l2r"][s, 1:c + 1] = words[w]
            out["cand_ys_r2l"][s, 1:c + 1] = words[w][::-1]
            out["n_pos"][s] = c + 1
    return out


def pair_scores(sd, enc, ys_l2r, ys_r2l, n_pos, group, n_layers):
    """sd: the decoder.* oracle state dict, enc (N, T, 512) CPU tensor, ys_* (S, 17) int64 tensors (slot s belongs to clip
    s // group), n_pos (S,) integers or None (16).  Returns numpy fp32: logp (S, 16, 2), score_dir (S, 2), score (S)."""
    S = ys_l2r.size(0)
    n_pos = [PB.MAXLEN] * S if n_pos is None else [int(v) for v in n_pos]
    logp = np.zeros((S, PB.MAXLEN, 2), np.float32)
    with torch.no_grad():
        kv = PB.hoist_kv(sd, enc, n_layers)
        clip = torch.arange(enc.size(0)).repeat_interleave(group)
        for i in range(max(n_pos)):
            lp_l, lp_r = PB.stage_logprobs(sd, kv, clip, ys_l2r[:, :i + 1], ys_r2l[:, :i + 1], n_layers)
            a = lp_l.gather(1, ys_l2r[:, i + 1:i + 2]).squeeze(1).numpy()
            b = lp_r.gather(1, ys_r2l[:, i + 1:i + 2]).squeeze(1).numpy()
            for s in range(S):
                if i < n_pos[s]:
                    logp[s, i] = (a[s], b[s])
    score_dir, score = np.zeros((S, 2), np.float32), np.zeros(S, np.float32)
    for s in range(S):
        for i in range(n_pos[s]):
            score_dir[s] = score_dir[s] + logp[s, i]
            score[s] = np.float32(score[s] + np.float32(logp[s, i, 0] + logp[s, i, 1]))
    return logp, score_dir, score
