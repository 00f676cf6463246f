"""Plain-torch restatement of the beam search of the bidirectional SBL decoder (Decoder.beam_search, csrc/pair_beam.hip) on
the primitives of oracle.sbl_oracle: decoder_layer, sbl_fusion, mha_project_kv, positional_encoding.

(a) pair_beam(sd, enc, n_layers, W): the search, exhaustive over the V x V candidates of every live slot.
(b) follow(history, sd, enc, n_layers, W): a checker that needs no decision margin.  Adjacent candidates of a decision lie
    about 1e-3 apart on synthetic weights, closer than fp32 GPU and CPU logits agree, so the tokens of two correct searches
    may differ.  follow therefore rebuilds the prefixes that the given history kept, recomputes every candidate of THAT state
    and checks, with tol_i = 2 * 1e-3 * (i + 1) (the project's logit tolerance, once per direction and step):
      * the kept pairs of a clip are distinct;
      * the totals do not rise with the rank (within tol_i);
      * every reported score is within tol_i of the oracle's score of the same candidate along the same path;
      * no kept candidate's oracle score is below the oracle's W-th best of the state by more than 2 * tol_i.
    It raises AssertionError naming the first (clip, step, rank) that fails.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import sbl_oracle as O

MAXLEN = O.MAXLEN
LOGIT_TOL = 1e-3
NEG = float("-inf")


def step_tol(i):
    return 2 * LOGIT_TOL * (i + 1)


def decoder_names(n_layers, prefix="decoder"):
    return {d: ["%s.layer_first_%s" % (prefix, d)] + ["%s.layer_stack_%s.%d" % (prefix, d, n) for n in range(n_layers - 1)]
            for d in ("l2r", "r2l")}


def hoist_kv(sd, enc, n_layers, prefix="decoder"):
    names = decoder_names(n_layers, prefix)
    return {d: [O.mha_project_kv(sd, p + ".enc_attn", enc) for p in names[d]] for d in names}


def stage_logprobs(sd, kv, clip, ys_l, ys_r, n_layers, n_head=8, prefix="decoder"):
    """One step of the decoder on S pairs: ys_l / ys_r (S, L) prefixes, clip (S,) the clip of every pair (its rows of the
    hoisted K/V).  Returns (lpL, lpR) (S, V): log_softmax of the two heads at the last position, as _decoder_steps feeds them."""
    names = decoder_names(n_layers, prefix)
    emb = sd[prefix + ".tgt_word_emb.weight"]
    S, L = ys_l.shape
    pe = O.positional_encoding(MAXLEN + 1, emb.size(1))
    causal = torch.triu(torch.ones(L, L, dtype=torch.bool), diagonal=1).unsqueeze(0).expand(S, -1, -1)
    a = F.embedding(ys_l, emb) + pe[:L].unsqueeze(0)
    b = F.embedding(ys_r, emb) + pe[:L].unsqueeze(0)
    for n in range(n_layers):
        m = causal if n == 0 else None
        a = O.decoder_layer(sd, names["l2r"][n], a, None, m, tuple(t[clip] for t in kv["l2r"][n]), n_head)
        b = O.decoder_layer(sd, names["r2l"][n], b, None, m, tuple(t[clip] for t in kv["r2l"][n]), n_head)
        a, b = O.sbl_fusion(a, b)
    lp_l = torch.log_softmax(F.linear(a[:, -1], sd[prefix + ".tgt_word_prj_l2r.weight"]), -1)
    lp_r = torch.log_softmax(F.linear(b[:, -1], sd[prefix + ".tgt_word_prj_r2l.weight"]), -1)
    return lp_l, lp_r


def _ranks(lp):
    """rank of every class in the ordering (log-prob descending, token id ascending); lp (V,) numpy"""
    order = np.argsort(-lp, kind="stable")
    r = np.empty_like(order)
    r[order] = np.arange(len(lp))
    return r


def candidates(score, lp_l, lp_r):
    """All candidates of one clip's state: score (W,) fp32, lp_l / lp_r (W, V) fp32 numpy.  Returns (total (W, V, V) fp32 =
    score[s] + (lpL[s][a] + lpR[s][b]) added in fp32 in that order, order = the flat indices of the finite ones, sorted by
    (total descending, s, rank of a, rank of b))."""
    W, V = lp_l.shape
    total = (score[:, None, None] + (lp_l[:, :, None] + lp_r[:, None, :])).astype(np.float32)
    total[~(total > NEG)] = NEG
    ra = np.stack([_ranks(lp_l[s]) for s in range(W)])
    rb = np.stack([_ranks(lp_r[s]) for s in range(W)])
    s_i, a_i, b_i = np.meshgrid(np.arange(W), np.arange(V), np.arange(V), indexing="ij")
    keys = (rb[s_i, b_i].ravel(), ra[s_i, a_i].ravel(), s_i.ravel(), -total.ravel().astype(np.float64))
    order = np.lexsort(keys)
    return total, order[total.ravel()[order] > NEG]


def pair_beam(sd, enc, n_layers, W, n_head=8, sos=0, eos=1):
    """The search of Decoder.beam_search.  Returns a dict of numpy arrays: tok_l / tok_r / par (N, 16, W) int, score (N, 16, W)
    fp32 (the history), ys_l2r / ys_r2l (N, W, 17), scores (N, W), scores_dir (N, W, 2), and gap = the smallest difference
    between the W-th and the (W+1)-th total of any decision."""
    N = enc.size(0)
    with torch.no_grad():
        kv = hoist_kv(sd, enc, n_layers)
        clip = torch.arange(N).repeat_interleave(W)
        ys = [torch.full((N * W, 1), sos, dtype=torch.long) for _ in (0, 1)]
        score = np.full((N, W), NEG, np.float32)
        score[:, 0] = 0.0
        sdir = np.full((N, W, 2), NEG, np.float32)
        sdir[:, 0] = 0.0
        out = dict(tok_l=np.full((N, MAXLEN, W), eos), tok_r=np.full((N, MAXLEN, W), eos), par=np.zeros((N, MAXLEN, W), int),
                   score=np.full((N, MAXLEN, W), NEG, np.float32), gap=np.inf)
        for i in range(MAXLEN):
            lp_l, lp_r = (t.numpy().reshape(N, W, -1) for t in stage_logprobs(sd, kv, clip, ys[0], ys[1], n_layers, n_head))
            V = lp_l.shape[-1]
            new = [torch.full((N * W, i + 2), eos, dtype=torch.long) for _ in (0, 1)]
            nscore, ndir = np.full_like(score, NEG), np.full_like(sdir, NEG)
            for n in range(N):
                total, order = candidates(score[n], lp_l[n], lp_r[n])
                flat = total.ravel()
                if len(order) > W:
                    out["gap"] = min(out["gap"], float(flat[order[W - 1]]) - float(flat[order[W]]))
                for r in range(W):
                    par, a, b = (r, eos, eos) if r >= len(order) else np.unravel_index(order[r], (W, V, V))
                    if r < len(order):
                        nscore[n, r] = flat[order[r]]
                        ndir[n, r] = (np.float32(sdir[n, par, 0] + lp_l[n, par, a]), np.float32(sdir[n, par, 1] + lp_r[n, par, b]))
                    out["tok_l"][n, i, r], out["tok_r"][n, i, r], out["par"][n, i, r] = a, b, par
                    out["score"][n, i, r] = nscore[n, r]
                    for d, t in ((0, a), (1, b)):
                        new[d][n * W + r, :i + 1] = ys[d][n * W + par]
                        new[d][n * W + r, i + 1] = int(t)
            ys, score, sdir = new, nscore, ndir
    out.update(ys_l2r=ys[0].numpy().reshape(N, W, -1), ys_r2l=ys[1].numpy().reshape(N, W, -1), scores=score, scores_dir=sdir)
    return out


def follow(history, sd, enc, n_layers, W, n_head=8, sos=0, eos=1):
    """history = (tok_l, tok_r, par, score), each (N, 16, W) (numpy or tensors): see the module docstring.  Returns
    dict(max_dscore = the largest |reported - oracle| score, max_deficit = the largest amount by which a kept candidate's
    oracle score lies below the oracle's W-th best, ys_l2r / ys_r2l (N, W, 17) = the prefixes the history spells)."""
    tok_l, tok_r, par, rep = (np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in history)
    N = enc.size(0)
    assert tok_l.shape == tok_r.shape == par.shape == rep.shape == (N, MAXLEN, W), (tok_l.shape, (N, MAXLEN, W))
    stats = dict(max_dscore=0.0, max_deficit=0.0)
    with torch.no_grad():
        kv = hoist_kv(sd, enc, n_layers)
        clip = torch.arange(N).repeat_interleave(W)
        ys = [torch.full((N * W, 1), sos, dtype=torch.long) for _ in (0, 1)]
        score = np.full((N, W), NEG, np.float32)      # the ORACLE's score of the followed path in every slot
        score[:, 0] = 0.0
        for i in range(MAXLEN):
            tol = step_tol(i)
            lp_l, lp_r = (t.numpy().reshape(N, W, -1) for t in stage_logprobs(sd, kv, clip, ys[0], ys[1], n_layers, n_head))
            V = lp_l.shape[-1]
            new = [torch.full((N * W, i + 2), eos, dtype=torch.long) for _ in (0, 1)]
            nscore = np.full_like(score, NEG)
            for n in range(N):
                total, order = candidates(score[n], lp_l[n], lp_r[n])
                flat = total.ravel()
                n_keep = min(W, len(order))
                kept = [r for r in range(W) if rep[n, i, r] > NEG]
                at = lambda r: "clip %d step %d rank %d" % (n, i, r)      # noqa: E731
                assert kept == list(range(n_keep)), "%s: ranks %s are kept, the state has %d finite candidates" % (at(0), kept, len(order))
                wth = float(flat[order[n_keep - 1]]) if n_keep else NEG
                seen = set()
                for r in kept:
                    p, a, b = int(par[n, i, r]), int(tok_l[n, i, r]), int(tok_r[n, i, r])
                    assert 0 <= p < W and 0 <= a < V and 0 <= b < V, "%s: parent %d, tokens %d / %d out of range" % (at(r), p, a, b)
                    assert score[n, p] > NEG, "%s: parent slot %d is dead" % (at(r), p)
                    assert (p, a, b) not in seen, "%s: candidate (%d, %d, %d) is kept twice" % (at(r), p, a, b)
                    seen.add((p, a, b))
                    mine = float(total[p, a, b])
                    d = abs(float(rep[n, i, r]) - mine)
                    stats["max_dscore"] = max(stats["max_dscore"], d)
                    assert d <= tol, "%s: reported score %.6f, the oracle's score of that candidate %.6f (tol %.0e)" % (
                        at(r), rep[n, i, r], mine, tol)
                    assert r == 0 or rep[n, i, r] <= rep[n, i, r - 1] + tol, "%s: total %.6f above rank %d's %.6f" % (
                        at(r), rep[n, i, r], r - 1, rep[n, i, r - 1])
                    stats["max_deficit"] = max(stats["max_deficit"], wth - mine)
                    assert mine >= wth - 2 * tol, "%s: the oracle scores the kept candidate %.6f, its W-th best is %.6f (2 tol %.0e)" % (
                        at(r), mine, wth, 2 * tol)
                    nscore[n, r] = total[p, a, b]
                    for dd, t in ((0, a), (1, b)):
                        new[dd][n * W + r, :i + 1] = ys[dd][n * W + p]
                        new[dd][n * W + r, i + 1] = t
            ys, score = new, nscore
    stats.update(ys_l2r=ys[0].numpy().reshape(N, W, -1), ys_r2l=ys[1].numpy().reshape(N, W, -1))
    return stats


def decoder_state_dict(n_layers, salt, gains="varied"):
    """The decoder.* entries of the oracle state dict of an n_layers decoder, filled as O.make_state_dict fills them."""
    from sbl_for_multilingual_lip_reading_amd import detfill
    shapes = {k: v for k, v in O.state_dict_shapes(1, n_layers).items() if k.startswith("decoder.")}
    return {k: torch.from_numpy(v.copy()) for k, v in detfill.fill_state_dict(shapes, salt, gains).items()}


def encoder_output(N, T, salt):
    """A synthetic (N, T, 512) encoder output of LayerNorm scale."""
    gen = torch.Generator().manual_seed(9000 + salt)
    return torch.randn(N, T, 512, generator=gen)
