"""Plain-torch restatement of the lexicon-constrained pair beam search of the SBL decoder (Decoder.beam_search_lex,
include/sbl_hip.h: sbl_pair_beam_tail_lex) on the primitives of tests/sbl_beam_oracle.py (stage_logprobs, hoist_kv, step_tol).
Used by the tests only.

The pair trie is a plain dict here, built from the STATES of the words - (w[:t], w[c-t:]) - and not from key paths as
Lexicon.pair_trie builds it: nothing is shared with that code, whose tables the tests check against this one.

(a) pair_tables(words): the (begin, key, word) tables the header defines, as lists.
(b) pair_lex_beam(sd, enc, n_layers, words, W): the search.
(c) brute_force(sd, enc, n_layers, words): every word's teacher-forced pair score over its c_w + 1 positions.
(d) follow_lex(history, sd, enc, n_layers, words, W): the margin-free checker in the manner of sbl_beam_oracle.follow.  It
    rebuilds the prefixes and nodes that the given history kept, recomputes every candidate of THAT state and checks, with
    tol_i = step_tol(i):
      * the kept candidates of a clip are distinct;
      * the totals do not rise with the rank (within tol_i);
      * every reported score is within tol_i of the oracle's score of the same candidate along the same path;
      * no kept candidate's oracle score is below the oracle's W-th best of the state by more than 2 * tol_i;
      * every kept (parent, tokens) is an edge of the parent's node and the reported node is that edge's child (an ended
        parent: tokens (eos, eos), the parent's own node).
    It raises AssertionError naming the first (clip, step, rank) that fails.
"""
import numpy as np
import torch

import sbl_beam_oracle as PB

NEG = float("-inf")
ROW = PB.MAXLEN + 1
# six words of 1..5 tokens for the exhaustive searches (W = 8): a word that is a prefix of two others, its reverse, a
# one-token word and a word of repeated tokens
WORDS6 = [[5, 9], [7], [5, 9, 11, 3, 8], [9, 5], [5, 9, 4], [12, 12, 12, 6]]


# --------------------------------------------------------------------------- the pair trie as a dict of states
def _path(prefix, suffix):
    """The key sequence that leads to the state (prefix, suffix) of depth t: step i emits (prefix[i], suffix[t-1-i])."""
    t = len(prefix)
    return tuple(prefix[i] * 64 + suffix[t - 1 - i] for i in range(t))


def dict_pair_trie(words, eos=1):
    """(paths, terminal): paths = the key path of every node - one per distinct state (w[:t], w[c-t:]), t = 0..c, of any word
    and one per distinct word behind (eos, eos) - as a set; terminal = {key path of a word's terminal node: lowest index}."""
    states, terminal = set(), {}
    for i, w in enumerate(words):
        w = tuple(int(t) for t in w)
        c = len(w)
        for t in range(c + 1):
            states.add((w[:t], w[c - t:]))
        terminal.setdefault(_path(w, w) + (eos * 64 + eos,), i)
    paths = {_path(p, s) for p, s in states}
    assert len(paths) == len(states) and not paths & set(terminal)      # a key path names one state; no word holds eos
    return paths | set(terminal), terminal


def pair_tables(words, eos=1):
    """(begin (P + 1), key (P - 1), word (P)) as lists, and index = {key path: node}.  Breadth-first numbering with the
    children of a node in ascending key = the paths sorted by (length, keys): within one depth the parents are in that order
    by induction, and so are their children; hence the child behind CSR entry e is node e + 1."""
    paths, terminal = dict_pair_trie(words, eos)
    order = sorted(paths, key=lambda p: (len(p), p))
    index = {p: k for k, p in enumerate(order)}
    n_child = [0] * len(order)
    for p in order[1:]:
        n_child[index[p[:-1]]] += 1
    begin = [0]
    for c in n_child:
        begin.append(begin[-1] + c)
    return begin, [p[-1] for p in order[1:]], [terminal.get(p, -1) for p in order], index


def children_of(paths):
    kids = {p: [] for p in paths}
    for p in paths:
        if p:
            kids[p[:-1]].append(p[-1])
    return {p: sorted(k) for p, k in kids.items()}


def word_rows(words, sos=0, eos=1):
    """(ys_l2r, ys_r2l) int64 (Wn, 17): sos, w, eos fill and sos, reversed(w), eos fill."""
    rows = [np.full((len(words), ROW), eos, np.int64) for _ in (0, 1)]
    for i, w in enumerate(words):
        rows[0][i, 0] = rows[1][i, 0] = sos
        rows[0][i, 1:len(w) + 1] = w
        rows[1][i, 1:len(w) + 1] = w[::-1]
    return rows


# --------------------------------------------------------------------------- the search
def _candidates(score, lp_l, lp_r, node, kids, terminal, eos):
    """The finite candidates of one clip's state, sorted by (total descending, slot, key): [(total fp32, slot, a, b, child path)]."""
    out = []
    for s in range(len(score)):
        if not score[s] > NEG:
            continue
        if node[s] in terminal:
            out.append((np.float32(score[s]), s, eos, eos, node[s]))
            continue
        for k in kids[node[s]]:
            a, b = k >> 6, k & 63
            t = np.float32(score[s] + np.float32(lp_l[s, a] + lp_r[s, b]))
            if t > NEG:
                out.append((t, s, a, b, node[s] + (k,)))
    return sorted(out, key=lambda c: (-float(c[0]), c[1], c[2] * 64 + c[3]))


def pair_lex_beam(sd, enc, n_layers, words, W, n_head=8, sos=0, eos=1):
    """The search of Decoder.beam_search_lex.  Returns a dict of numpy arrays: tok_l / tok_r / par / node (N, steps, W) int,
    score (N, steps, W) fp32 (the history), ys_l2r / ys_r2l (N, W, 17), scores (N, W), scores_dir (N, W, 2), cand (N, W) =
    the word of every final slot (-1: dead), steps = longest word + 1."""
    N = enc.size(0)
    steps = max(len(w) for w in words) + 1
    paths, terminal = dict_pair_trie(words, eos)
    kids = children_of(paths)
    index = pair_tables(words, eos)[3]
    with torch.no_grad():
        kv = PB.hoist_kv(sd, enc, n_layers)
        clip = torch.arange(N).repeat_interleave(W)
        ys = [torch.full((N * W, 1), sos, dtype=torch.long) for _ in (0, 1)]
        score = np.full((N, W), NEG, np.float32)
        score[:, 0] = 0.0
        sdir = np.full((N, W, 2), NEG, np.float32)
        sdir[:, 0] = 0.0
        node = [[()] * W for _ in range(N)]
        out = dict(tok_l=np.full((N, steps, W), eos), tok_r=np.full((N, steps, W), eos), par=np.zeros((N, steps, W), int),
                   node=np.zeros((N, steps, W), int), score=np.full((N, steps, W), NEG, np.float32), steps=steps)
        for i in range(steps):
            lp_l, lp_r = (t.numpy().reshape(N, W, -1) for t in PB.stage_logprobs(sd, kv, clip, ys[0], ys[1], n_layers, n_head))
            new = [torch.full((N * W, i + 2), eos, dtype=torch.long) for _ in (0, 1)]
            nscore, ndir, nnode = np.full_like(score, NEG), np.full_like(sdir, NEG), [[()] * W for _ in range(N)]
            for n in range(N):
                cands = _candidates(score[n], lp_l[n], lp_r[n], node[n], kids, terminal, eos)
                for r in range(W):
                    par, a, b = r, eos, eos
                    if r < len(cands):
                        t, par, a, b, child = cands[r]
                        ended = node[n][par] in terminal
                        nscore[n, r], nnode[n][r] = t, child
                        ndir[n, r] = sdir[n, par] if ended else (np.float32(sdir[n, par, 0] + lp_l[n, par, a]),
                                                                 np.float32(sdir[n, par, 1] + lp_r[n, par, b]))
                    out["tok_l"][n, i, r], out["tok_r"][n, i, r], out["par"][n, i, r] = a, b, par
                    out["score"][n, i, r], out["node"][n, i, r] = nscore[n, r], index[nnode[n][r]]
                    for d, tok in ((0, a), (1, b)):
                        new[d][n * W + r, :i + 1] = ys[d][n * W + par]
                        new[d][n * W + r, i + 1] = int(tok)
            ys, score, sdir, node = new, nscore, ndir, nnode
    out.update(ys_l2r=_rows17(ys[0], N, W, eos), ys_r2l=_rows17(ys[1], N, W, eos), scores=score, scores_dir=sdir,
               cand=np.array([[terminal.get(node[n][r], -1) if score[n, r] > NEG else -1 for r in range(W)] for n in range(N)]))
    return out


def _rows17(ys, N, W, eos):
    out = np.full((N * W, ROW), eos, np.int64)
    out[:, :ys.size(1)] = ys.numpy()
    return out.reshape(N, W, ROW)


def brute_force(sd, enc, n_layers, words, n_head=8, sos=0, eos=1):
    """(N, Wn) fp32: the teacher-forced pair score of every word for every clip - the sum over its c_w + 1 positions of
    (lpL_i + lpR_i) at the tokens (w[i], w[c-1-i]) and the closing (eos, eos), added in step order in fp32 like the search's
    totals (and like Decoder.score_pairs with n_pos = c_w + 1)."""
    N, Wn = enc.size(0), len(words)
    rows = word_rows(words, sos, eos)
    score = np.zeros((N, Wn), np.float32)
    with torch.no_grad():
        kv = PB.hoist_kv(sd, enc, n_layers)
        for i in range(max(len(w) for w in words) + 1):
            use = [k for k, w in enumerate(words) if len(w) >= i]
            clip = torch.arange(N).repeat_interleave(len(use))
            ys = [torch.from_numpy(rows[d][use, :i + 1]).repeat(N, 1) for d in (0, 1)]
            lp_l, lp_r = (t.numpy().reshape(N, len(use), -1) for t in PB.stage_logprobs(sd, kv, clip, ys[0], ys[1], n_layers, n_head))
            for j, k in enumerate(use):
                a, b = int(rows[0][k, i + 1]), int(rows[1][k, i + 1])
                score[:, k] = score[:, k] + (lp_l[:, j, a] + lp_r[:, j, b]).astype(np.float32)
    return score


def follow_lex(history, sd, enc, n_layers, words, W, n_head=8, sos=0, eos=1):
    """history = (tok_l, tok_r, par, score, node), each (N, steps, W) (numpy or tensors): see the module docstring.  Returns
    dict(max_dscore, max_deficit, ys_l2r / ys_r2l (N, W, 17) = the prefixes the history spells, cand (N, W) = the word of
    every final slot, -1 at a dead one, scores (N, W) = the ORACLE's totals of the followed paths)."""
    tok_l, tok_r, par, rep, rnode = (np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in history)
    N = enc.size(0)
    steps = max(len(w) for w in words) + 1
    assert tok_l.shape == tok_r.shape == par.shape == rep.shape == rnode.shape == (N, steps, W), (tok_l.shape, (N, steps, W))
    paths, terminal = dict_pair_trie(words, eos)
    kids = children_of(paths)
    index = pair_tables(words, eos)[3]
    stats = dict(max_dscore=0.0, max_deficit=0.0)
    with torch.no_grad():
        kv = PB.hoist_kv(sd, enc, n_layers)
        clip = torch.arange(N).repeat_interleave(W)
        ys = [torch.full((N * W, 1), sos, dtype=torch.long) for _ in (0, 1)]
        score = np.full((N, W), NEG, np.float32)      # the ORACLE's score of the followed path in every slot
        score[:, 0] = 0.0
        node = [[()] * W for _ in range(N)]
        for i in range(steps):
            tol = PB.step_tol(i)
            lp_l, lp_r = (t.numpy().reshape(N, W, -1) for t in PB.stage_logprobs(sd, kv, clip, ys[0], ys[1], n_layers, n_head))
            new = [torch.full((N * W, i + 2), eos, dtype=torch.long) for _ in (0, 1)]
            nscore, nnode = np.full_like(score, NEG), [[()] * W for _ in range(N)]
            for n in range(N):
                cands = _candidates(score[n], lp_l[n], lp_r[n], node[n], kids, terminal, eos)
                mine_of = {(c[1], c[2], c[3]): c for c in cands}
                n_keep = min(W, len(cands))
                kept = [r for r in range(W) if rep[n, i, r] > NEG]
                at = lambda r: "clip %d step %d rank %d" % (n, i, r)      # noqa: E731
                assert kept == list(range(n_keep)), "%s: ranks %s are kept, the state has %d finite candidates" % (at(0), kept, len(cands))
                wth = float(cands[n_keep - 1][0]) if n_keep else NEG
                seen = set()
                for r in range(W):
                    p, a, b = int(par[n, i, r]), int(tok_l[n, i, r]), int(tok_r[n, i, r])
                    if r >= n_keep:
                        assert (p, a, b, int(rnode[n, i, r])) == (r, eos, eos, 0), "%s: a dead rank holds (%d, %d, %d), node %d" % (
                            at(r), p, a, b, rnode[n, i, r])
                    else:
                        assert 0 <= p < W and score[n, p] > NEG, "%s: parent slot %d is out of range or dead" % (at(r), p)
                        assert (p, a, b) not in seen, "%s: candidate (%d, %d, %d) is kept twice" % (at(r), p, a, b)
                        seen.add((p, a, b))
                        if node[n][p] in terminal:
                            assert (a, b) == (eos, eos), "%s: the ended parent %d goes on with (%d, %d)" % (at(r), p, a, b)
                            child = node[n][p]
                        else:
                            assert a * 64 + b in kids[node[n][p]], "%s: (%d, %d) is no edge of the node of parent %d" % (at(r), a, b, p)
                            child = node[n][p] + (a * 64 + b,)
                        assert int(rnode[n, i, r]) == index[child], "%s: reported node %d, the edge's child is %d" % (
                            at(r), rnode[n, i, r], index[child])
                        assert (p, a, b) in mine_of, "%s: the oracle scores candidate (%d, %d, %d) -inf" % (at(r), p, a, b)
                        mine = float(mine_of[p, a, b][0])
                        d = abs(float(rep[n, i, r]) - mine)
                        stats["max_dscore"] = max(stats["max_dscore"], d)
                        assert d <= tol, "%s: reported score %.6f, the oracle's score of that candidate %.6f (tol %.0e)" % (
                            at(r), rep[n, i, r], mine, tol)
                        assert r == 0 or rep[n, i, r] <= rep[n, i, r - 1] + tol, "%s: total %.6f above rank %d's %.6f" % (
                            at(r), rep[n, i, r], r - 1, rep[n, i, r - 1])
                        stats["max_deficit"] = max(stats["max_deficit"], wth - mine)
                        assert mine >= wth - 2 * tol, "%s: the oracle scores the kept candidate %.6f, its W-th best is %.6f (2 tol %.0e)" % (
                            at(r), mine, wth, 2 * tol)
                        nscore[n, r], nnode[n][r] = mine_of[p, a, b][0], child
                    for dd, t in ((0, a), (1, b)):
                        new[dd][n * W + r, :i + 1] = ys[dd][n * W + p]
                        new[dd][n * W + r, i + 1] = t
            ys, score, node = new, nscore, nnode
    stats.update(ys_l2r=_rows17(ys[0], N, W, eos), ys_r2l=_rows17(ys[1], N, W, eos), scores=score,
                 cand=np.array([[terminal.get(node[n][r], -1) if score[n, r] > NEG else -1 for r in range(W)] for n in range(N)]))
    return stats
