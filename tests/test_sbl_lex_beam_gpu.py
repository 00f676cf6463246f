"""GPU checks of the lexicon-constrained pair beam search of the SBL decoder (csrc/pair_beam.hip: sbl_pair_beam_tail_lex,
Lexicon.pair_trie, Decoder.beam_search_lex, Transformer.validate_words_lex): the tail kernel alone against a float64
restatement on planted tables, its tie order, tables that point out of range, the whole search against the plain-torch
checker (tests/sbl_lex_beam_oracle.py: follow_lex) and against Decoder.score_pairs, an exhaustive search, a one-word lexicon,
the validation call with its meter under one hipGraph, and the argument errors."""
import numpy as np
import pytest
import torch

import lex_beam_oracle as LB
import sbl_beam_oracle as PB
import sbl_lex_beam_oracle as PL
from sbl_for_multilingual_lip_reading_amd import detfill

pytestmark = pytest.mark.gpu
NEG = float("-inf")
DEV = "cuda:0"
V, SOS, EOS = 58, 0, 1


@pytest.fixture(params=["f32", "bf16x6"])
def precision(request):
    from sbl_for_multilingual_lip_reading_amd import ops
    ops.set_matmul_precision(request.param)
    yield request.param
    ops.set_matmul_precision("f32")


# --------------------------------------------------------------------------- tail kernel
def _csr(children, word):
    """(begin, key, word) lists from the key lists of the first nodes; the nodes behind them are childless."""
    P = 1 + sum(len(k) for k in children)
    begin = [0]
    for p in range(P):
        begin.append(begin[-1] + (len(children[p]) if p < len(children) else 0))
    out_word = [-1] * P
    for p, w in word.items():
        out_word[p] = w
    return begin, [k for ks in children for k in ks], out_word


def _planted():
    """Tables that no lexicon needs to produce (the kernel only reads them).  Node 0: 300 children and two whose key holds a
    token >= V (more than one pass of 256 threads); 1: five children; 2: a single child; 3: a terminal (word 7); 4: 39
    children and one with the l2r token V; 5: two children.  The 349 nodes behind them have no children."""
    rng = np.random.RandomState(11)
    def keys(k):      # noqa: E306
        flat = rng.choice((V - 2) * (V - 2), size=k, replace=False)
        return sorted(int((f // (V - 2) + 2) * 64 + f % (V - 2) + 2) for f in flat)
    children = [sorted(keys(300) + [60 * 64 + 3, 5 * 64 + 63]), keys(5), keys(1), [], sorted(keys(39) + [V * 64 + 2]), keys(2)]
    return _csr(children, {3: 7})


def _launch(tables, W, step, score, sdir, node, y, w, maxlen=6, N=3):
    """One launch of the tail on a planted state -> (the inputs, the PairBeamState after it)."""
    from sbl_for_multilingual_lip_reading_amd import ops
    S = N * W
    rng = np.random.RandomState(1000 * W + step)
    ys_old = np.full((2, S, 17), EOS, np.int64)
    ys_old[:, :, 0] = SOS
    ys_old[:, :, 1:step + 1] = rng.randint(2, V, (2, S, step))
    st = ops.PairBeamState(N, W, maxlen, SOS, EOS, DEV, lex=True, row_len=17)
    assert st.ys.shape == (2, 2, S, 17) and st.node.shape == (2, N, W) and st.hist_node.shape == (N, maxlen, W)
    assert int(st.node.abs().sum()) == 0      # reset(): every slot at the root
    st.score.copy_(torch.from_numpy(score))
    st.score_dir.copy_(torch.from_numpy(sdir))
    st.ys.fill_(-7)
    st.ys[:, step % 2].copy_(torch.from_numpy(ys_old))
    st.node.fill_(-7)
    st.node[step % 2].copy_(torch.from_numpy(node))
    for t in st.history()[:3] + (st.hist_node,):
        t.fill_(-7)
    st.hist_score.fill_(-7.0)
    trie = tuple(torch.tensor(t, dtype=torch.int32, device=DEV) for t in tables)
    ops.pair_beam_tail_lex(*(torch.from_numpy(a).to(DEV) for a in y + w), st, step, trie)
    torch.cuda.synchronize()
    return dict(N=N, W=W, step=step, maxlen=maxlen, y=y, w=w, score=score, sdir=sdir, node=node, ys_old=ys_old, tables=tables), st


def _reference(c):
    """float64 restatement of the candidates of include/sbl_hip.h: per clip {(slot, a, b): (total, dir l2r, dir r2l, node,
    ended)}, with the clamps of the header (nodes to 0 .. P-1, begin to 0 .. E, a key with a token >= V or a negative key: no
    candidate)."""
    begin, key, word = c["tables"]
    N, W, P, E = c["N"], c["W"], len(word), len(key)
    lp = []
    for d in (0, 1):
        logits = c["y"][d].astype(np.float64) @ c["w"][d].astype(np.float64).T
        m = logits.max(1, keepdims=True)
        lp.append((logits - m - np.log(np.exp(logits - m).sum(1, keepdims=True))).reshape(N, W, V))
    out = []
    for n in range(N):
        cands = {}
        for s in range(W):
            if not c["score"][n, s] > NEG:
                continue
            q = min(max(int(c["node"][n, s]), 0), P - 1)
            sc, sd = float(c["score"][n, s]), c["sdir"][n, s].astype(np.float64)
            if word[q] >= 0:
                cands[s, EOS, EOS] = (sc, sd[0], sd[1], q, True)
                continue
            for e in range(min(max(begin[q], 0), E), min(max(begin[q + 1], 0), E)):
                a, b = key[e] >> 6, key[e] & 63
                if key[e] >= 0 and a < V and b < V:
                    cands[s, a, b] = (sc + lp[0][n, s, a] + lp[1][n, s, b], sd[0] + lp[0][n, s, a], sd[1] + lp[1][n, s, b], e + 1, False)
        out.append(cands)
    return out


def _check(c, st, tol=1e-5):
    """The keep / score rule of test_pair_beam_tail_kernel with its 1e-5: the kept candidates are distinct candidates of the
    float64 restatement, the totals fall with the rank, every score (total and per direction) is the float64 score of that
    candidate within tol, no kept candidate is more than 2 tol below the float64 W-th best; an ended slot's three scores are
    carried bit for bit; the node is the entry's e + 1 (the slot's own node behind an ended slot) in node_new and hist_node;
    a rank without a candidate is dead with node 0; the new prefixes are ys_old[parent] || token || eos up to maxlen and
    untouched behind; every other history row and the node buffer that was read are untouched.  Returns the references."""
    N, W, step, maxlen = c["N"], c["W"], c["step"], c["maxlen"]
    ref = _reference(c)
    tok_l, tok_r, par, hs, hn = (t.cpu().numpy() for t in st.history() + (st.hist_node,))
    new = st.ys[:, 1 - step % 2].cpu().numpy()
    got_score, got_dir, got_node = st.score.cpu().numpy(), st.score_dir.cpu().numpy(), st.node[1 - step % 2].cpu().numpy()
    assert np.array_equal(st.ys[:, step % 2].cpu().numpy(), c["ys_old"]) and np.array_equal(st.node[step % 2].cpu().numpy(), c["node"])
    other = [i for i in range(maxlen) if i != step]
    assert all(np.all(a[:, other] == -7) for a in (tok_l, tok_r, par, hs, hn))
    assert np.array_equal(hs[:, step].view(np.int32), got_score.view(np.int32)) and np.array_equal(hn[:, step], got_node)
    worst = 0.0
    for n in range(N):
        best = sorted((v[0] for v in ref[n].values()), reverse=True)
        n_keep = min(W, len(best))
        assert [r for r in range(W) if got_score[n, r] > NEG] == list(range(n_keep)), (n, got_score[n], len(best))
        seen = set()
        for r in range(W):
            msg = "W=%d step=%d clip %d rank %d" % (W, step, n, r)
            p, a, b = int(par[n, step, r]), int(tok_l[n, step, r]), int(tok_r[n, step, r])
            if r >= n_keep:
                assert (p, a, b, int(got_node[n, r])) == (r, EOS, EOS, 0) and np.all(got_dir[n, r] == NEG), msg
            else:
                assert (p, a, b) in ref[n] and (p, a, b) not in seen, msg
                seen.add((p, a, b))
                total, dl, dr, node, ended = ref[n][p, a, b]
                worst = max(worst, abs(got_score[n, r] - total))
                assert abs(got_score[n, r] - total) <= tol, msg
                assert r == 0 or got_score[n, r] <= got_score[n, r - 1], msg
                assert total >= best[n_keep - 1] - 2 * tol, msg
                assert abs(got_dir[n, r, 0] - dl) <= tol and abs(got_dir[n, r, 1] - dr) <= tol, msg
                assert int(got_node[n, r]) == node, msg
                if ended:
                    assert got_score[n, r].view(np.int32) == c["score"][n, p].view(np.int32), msg
                    assert np.array_equal(got_dir[n, r].view(np.int32), c["sdir"][n, p].view(np.int32)), msg
            for d, t in ((0, a), (1, b)):
                want = np.full(17, -7, np.int64)
                want[:maxlen + 1] = EOS
                want[:step + 1] = c["ys_old"][d, n * W + p, :step + 1]
                want[step + 1] = t
                assert np.array_equal(new[d, n * W + r], want), msg
    print("W=%d step=%d: max|dscore| %.2e (bound %.0e)" % (W, step, worst, tol))
    return ref


def _random_inputs(N, W, seed):
    rng = np.random.RandomState(seed)
    y = [rng.randn(N * W, 512).astype(np.float32) for _ in (0, 1)]
    w = [(rng.randn(V, 512) * 0.05).astype(np.float32) for _ in (0, 1)]
    return rng, y, w


@pytest.mark.parametrize("W", [1, 2, 5, 16])
def test_tail_kernel_at_the_root(W):
    """Step 0, N = 3, V = 58: slot 0 of every clip is live at the root, whose 302 entries are more than one pass of the 256
    threads; the two keys with a token >= V are never kept."""
    tables = _planted()
    _, y, w = _random_inputs(3, W, 50 + W)
    score, sdir = np.full((3, W), NEG, np.float32), np.full((3, W, 2), NEG, np.float32)
    score[:, 0], sdir[:, 0] = 0.0, 0.0
    c, st = _launch(tables, W, 0, score, sdir, np.zeros((3, W), np.int32), y, w)
    ref = _check(c, st)
    assert all(len(r) == 300 for r in ref)
    assert np.all(st.hist_par[:, 0].cpu().numpy() == 0)
    assert np.all(st.hist_tok_l[:, 0].cpu().numpy() < V) and np.all(st.hist_tok_r[:, 0].cpu().numpy() < V)


@pytest.mark.parametrize("W", [1, 2, 5, 16])
def test_tail_kernel_on_mixed_slots(W):
    """Step 3.  Clip 0: ordinary nodes, the node with a single child, an ended slot and the node that holds a token >= V, in
    turn, its last slot dead (W > 1).  Clip 1: the single-child node, an ended slot (W > 2) and dead slots: fewer candidates
    than W from W = 2 on, the other ranks dead with node 0.  Clip 2: every slot live, the ended slot scoring best."""
    tables = _planted()
    rng, y, w = _random_inputs(3, W, 70 + W)
    score = (-rng.rand(3, W) * 10).astype(np.float32)
    sdir = (-rng.rand(3, W, 2) * 10).astype(np.float32)
    node = np.zeros((3, W), np.int32)
    node[0] = [(1, 2, 3, 4, 5)[s % 5] for s in range(W)]
    node[2] = [(3, 4, 5, 1, 2)[s % 5] for s in range(W)]
    node[1, 0] = 2 if W > 1 else 3
    score[2, 0] = 5.0      # the ended slot of clip 2 leads
    if W > 1:
        score[0, W - 1], sdir[0, W - 1] = NEG, NEG
        score[1, 1:], sdir[1, 1:] = NEG, NEG
    if W > 2:
        node[1, 1] = 3
        score[1, 1], sdir[1, 1] = -1.5, (-0.25, -1.25)
    c, st = _launch(tables, W, 3, score, sdir, node, y, w)
    ref = _check(c, st)
    par, tok_l = st.hist_par[:, 3].cpu().numpy(), st.hist_tok_l[:, 3].cpu().numpy()
    if W > 1:
        assert not np.any(par[0] == W - 1)                                   # the dead slot is nobody's parent
        assert len(ref[1]) == min(W - 1, 2) and len(ref[1]) < W               # fewer candidates than W
        assert np.all(st.node[0, 1, len(ref[1]):].cpu().numpy() == 0)         # step 3 writes node buffer 0
    assert (par[2, 0], tok_l[2, 0]) == (0, EOS) and float(st.score[2, 0]) == 5.0 and int(st.node[0, 2, 0]) == 3
    assert any(v[4] for v in ref[0].values()) == (W > 3)                      # a live ended slot in clip 0 from W = 5 on
    assert all(a < V and b < V for r in ref for (_, a, b) in r)


def test_tail_tie_order():
    """Every slot reads the same rows and head rows 2, 3 (l2r) and 5, 6 (r2l) are exact copies that dominate, so the entries
    (2,5) (2,6) (3,5) (3,6) of a slot tie bit for bit (the fifth entry, (4,7), is far behind): they are kept in key order,
    the lower slot first among equal slots; clip 0's slot 1 is ahead of its other slots."""
    N, W = 2, 6
    rng = np.random.RandomState(7)
    y = [np.tile(rng.randn(1, 512).astype(np.float32), (N * W, 1)) for _ in (0, 1)]
    w = [(rng.randn(V, 512) * 0.01).astype(np.float32) for _ in (0, 1)]
    w[0][2] = w[0][3] = y[0][0] * 0.02
    w[1][5] = w[1][6] = y[1][0] * 0.02
    ties = [2 * 64 + 5, 2 * 64 + 6, 3 * 64 + 5, 3 * 64 + 6]
    tables = _csr([[9 * 64 + 9], ties + [4 * 64 + 7]], {})      # node 1 holds the entries 1 .. 5: children 2 .. 6
    score, sdir = np.full((N, W), -1.0, np.float32), np.full((N, W, 2), -0.5, np.float32)
    score[0, 1] = -0.5
    c, st = _launch(tables, W, 1, score, sdir, np.ones((N, W), np.int32), y, w, N=N)
    _check(c, st)
    tok_l, tok_r, par, hs = (t.cpu().numpy()[:, 1] for t in st.history())
    assert tok_l.tolist() == [[2, 2, 3, 3, 2, 2]] * 2 and tok_r.tolist() == [[5, 6, 5, 6, 5, 6]] * 2
    assert par.tolist() == [[1, 1, 1, 1, 0, 0], [0, 0, 0, 0, 1, 1]]
    assert st.hist_node[:, 1].cpu().tolist() == [[2, 3, 4, 5, 2, 3]] * 2
    assert len(set(hs[0, :4].tolist())) == 1 and len(set(hs[1].tolist())) == 1 and hs[0, 4] == hs[1, 0]


def test_tail_with_tables_that_point_out_of_range():
    """Node values outside 0 .. P-1 and begin values outside 0 .. E: the launch succeeds and keeps exactly the candidates of
    the clamped tables (every index the kernel forms is clamped, so nothing is read out of bounds).  P = 6, E = 5; entry 2
    is a negative key, entry 3 holds the l2r token 60 >= V; node 4 is a terminal."""
    W = 3
    begin = [-7, 3, 2, 10 ** 6, 4, -1, 5]      # clamped: 0 3 2 5 4 0 5 -> node 1 and node 3 have inverted ranges
    key = [2 * 64 + 3, 4 * 64 + 5, -1, 60 * 64 + 2, 6 * 64 + 7]
    word = [-1, -1, -1, -1, 3, -1]
    node = np.array([[-5, 106, 2], [1, 2, 3], [4, -(2 ** 31), 2 ** 31 - 1]], np.int32)
    rng, y, w = _random_inputs(3, W, 90)
    score = (-rng.rand(3, W) * 10).astype(np.float32)
    sdir = (-rng.rand(3, W, 2) * 10).astype(np.float32)
    c, st = _launch((begin, key, word), W, 2, score, sdir, node, y, w)
    ref = _check(c, st)
    assert sorted(ref[0]) == [(0, 2, 3), (0, 4, 5), (1, 2, 3), (1, 4, 5), (1, 6, 7), (2, 6, 7)]
    assert sorted(ref[1]) == [(1, 6, 7)] and sorted(ref[2]) == [(0, EOS, EOS), (1, 2, 3), (1, 4, 5), (2, 2, 3), (2, 4, 5), (2, 6, 7)]
    assert st.score[1].cpu().tolist()[1:] == [NEG, NEG] and st.node[1, 1].cpu().tolist() == [5, 0, 0]


# --------------------------------------------------------------------------- the whole search
_DECODERS = {}


def _decoder(salt):
    """A 2-layer SBL decoder on the GPU with the oracle's "varied" weights of `salt`, and those weights."""
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    if salt not in _DECODERS:
        sd = PB.decoder_state_dict(2, salt)
        dec = Decoder(SOS, EOS, V, 512, 2, 8, 64, 64, 512, 2048, dropout=0.0)
        own = dec.state_dict()
        dec.load_state_dict({k: (v if k.endswith("pe") else sd["decoder." + k]) for k, v in own.items()})
        _DECODERS[salt] = (dec.to(DEV).eval(), sd)
    return _DECODERS[salt]


def _lexicon(words):
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    return Lexicon(words, device=DEV, vocab=V, sos_id=SOS, eos_id=EOS)


def _host(res):
    out = {k: getattr(res, k) for k in ("word", "cand", "score", "score_dir", "ys_l2r", "ys_r2l")}
    out.update(zip(("tok_l", "tok_r", "par", "hist_score", "node"), res.history))
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def _reversed_rows(ys):
    """sos, reversed(tokens before the first eos), eos fill, for (..., 17) numpy rows."""
    out = np.full_like(ys, EOS)
    for idx in np.ndindex(ys.shape[:-1]):
        w = LB.spelled(ys[idx].tolist(), SOS, EOS)
        out[idx][0] = SOS
        out[idx][1:len(w) + 1] = w[::-1]
    return out


@pytest.mark.parametrize("W,salt", [(3, 7), (5, 8)])
def test_search_passes_the_checker_and_score_pairs(W, salt, precision):
    """A 2-layer decoder, N = 3 clips of 8 encoder rows, 40 words of 1..6 tokens (with a duplicate row and a word that is a
    prefix of another).  follow_lex passes on the GPU's history; the returned rows, words and scores are the last step's
    slots; the n-best words of a clip are distinct; Lexicon.lookup of the l2r row and of the reversed r2l row both give
    `cand`; and Decoder.score_pairs over the c_w + 1 positions of the returned rows agrees with score / score_dir within
    step_tol(c_w)."""
    dec, sd = _decoder(salt)
    words = LB.make_words(40, V, salt, 1, 6)
    lex = _lexicon(words)
    N, nbest = 3, W
    enc = PB.encoder_output(N, 8, salt)
    with torch.no_grad():
        res = dec.beam_search_lex(enc.to(DEV), lex, W, nbest)
        got = _host(res)
    steps = lex.max_len + 1
    assert got["hist_score"].shape == (N, steps, W) and got["ys_l2r"].shape == (N, nbest, 17) and got["cand"].dtype == np.int32
    st = PL.follow_lex(tuple(got[k] for k in ("tok_l", "tok_r", "par", "hist_score", "node")), sd, enc, 2, words, W)
    print("W=%d salt %d %s: max|dscore| %.2e, max deficit %.2e (2 tol at the last step %.1e)" % (
        W, salt, precision, st["max_dscore"], st["max_deficit"], 2 * PB.step_tol(steps - 1)))
    assert np.array_equal(got["ys_l2r"], st["ys_l2r"]) and np.array_equal(got["ys_r2l"], st["ys_r2l"])
    assert np.array_equal(got["cand"], st["cand"]) and np.array_equal(got["word"], got["cand"][:, 0]) and got["word"].dtype == np.int64
    assert np.array_equal(got["score"], got["hist_score"][:, steps - 1]) and np.all(np.isfinite(got["score"]))
    assert np.all(got["cand"] >= 0) and all(len(set(row.tolist())) == nbest for row in got["cand"])
    rows = PL.word_rows(words, SOS, EOS)
    assert np.array_equal(got["ys_l2r"], rows[0][got["cand"]]) and np.array_equal(got["ys_r2l"], rows[1][got["cand"]])
    assert np.array_equal(lex.lookup(res.ys_l2r).cpu().numpy(), got["cand"])
    assert np.array_equal(lex.lookup(torch.from_numpy(_reversed_rows(got["ys_r2l"])).to(DEV)).cpu().numpy(), got["cand"])
    c_w = lex.lengths.numpy()[got["cand"]]
    with torch.no_grad():
        ps = dec.score_pairs(enc.to(DEV), res.ys_l2r, res.ys_r2l, torch.from_numpy((c_w + 1).astype(np.int32).reshape(-1)).to(DEV),
                             group=nbest)
    tol = 2 * PB.LOGIT_TOL * (c_w + 1)      # step_tol(c_w)
    d = np.abs(ps.score.cpu().numpy().reshape(N, nbest) - got["score"])
    dd = np.abs(ps.score_dir.cpu().numpy().reshape(N, nbest, 2) - got["score_dir"])
    print("  score_pairs: max|dscore| %.2e, max|ddir| %.2e (smallest bound %.1e)" % (d.max(), dd.max(), tol.min()))
    assert np.all(d <= tol) and np.all(dd <= tol[..., None])


def test_exhaustive_search_returns_every_word(precision):
    """6 words, W = nbest = 8: every clip returns every word once, best first; ranks 6 and 7 are dead (cand -1, score -inf);
    the scores are those of score_pairs over all six words within step_tol(c_w)."""
    dec, _ = _decoder(7)
    words = PL.WORDS6
    lex = _lexicon(words)
    N = 3
    enc = PB.encoder_output(N, 8, 31).to(DEV)
    rows = [torch.from_numpy(r).to(DEV).repeat(N, 1) for r in PL.word_rows(words, SOS, EOS)]
    with torch.no_grad():
        got = _host(dec.beam_search_lex(enc, lex, 8, 8))
        ps = dec.score_pairs(enc, rows[0], rows[1], (lex.lengths + 1).to(torch.int32).repeat(N).to(DEV), group=6)
    ref = ps.score.cpu().numpy().reshape(N, 6)
    assert got["hist_score"].shape == (N, 6, 8)
    for n in range(N):
        assert sorted(got["cand"][n, :6].tolist()) == list(range(6)) and got["cand"][n, 6:].tolist() == [-1, -1]
        assert np.all(got["score"][n, 6:] == NEG) and np.all(got["score_dir"][n, 6:] == NEG)
        assert np.all(np.diff(got["score"][n, :6]) <= 0) and got["word"][n] == got["cand"][n, 0]
        for r in range(6):
            w = got["cand"][n, r]
            assert abs(got["score"][n, r] - ref[n, w]) <= PB.step_tol(len(words[w])), (n, r, w)
        # the best word by score_pairs leads unless the two scores are closer than the tolerance
        assert ref[n, got["cand"][n, 0]] >= ref[n].max() - 2 * PB.step_tol(5)


def test_one_word_lexicon_with_beam_one():
    dec, _ = _decoder(7)
    lex = _lexicon([[7, 3, 9, 3]])
    enc = PB.encoder_output(4, 8, 32).to(DEV)
    with torch.no_grad():
        got = _host(dec.beam_search_lex(enc, lex, 1))
    assert got["word"].tolist() == [0] * 4 and got["cand"].tolist() == [[0]] * 4 and np.all(np.isfinite(got["score"]))
    assert got["ys_l2r"][:, 0, :6].tolist() == [[SOS, 7, 3, 9, 3, EOS]] * 4 and got["ys_r2l"][:, 0, :6].tolist() == [[SOS, 3, 9, 3, 7, EOS]] * 4
    assert got["node"][:, :, 0].tolist() == [[1, 2, 3, 4, 5]] * 4


# --------------------------------------------------------------------------- validation
def _transformer():
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    from sbl_for_multilingual_lip_reading_amd.transformer.transformer import Transformer
    m = Transformer(Encoder(512, 2, 8, 64, 64, 512, 2048), Decoder(SOS, EOS, V, 512, 2, 8, 64, 64, 512, 2048), None)
    m.load_state_dict({k: (v if k.endswith("pe") else torch.from_numpy(detfill.fill_value(k, tuple(v.shape), 0, "varied").copy()))
                       for k, v in m.state_dict().items()})
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    m.visual_frontend.frontend_dropout_p = 0.0
    return m.to(DEV)


def test_validate_words_lex_meter_and_graph_replay():
    """Transformer.validate_words_lex in eval() under no_grad.  Eager: the meter's counters equal those computed on the host
    from the returned word and cand, with gold words that are chosen, merely among the n-best, and absent; valid_rows masks
    the tail.  Then the whole call captured as ONE hipGraph: two replays on different clips equal the eager calls bit for
    bit (words, scores, token rows, the five histories) and the meter's counters equal the eager ones."""
    from sbl_for_multilingual_lip_reading_amd.transformer.metrics import WordAccuracyMeter
    B, T, Hh, Ww, W, nbest = 3, 8, 24, 24, 4, 3
    m = _transformer().eval()
    lex = _lexicon(LB.make_words(40, V, 4, 1, 6))
    xs = [torch.from_numpy(detfill.synthetic_batch(B, T, Hh, Ww, salt)[0]).to(DEV) for salt in (51, 52)]
    vr = torch.tensor([B - 1], dtype=torch.int32, device=DEV)
    host = lambda r: [t.cpu().numpy().copy() for t in r[:6] + r.history]      # noqa: E731
    with torch.no_grad():
        golds = []
        for x in xs:
            r = m.recognize_words_lex(x, lex, W, nbest)
            cand, word = r.cand.cpu().numpy(), r.word.cpu().numpy()
            assert np.array_equal(word, cand[:, 0]) and np.all(cand >= 0)
            absent = [w for w in range(40) if w not in cand[1]][0]
            golds.append(torch.tensor([word[0], absent, cand[2, 1]], dtype=torch.int64, device=DEV))
        full, eager, meter = (WordAccuracyMeter(device=DEV) for _ in range(3))
        r = m.validate_words_lex(xs[0], golds[0], lex, full, beam_size=W, nbest=nbest)
        assert full.acc.tolist() == [3, 1, 2] and r.cand.shape == (B, nbest) and r.word.dtype == torch.int64
        want = [host(m.validate_words_lex(x, g, lex, eager, valid_rows=vr, beam_size=W, nbest=nbest)) for x, g in zip(xs, golds)]
        assert eager.acc.tolist() == [2 * (B - 1), 2, 2]      # row 2, whose gold is among the n-best, is masked
        torch.cuda.synchronize()
        static_x, static_g = xs[0].clone(), golds[0].clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m.validate_words_lex(static_x, static_g, lex, meter, valid_rows=vr, beam_size=W, nbest=nbest)      # warm-up on the capture stream
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            res = m.validate_words_lex(static_x, static_g, lex, meter, valid_rows=vr, beam_size=W, nbest=nbest)
        meter.reset()
        for x, g, ref in zip(xs, golds, want):
            static_x.copy_(x)
            static_g.copy_(g)
            graph.replay()
            torch.cuda.synchronize()
            for k, (a, b) in enumerate(zip(host(res), ref)):
                assert np.array_equal(a, b), k
    assert eager.acc.tolist() == meter.acc.tolist()
    assert np.all(np.isfinite(want[0][2])) and not np.array_equal(want[0][2], want[1][2])


def test_argument_errors():
    from sbl_for_multilingual_lip_reading_amd import _lib, ops
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    dec, _ = _decoder(7)
    lex = _lexicon(PL.WORDS6)
    enc = PB.encoder_output(2, 8, 33)
    with pytest.raises(_lib.SblHipError, match="no CPU path"):
        dec.beam_search_lex(enc, lex, 3)
    enc = enc.to(DEV)
    for W in (0, 17):
        with pytest.raises(_lib.SblHipError, match="beam_size"):
            dec.beam_search_lex(enc, lex, W)
    with pytest.raises(_lib.SblHipError, match="nbest"):
        dec.beam_search_lex(enc, lex, 3, 4)
    with pytest.raises(_lib.SblHipError, match="not this decoder's"):
        dec.beam_search_lex(enc, Lexicon([[5, 6]], device=DEV, vocab=V, sos_id=2, eos_id=3), 3)
    # the tail refuses a state without node buffers and tables of the wrong kind
    st = ops.PairBeamState(2, 3, 6, SOS, EOS, DEV)
    y = torch.zeros(6, 512, device=DEV)
    w = torch.zeros(V, 512, device=DEV)
    with pytest.raises(_lib.SblHipError, match="lex=True"):
        ops.pair_beam_tail_lex(y, y, w, w, st, 0, lex.pair_trie())
    st = ops.PairBeamState(2, 3, 6, SOS, EOS, DEV, lex=True)
    with pytest.raises(_lib.SblHipError, match="pair trie tables"):
        ops.pair_beam_tail_lex(y, y, w, w, st, 0, lex.trie())
