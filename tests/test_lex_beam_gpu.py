"""GPU checks of the lexicon-constrained beam search of the single-direction decoder (sbl_beam_tail_lex in csrc/beam_step.hip,
sbl_lexicon_lookup in csrc/lexicon.hip, Seq2SeqDecoder.beam_search_lex / recognize_words, Seq2SeqTransformer.validate_words):
the constrained tail pinned bit for bit to sbl_beam_tail through the one-node table, the tail alone against a float64
restatement on planted trie tables, the lookup against a dict trie, the whole search against the plain-torch restatement
(tests/lex_beam_oracle.py; its margins are asserted in tests/test_lex_beam_cpu.py), hipGraph replay of validate_words, and
the guards."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import beam_oracle as B
import lex_beam_oracle as L
from test_lex_beam_cpu import TRIE_CASES
from test_seq2seq_gpu import gpu_model, precision  # noqa: F401  (precision is a fixture)

pytestmark = pytest.mark.gpu
NEG = float("-inf")
DEV = "cuda:0"


def _i64(bits):
    """Python bit patterns -> the int64 tensor that holds them."""
    return torch.tensor([b - 2 ** 64 if b >> 63 else b for b in bits], dtype=torch.int64)


def _pe():
    from sbl_for_multilingual_lip_reading_amd.transformer.module import PositionalEncoding
    return PositionalEncoding(512, max_len=64).pe[0]


def _snapshot(st, x_next):
    out = dict(score=st.score, last_tok=st.last_tok, anc=st.anc, end_score=st.end_score, end_ref=st.end_ref, end_count=st.end_count)
    out.update(zip(("hist_tok", "hist_par", "hist_score", "hist_flag"), st.history()))
    if x_next is not None:
        out["x_next"] = x_next
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


# --------------------------------------------------------------------------- 1. the pin against sbl_beam_tail
@pytest.mark.parametrize("prior", [False, True])
@pytest.mark.parametrize("V,W", [(5, 3), (42, 16), (64, 16)])
def test_one_node_table_is_the_unconstrained_tail(V, W, prior):
    """P = 1, mask = all V bits, first = 0: every candidate exists and every child clamps to the root, so a whole search of
    six steps through sbl_beam_tail_lex equals the one through sbl_beam_tail bit for bit in every output at every step
    (scores, tokens, both ancestry buffers, history, ended list, next input rows); the nodes stay 0."""
    from sbl_for_multilingual_lip_reading_amd import ops
    N, maxlen, eos, scale = 3, 6, 1, 0.25
    rng = np.random.RandomState(1000 * V + 10 * W + prior)
    w = torch.from_numpy((rng.randn(V, 512) * 0.05).astype(np.float32)).to(DEV)
    emb = torch.from_numpy(rng.randn(V, 512).astype(np.float32)).to(DEV)
    lp = None
    if prior:
        lp = (rng.randn(V, V) * 2).astype(np.float32)
        lp[rng.rand(V, V) < 0.3] = NEG
        lp[:, eos] = 1.0
        lp = torch.from_numpy(lp).to(DEV)
    pe = _pe().to(DEV)
    trie = (_i64([(1 << V) - 1]).to(DEV), torch.zeros(1, dtype=torch.int32, device=DEV))
    base, lex = ops.BeamState(N, W, maxlen, 0, DEV), ops.BeamState(N, W, maxlen, 0, DEV, lex=True)
    assert base.node is None and lex.node.shape == (N, W) and lex.node.dtype == torch.int32
    for st in (base, lex):          # the same sentinels where a step does not write
        st.anc.fill_(-7)
        for t in st.history() + (st.end_ref,):
            t.fill_(-7)
        st.end_score.fill_(-7.0)
    lex.node.fill_(9)
    lex.reset()
    assert int(lex.node.abs().sum()) == 0
    ended = 0
    for step in range(maxlen):
        y = torch.from_numpy(rng.randn(N * W, 512).astype(np.float32)).to(DEV)
        xa, xb = ((torch.full((N * W, 512), -7.0, device=DEV) for _ in range(2)) if step + 1 < maxlen else (None, None))
        ops.beam_tail(y, w, lp, base, step, eos, emb, pe, scale, x_next=xa)
        ops.beam_tail(y, w, lp, lex, step, eos, emb, pe, scale, x_next=xb, trie=trie)
        torch.cuda.synchronize()
        a, b = _snapshot(base, xa), _snapshot(lex, xb)
        for k in a:
            assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), "V=%d W=%d step %d: %s" % (V, W, step, k)
        assert int(lex.node.abs().sum()) == 0
        ended = int(a["end_count"].sum())
    assert ended > 0 and (a["hist_flag"] != 0).any()


# --------------------------------------------------------------------------- 2. the tail alone
@pytest.mark.parametrize("V,W", L.TAIL_SHAPES)
def test_lex_tail_kernel(V, W):
    """Two launches on N = 3 clips against float64 (lex_beam_oracle.tail_ref), a middle step and the last one, on the
    planted table and states of lex_beam_oracle.tail_case: a slot whose node allows only eos, a node whose only child is
    token V - 1, a dead slot, a clip with fewer candidates than W, all-zero masks where nothing is kept, an exact tie of
    two parents, nodes out of range on input and children that clamp.  Integers exact - tokens, parents, flags, nodes,
    ancestry rows, ended refs and counts - scores 1e-5 (the bound of test_beam_tail_kernel), next input rows 1e-6;
    untouched history rows, ended records and ancestry columns keep their sentinel."""
    from sbl_for_multilingual_lip_reading_amd import ops
    N, maxlen, eos, scale = L.TAIL_N, L.TAIL_MAXLEN, L.TAIL_EOS, L.TAIL_SCALE
    Sn = N * W
    case = L.tail_case(V, W)
    w, emb, lp = case["w"], case["emb"], case["lp"]
    pe = _pe().numpy()
    wd, ed, ped, lpd = (torch.from_numpy(a).to(DEV) for a in (w, emb, pe, lp))
    trie = (_i64(case["mask"]).to(DEV), torch.tensor(case["first"], dtype=torch.int32, device=DEV))
    saw = set()
    for c in case["steps"]:
        step, ref, counts = c["step"], c["ref"], c["counts"]
        st = ops.BeamState(N, W, maxlen, 0, DEV, lex=True)
        st.score.copy_(torch.from_numpy(c["score"]).view(N, W))
        st.last_tok.copy_(torch.from_numpy(c["last"]).view(N, W))
        st.node.copy_(torch.from_numpy(c["node"]).view(N, W))
        st.anc[step % 2].copy_(torch.from_numpy(c["anc_old"]))
        st.anc[1 - step % 2].fill_(-7)
        for t in st.history() + (st.end_ref,):
            t.fill_(-7)
        st.end_score.fill_(-7.0)
        st.end_count.copy_(torch.from_numpy(counts))
        x_next = torch.full((Sn, 512), -7.0, device=DEV) if step + 1 < maxlen else None
        ops.beam_tail(torch.from_numpy(c["y"]).to(DEV), wd, lpd, st, step, eos, ed, ped, scale, x_next=x_next, trie=trie)
        torch.cuda.synchronize()
        tok, par, hs, flag = (t.cpu().numpy() for t in st.history())
        msg = "V=%d W=%d step=%d" % (V, W, step)
        assert np.array_equal(flag[:, step], ref["flag"]), msg
        assert np.array_equal(tok[:, step], ref["tok"]) and np.array_equal(par[:, step], ref["par"]), msg
        assert np.array_equal(st.node.cpu().numpy(), ref["node"]), msg
        fin = ref["flag"] != 0
        assert np.all(hs[:, step][~fin] == NEG) and (not fin.any() or np.abs(hs[:, step][fin] - ref["score"][fin]).max() <= 1e-5), msg
        other = [i for i in range(maxlen) if i != step]
        assert all(np.all(a[:, other] == -7) for a in (tok, par, hs, flag)), msg
        ns = st.score.cpu().numpy()
        live = ref["flag"] == 1
        assert np.all(ns[~live] == NEG) and (not live.any() or np.abs(ns[live] - ref["score"][live]).max() <= 1e-5), msg
        assert np.array_equal(st.last_tok.cpu().numpy(), ref["tok"]), msg
        anc_new = st.anc[1 - step % 2].cpu().numpy()
        assert np.array_equal(anc_new[:, :step + 1], ref["anc"]) and np.all(anc_new[:, step + 1:] == -7), msg
        assert np.array_equal(st.anc[step % 2].cpu().numpy(), c["anc_old"]), msg
        es, er, ec = st.end_score.cpu().numpy(), st.end_ref.cpu().numpy(), st.end_count.cpu().numpy()
        for n in range(N):
            c0, k = int(counts[n]), len(ref["ended"][n])
            assert ec[n] == c0 + k, msg
            assert np.all(er[n, :c0] == -7) and np.all(er[n, c0 + k:] == -7) and np.all(es[n, c0 + k:] == -7.0), msg
            assert er[n, c0:c0 + k].tolist() == [r for _, r in ref["ended"][n]], msg
            assert k == 0 or np.abs(es[n, c0:c0 + k] - np.array([s for s, _ in ref["ended"][n]])).max() <= 1e-5, msg
        if x_next is not None:
            want = emb.astype(np.float64)[ref["tok"].reshape(-1)] * scale + pe[step + 1].astype(np.float64)
            assert np.abs(x_next.cpu().numpy() - want).max() <= 1e-6, msg
        saw |= c["saw"]
    want = {"all-zero mask", "node out of range", "only eos", "only child V - 1"}
    assert want <= saw and (W == 1 or {"dead slot", "fewer candidates than W", "parent tie"} <= saw), saw


# --------------------------------------------------------------------------- 3. lookup
def _rows(seqs, sos, eos, Ly=17):
    out = np.full((len(seqs), Ly), eos, np.int64)
    out[:, 0] = sos
    for i, s in enumerate(seqs):
        out[i, 1:1 + len(s)] = s
    return out


@pytest.mark.parametrize("name,words,V,sos,eos", TRIE_CASES, ids=[c[0] for c in TRIE_CASES])
def test_lexicon_lookup(name, words, V, sos, eos):
    """Every word finds itself (duplicates: the lowest index), a truncated word and a word with another last token find
    what the dict trie says (-1 unless they spell another word), an empty row gives -1; `node` is the breadth-first id of
    the row's prefix or -1.  Also through a strided (R, 2, 17) view and with sos / ignore entries inside a row."""
    from sbl_for_multilingual_lip_reading_amd import ops
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    lex = Lexicon(words, device=DEV, vocab=V, sos_id=sos, eos_id=eos)
    children, owner = L.dict_trie(words)
    ident = {p: k for k, p in enumerate(L.bfs_order(children))}
    other = next(t for t in range(V) if t not in (sos, eos))
    seqs = [tuple(w) for w in words]
    seqs += [s[:-1] for s in seqs[:len(words)]]
    seqs += [s[:-1] + ((s[-1] + 1 if s[-1] + 1 < V and s[-1] + 1 not in (sos, eos) else other),) for s in seqs[:len(words)]]
    seqs += [()]
    ys = torch.from_numpy(_rows(seqs, sos, eos)).to(DEV)
    word, node = ops.lexicon_lookup(ys, lex.trie(), sos, eos, -1)
    torch.cuda.synchronize()
    assert word.dtype == torch.int32 and word.shape == (len(seqs),) and node.shape == word.shape
    want_w = [owner.get(s, -1) for s in seqs]
    want_n = [ident.get(s, -1) for s in seqs]
    assert word.tolist() == want_w and node.tolist() == want_n, name
    assert want_w[:len(words)] == [owner[tuple(w)] for w in words] and min(want_w[:len(words)]) >= 0
    assert want_w[-1] == -1 and want_n[-1] == 0 and -1 in want_w[len(words):2 * len(words)] and -1 in want_w[2 * len(words):-1]
    assert torch.equal(lex.lookup(ys), word)
    # a strided view, and rows with an ignore and a sos entry inside (dropped) and tokens behind the first eos (cut)
    wide = torch.full((len(seqs), 2, 17), 5, dtype=torch.int64, device=DEV)
    wide[:, 0] = ys
    assert torch.equal(lex.lookup(wide[:, 0]), word) and lex.lookup(wide).shape == (len(seqs), 2)
    w0 = list(words[0])
    messy = [sos, -1] + w0[:1] + [sos] + w0[1:] + [eos, other, other]
    row = torch.tensor([messy + [eos] * (20 - len(messy))], dtype=torch.int64, device=DEV)
    assert lex.lookup(row).tolist() == [owner[tuple(w0)]]
    assert ops.lexicon_lookup(ys[:0], lex.trie(), sos, eos, -1)[0].shape == (0,)


# --------------------------------------------------------------------------- 4. the whole search
_MODELS = {}


def _model(shape, salt):
    """The model of a shape and salt on the device with its fixture view, built once per process."""
    if (shape, salt) not in _MODELS:
        g = L.e2e_fixture(shape, salt)
        _MODELS[shape, salt] = (g, gpu_model(g, train=False))
    return _MODELS[shape, salt]


def _got(res):
    out = dict(yseq=res.yseq, lengths=res.lengths, scores=res.scores, n_hyps=res.n_hyps)
    out.update(zip(("hist_tok", "hist_par", "hist_score", "hist_flag"), res.history))
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("shape,Wn,W,prior", L.E2E_CASES)
def test_lexicon_search_matches_oracle(shape, Wn, W, prior, precision):  # noqa: F811
    """beam_search_lex and recognize_words (nbest = 5 and 1) against tests/lex_beam_oracle.py on unseen weights and clips:
    kept tokens, parents and flags of every step, n-best tokens, lengths, n_hyps and words exact; scores within
    score_tol(maxlen).  cand rows hold no repeated word, word == cand[:, 0], Lexicon.lookup(yseq) == cand."""
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    salt, _, clips = L.e2e_pick(shape, Wn, W, prior)
    ref = L.e2e_oracle(shape, Wn, W, prior)
    g, m = _model(shape, salt)
    lex = Lexicon(L.e2e_words(shape, Wn, W, prior), device=DEV, vocab=m.decoder.n_tgt_vocab)
    lp = L.e2e_prior(shape).to(DEV) if prior else None
    maxlen = ref["maxlen"]
    tag = "%s Wn=%d W=%d prior=%d/%s" % (shape, Wn, W, prior, precision)
    with torch.no_grad():
        enc, _ = m._encode(B.case_clips(g)[:clips].to(DEV))
        res = m.decoder.beam_search_lex(enc, W, L.E2E_NBEST, 0, lp, lex)
        words = {k: m.decoder.recognize_words(enc, lex, beam_size=W, nbest=k, log_prior=lp) for k in (L.E2E_NBEST, 1)}
    torch.cuda.synchronize()
    got = _got(res)
    why = lambda: "%s: %s" % (tag, B.first_divergence(got, ref))      # noqa: E731
    assert got["yseq"].shape == (len(enc), L.E2E_NBEST, maxlen + 2) and got["hist_tok"].shape == (len(enc), maxlen, W)
    assert B.first_divergence(got, ref) == "the histories agree", why()
    fin = ref["hist_flag"] != 0
    dh = np.abs(got["hist_score"][fin] - ref["hist_score"][fin]).max()
    assert np.all(got["hist_score"][~fin] == NEG) and dh <= B.score_tol(maxlen), why()
    for k, wr in words.items():
        r = L.first_k(ref, k)
        fin_k = np.isfinite(r["scores"])
        d = np.abs(wr.score.cpu().numpy()[fin_k] - r["scores"][fin_k]).max()
        print("%s nbest=%d: max|dscore| %.2e (bound %.0e)" % (tag, k, d, B.score_tol(maxlen)))
        assert np.array_equal(wr.n_hyps.cpu().numpy(), r["n_hyps"]), why()
        assert np.array_equal(wr.yseq.cpu().numpy(), r["yseq"]), why()
        assert np.array_equal(np.isfinite(wr.score.cpu().numpy()), np.isfinite(r["scores"])) and d <= B.score_tol(maxlen), why()
        cand = wr.cand.cpu().numpy()
        assert wr.cand.dtype == torch.int32 and wr.word.dtype == torch.int64 and cand.shape == (len(enc), k)
        assert np.array_equal(cand, r["cand"]), why()
        assert np.array_equal(wr.word.cpu().numpy(), cand[:, 0]) and np.array_equal(wr.word.cpu().numpy(), r["word"])
        for n in range(len(cand)):
            row = cand[n, :r["n_hyps"][n]].tolist()
            assert len(set(row)) == len(row) and min(row) >= 0 and np.all(cand[n, r["n_hyps"][n]:] == -1)
        assert torch.equal(lex.lookup(wr.yseq), wr.cand)
    assert np.array_equal(got["yseq"], words[L.E2E_NBEST].yseq.cpu().numpy())
    assert np.array_equal(got["lengths"], ref["lengths"])


# --------------------------------------------------------------------------- 5. graph replay
def test_validate_words_graph_replay():
    """validate_words with a WordAccuracyMeter and valid_rows captured as ONE hipGraph after a warm-up on the capture stream:
    replays on two other batches (clips, gold words and valid_rows copied into the static tensors) leave the counters of the
    eager calls, and the returned words are the eager ones bit for bit.  Gold words: the clip's own word, its second
    candidate, or another word, so that all three counters differ."""
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    from sbl_for_multilingual_lip_reading_amd.transformer.metrics import WordAccuracyMeter
    shape, Wn, W = "beam_varied", 257, 8
    g, m = _model(shape, L.e2e_pick(shape, Wn, W, False)[0])
    lex = Lexicon(L.e2e_words(shape, Wn, W, False), device=DEV, vocab=m.decoder.n_tgt_vocab)
    x = B.case_clips(g)
    batches = [x.to(DEV), (x.flip(0) * 0.5).to(DEV)]
    rows = [torch.tensor([3], dtype=torch.int32, device=DEV), torch.tensor([4], dtype=torch.int32, device=DEV)]
    run = lambda xs, gold, vr, meter: m.validate_words(xs, gold, lex, meter, valid_rows=vr, beam_size=W, nbest=3)      # noqa: E731
    with torch.no_grad():
        first = [m.recognize_words(b, lex, beam_size=W, nbest=3) for b in batches]
        golds = []
        for r in first:
            gold = r.word.clone()
            gold[1] = r.cand[1, 1].long()                 # among the n-best, not the best
            gold[2] = (r.word[2] + 1) % Wn if int((r.cand[2] == (r.word[2] + 1) % Wn).sum()) == 0 else -5
            golds.append(gold)
        eager = WordAccuracyMeter(device=DEV)
        eager_res = [run(b, gd, vr, eager) for b, gd, vr in zip(batches, golds, rows)]
        torch.cuda.synchronize()
        xs, gs, vs = batches[0].clone(), golds[0].clone(), rows[0].clone()
        meter = WordAccuracyMeter(device=DEV)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            run(xs, gs, vs, meter)       # warm-up on the capture stream (builds the meter's buffers)
        torch.cuda.synchronize()
        meter.reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            res = run(xs, gs, vs, meter)
        meter.reset()
        for b, gd, vr, ref in zip(batches, golds, rows, eager_res):
            xs.copy_(b)
            gs.copy_(gd)
            vs.copy_(vr)
            graph.replay()
            torch.cuda.synchronize()
            for a, c in zip(res, ref):
                assert torch.equal(a, c)
    assert torch.equal(meter.acc, eager.acc)
    n, ok, among = eager.acc.tolist()
    assert n == 7 and 0 < ok < among <= n, eager.acc.tolist()
    assert not torch.equal(eager_res[0].score, eager_res[1].score)


# --------------------------------------------------------------------------- 6. guards
def test_guards_and_the_unconstrained_path():
    """A lexicon of another vocab or eos, a lexicon on another device and decode_max_len != 0 with a lexicon raise
    SblHipError; beam_search_lex(lexicon=None) returns what beam_search returned before: the reference fixture, bit for bit
    the result of beam_search."""
    from sbl_for_multilingual_lip_reading_amd import _lib
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    g = load_golden("beam_varied.npz")
    c = B.beam_config(g)
    m = gpu_model(g, train=False)
    lp = B.log_prior(g).to(DEV)
    V = c["vocab"]
    with torch.no_grad():
        enc, _ = m._encode(B.case_clips(g).to(DEV))
        for lex, kw in ((Lexicon([[5, 6]], device=DEV, vocab=V - 1), {}), (Lexicon([[5, 6]], device=DEV, vocab=V, eos_id=2), {}),
                        (Lexicon([[5, 6]], device="cpu", vocab=V), {}), (Lexicon([[5, 6]], device=DEV, vocab=V), dict(decode_max_len=5))):
            with pytest.raises(_lib.SblHipError):
                m.decoder.beam_search_lex(enc, 3, lexicon=lex, **kw)
        with pytest.raises(_lib.SblHipError):
            m.decoder.recognize_words(enc, Lexicon([[5, 6]], device="cpu", vocab=V))
        a = _got(m.decoder.beam_search_lex(enc, c["W"], c["nbest"], c["decode_max_len"], lp, None))
        b = _got(m.decoder.beam_search(enc, c["W"], c["nbest"], c["decode_max_len"], lp))
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["yseq"], g["yseq"]) and np.array_equal(a["lengths"], g["lengths"]) and np.array_equal(a["n_hyps"], g["n_hyps"])
    assert np.abs(a["scores"] - g["scores"]).max() <= B.score_tol(c["maxlen"])
