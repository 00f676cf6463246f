"""GPU checks of ragged clips in the single-direction baseline: the step attention with a key count per K/V
entry against float64 and, bit for bit, against the entry without counts; the beam tail and finish with a per-clip last step
against the numpy restatement and, with full counts, against the entries without; the model against the reference's fixtures
(tests/golden/ragged_s2s_*.npz) and the restatement on unseen salts; the cross-path equalities; hipGraph replay with the
lengths overwritten in place; and the training plumbing."""
import numpy as np
import pytest
import torch

from conftest import load_golden, maxdiff
import beam_oracle as B
import lex_beam_oracle as L
import ragged_s2s_oracle as R
import seq2seq_oracle as S
from test_seq2seq_gpu import gpu_model, precision  # noqa: F401  (precision is a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEG = float("-inf")
H = 8


# --------------------------------------------------------------------------- 1. step attention with key counts
def _attn_ref(q, k, v, counts, W):
    """float64 softmax(q K^T / 8) V over the first clamp(count, 0, T) rows of the row's clip; no visible key: 0."""
    Sn, T = q.shape[0], k.shape[1]
    out = torch.zeros(Sn, H * 64, dtype=torch.float64)
    for b in range(Sn):
        n = min(max(int(counts[b // W]), 0), T)
        if n:
            qh = q[b].double().view(H, 1, 64)
            kh = k[b // W, :n].double().view(n, H, 64).transpose(0, 1)
            vh = v[b // W, :n].double().view(n, H, 64).transpose(0, 1)
            out[b] = (torch.softmax(qh @ kh.transpose(1, 2) / 8.0, -1) @ vh).reshape(H * 64)
    return out


@pytest.mark.parametrize("slots", [False, True], ids=["decode", "slots"])
@pytest.mark.parametrize("T", [7, 29, 64])
def test_attn_step_len_kernel(T, slots):
    """B = 5 rows (slots: S = 6 = 2 clips x W = 3, three launches), H = 8, over the hoisted (clips, T, [K | V]) block.  Counts
    0, -1, 1, T, T + 3 and one in the middle: float64 within 5e-6 (the bound of test_decode_attn_step_kernel); every row
    bit-equal to the entry without counts at n_prev = its clamped count (0 keys: exact zeros); the same bits with zeros, NaN
    and 1e30 behind the counts; the sentinels around o and the K / V block untouched."""
    from sbl_for_multilingual_lip_reading_amd import ops
    W = 3 if slots else 1
    sets = [(0, T), (-1, 1), (T + 3, (T + 1) // 2)] if slots else [(0, -1, 1, T, T + 3), (T, (T + 1) // 2, 2, T - 1, 1)]
    nc = len(sets[0])
    Sn = nc * W
    gen = torch.Generator().manual_seed(10 * T + slots)
    q = torch.randn(Sn, H * 64, generator=gen)
    kv = torch.randn(nc, T, 2 * H * 64, generator=gen)
    qd = q.to(DEV)

    def run(kvd, counts=None, n_prev=T):
        full = torch.full((Sn + 2, H * 64 + 8), -7.0, device=DEV)
        out = full[1:-1, :H * 64]
        kw = {} if counts is None else dict(kv_len=torch.tensor(counts, dtype=torch.int32, device=DEV))
        if slots:
            ops.beam_attn_step(qd, None, None, kvd[:, :, :512], kvd[:, :, 512:], T, None, out, W, H, n_prev, False, **kw)
        else:
            ops.decode_attn_step(qd, None, None, kvd[:, :, :512], kvd[:, :, 512:], T, out, H, n_prev, False, **kw)
        torch.cuda.synchronize()
        full = full.cpu()
        assert bool((full[0] == -7).all() and (full[-1] == -7).all() and (full[:, H * 64:] == -7).all()), "sentinels around o"
        return full[1:-1, :H * 64].clone()

    for counts in sets:
        kvd = kv.to(DEV)
        got = run(kvd, counts)
        assert torch.equal(kvd.cpu(), kv)
        d = maxdiff(got, _attn_ref(q, kv[:, :, :512], kv[:, :, 512:], counts, W))
        print("attn_step_len T=%d slots=%d counts %s: max|d| %.2e (bound 5e-6)" % (T, slots, counts, d))
        assert d < 5e-6
        for n, l in enumerate(counts):          # bit-equal to the entry without counts called with n_prev = the count
            l = min(max(l, 0), T)
            rows = slice(n * W, (n + 1) * W)
            if l == 0:
                assert not got[rows].any()
            else:
                assert torch.equal(got[rows].view(torch.int32), run(kvd, None, l)[rows].view(torch.int32)), (counts, n)
        for poison in (0.0, float("nan"), 1e30):
            pk = kv.clone()
            for n, l in enumerate(counts):
                pk[n, min(max(l, 0), T):] = poison
            assert torch.equal(run(pk.to(DEV), counts).view(torch.int32), got.view(torch.int32)), (counts, poison)


# --------------------------------------------------------------------------- 2. tail and finish with a per-clip last step
def _pe():
    from sbl_for_multilingual_lip_reading_amd.transformer.module import PositionalEncoding
    return PositionalEncoding(512, max_len=64).pe[0]


def _snapshot(st, x_next):
    d = dict(score=st.score, last_tok=st.last_tok, anc0=st.anc[0], anc1=st.anc[1], hist_tok=st.hist_tok, hist_par=st.hist_par,
             hist_score=st.hist_score, hist_flag=st.hist_flag, end_score=st.end_score, end_ref=st.end_ref, end_count=st.end_count)
    if x_next is not None:
        d["x_next"] = x_next
    return {k: v.cpu().numpy().copy() for k, v in d.items()}


def _tail_setup(W, seed):
    V, eos = 48, 1
    rng = np.random.RandomState(seed)
    w = (rng.randn(V, 512) * 0.05).astype(np.float32)
    emb = rng.randn(V, 512).astype(np.float32)
    lp = (rng.randn(V, V) * 2).astype(np.float32)
    lp[rng.rand(V, V) < 0.3] = NEG
    lp[:, eos] = 1.0
    return V, eos, rng, w, emb, lp


@pytest.mark.parametrize("W", [1, 3])
def test_beam_tail_and_finish_len_kernels(W):
    """A whole search of maxlen = 6 steps on N = 3 clips, V = 48, clip_steps (1, 4, maxlen), with the state read back before
    every launch and held to lex_beam_oracle.tail_ref per clip (the one-node table = the unconstrained tail) with the clip's
    own maxlen: integers exact, scores 1e-5 (the bound of test_beam_tail_kernel).  Behind its last step a clip keeps nothing:
    flags 0, scores -inf, the ended count unchanged.  Then the finish: a hypothesis that ended at the clip's last step s has
    length s + 3, any other s + 2."""
    from sbl_for_multilingual_lip_reading_amd import ops
    N, maxlen, scale = 3, 6, 0.25
    V, eos, rng, w, emb, lp = _tail_setup(W, 77 + W)
    steps = (1, 4, maxlen)
    cs = torch.tensor(steps, dtype=torch.int32, device=DEV)
    wd, ed, lpd, ped = [torch.from_numpy(a).to(DEV) for a in (w, emb, lp)] + [_pe().to(DEV)]
    st = ops.BeamState(N, W, maxlen, 0, DEV)
    mask, first = [(1 << V) - 1], [0]
    forced = 0
    for step in range(maxlen):
        y = rng.randn(N * W, 512).astype(np.float32)
        score, last = st.score.cpu().numpy().reshape(-1), st.last_tok.cpu().numpy().reshape(-1)
        anc_old, count0 = st.anc[step % 2].cpu().numpy(), st.end_count.cpu().numpy().copy()
        x_next = torch.empty(N * W, 512, device=DEV) if step + 1 < maxlen else None
        ops.beam_tail(torch.from_numpy(y).to(DEV), wd, lpd, st, step, eos, ed, ped, scale, x_next=x_next, clip_steps=cs)
        torch.cuda.synchronize()
        tok, par, hs, flag = (t.cpu().numpy()[:, step] for t in st.history())
        for n in range(N):
            sl = slice(n * W, (n + 1) * W)
            ref = L.tail_ref(y[sl], w, lp, score[sl], last[sl], np.zeros(W, np.int32), mask, first, anc_old[sl] - n * W, step, steps[n],
                             eos, W)
            msg = "W=%d step %d clip %d" % (W, step, n)
            assert ref["gap"] > 1e-4, "test data: a near tie"
            assert np.array_equal(flag[n], ref["flag"][0]) and np.array_equal(tok[n], ref["tok"][0]), msg
            assert np.array_equal(par[n], ref["par"][0]), msg
            fin = ref["flag"][0] != 0
            assert np.all(hs[n][~fin] == NEG) and (not fin.any() or np.abs(hs[n][fin] - ref["score"][0][fin]).max() <= 1e-5), msg
            assert int(st.end_count[n]) == (0 if step == 0 else count0[n]) + len(ref["ended"][0]), msg
            if step >= steps[n]:
                assert not flag[n].any() and bool((st.score[n] == NEG).all()), msg
            if step == steps[n] - 1:
                assert np.all(flag[n][fin] == 2) and bool((st.score[n] == NEG).all()), msg
                forced += int((tok[n][fin] != eos).sum())
    assert forced > 0, "no hypothesis was ended by its clip's last step"
    yseq, lengths, scores, n_hyps = (t.cpu().numpy() for t in ops.beam_finish(st, 2, eos, clip_steps=cs))
    er, es = st.end_ref.cpu().numpy(), st.end_score.cpu().numpy()
    for n in range(N):
        E = int(st.end_count[n])
        order = sorted(range(E), key=lambda e: -es[n, e])[:2]          # stable
        assert n_hyps[n] == len(order)
        for k, e in enumerate(order):
            s = er[n, e] // W
            assert s < steps[n] and lengths[n, k] == (s + 3 if s == steps[n] - 1 else s + 2) and scores[n, k] == es[n, e]
            assert yseq[n, k, 0] == 0 and np.all(yseq[n, k, s + 2:] == eos)


@pytest.mark.parametrize("W", [1, 3])
def test_full_clip_steps_are_the_tail_and_finish_without(W):
    """clip_steps = maxlen for every clip (and above it: clamped): every output of every step and the finish's four
    results equal sbl_beam_tail / sbl_beam_finish bit for bit."""
    from sbl_for_multilingual_lip_reading_amd import ops
    N, maxlen, scale = 3, 6, 0.25
    V, eos, rng, w, emb, lp = _tail_setup(W, 5 + W)
    wd, ed, lpd, ped = [torch.from_numpy(a).to(DEV) for a in (w, emb, lp)] + [_pe().to(DEV)]
    cs = torch.tensor([maxlen, maxlen + 9, maxlen], dtype=torch.int32, device=DEV)
    base, rag = ops.BeamState(N, W, maxlen, 0, DEV), ops.BeamState(N, W, maxlen, 0, DEV)
    for st in (base, rag):
        st.anc.fill_(-7)
        for t in st.history() + (st.end_ref,):
            t.fill_(-7)
        st.end_score.fill_(-7.0)
    for step in range(maxlen):
        y = torch.from_numpy(rng.randn(N * W, 512).astype(np.float32)).to(DEV)
        xa, xb = ((torch.full((N * W, 512), -7.0, device=DEV) for _ in range(2)) if step + 1 < maxlen else (None, None))
        ops.beam_tail(y, wd, lpd, base, step, eos, ed, ped, scale, x_next=xa)
        ops.beam_tail(y, wd, lpd, rag, step, eos, ed, ped, scale, x_next=xb, clip_steps=cs)
        torch.cuda.synchronize()
        a, b = _snapshot(base, xa), _snapshot(rag, xb)
        for k in a:
            assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), "W=%d step %d: %s" % (W, step, k)
    assert int(base.end_count.sum()) > 0
    for a, b in zip(ops.beam_finish(base, 2, eos), ops.beam_finish(rag, 2, eos, clip_steps=cs)):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------- 3. the model against the fixtures
def _lens(g, device=True):
    lens = [int(l) for l in g["lengths"]]
    return torch.tensor(lens, dtype=torch.int32, device=DEV) if device else lens


def _greedy_with_logits(m, x, lens):
    """recognize with the lengths, the logits of every step taken from sbl_decode_tail's optional output."""
    from sbl_for_multilingual_lip_reading_amd import ops
    logits, tail = [], ops.decode_tail

    def spy(y, w, ys, step, emb, pe, scale, x_next=None, logits_=None):
        logits.append(torch.empty(y.size(0), w.size(0), device=y.device))
        tail(y, w, ys, step, emb, pe, scale, x_next=x_next, logits=logits[-1])

    ops.decode_tail = spy
    try:
        with torch.no_grad():
            ys = m.recognize(x, input_lengths=lens)
    finally:
        ops.decode_tail = tail
    return ys, torch.stack(logits, 1)


def _check_greedy(m, g, x, ref, tag):
    lengths = [int(l) for l in g["lengths"]]
    T = x.shape[1]
    ys, logits = _greedy_with_logits(m, x.to(DEV), lengths)
    with torch.no_grad():
        enc, _ = m._encode(x.to(DEV), _lens(g))
    ys, logits, enc = ys.cpu().numpy(), logits.cpu().numpy(), enc.cpu().numpy()
    valid = np.arange(T)[None, :] < np.array(lengths)[:, None]
    d_log = np.abs(np.where(valid[:, :, None], logits - ref["logits"], 0.0)).max()
    d_enc = np.abs(enc - ref["enc"]).max()
    print("%s: max|dlogit| %.2e max|denc| %.2e (bound 1e-3)" % (tag, d_log, d_enc))
    assert np.array_equal(ys, ref["tokens"]), tag
    assert d_log < 1e-3 and d_enc < 1e-3
    for n, l in enumerate(lengths):
        assert not enc[n, l:].any() and np.all(ys[n, l + 1:] == 1)
    return ys


def test_greedy_matches_reference_fixture(precision):  # noqa: F811
    g = load_golden("ragged_s2s_small.npz")
    m = gpu_model(g, train=False)
    x = torch.from_numpy(g["clips"])
    _check_greedy(m, g, x, g, "ragged_s2s_small/" + precision)
    with torch.no_grad():          # without the lengths the padding is attended to: the fixture's other tokens
        assert np.array_equal(m.recognize(x.to(DEV)).cpu().numpy(), g["tokens_padded"])


def test_greedy_matches_oracle_on_unseen_inputs(precision):  # noqa: F811
    case = "ragged_s2s_small"
    g, x, ref = R.oracle_case(case, R.UNSEEN_SALTS[case])
    _check_greedy(gpu_model(g, train=False), g, x, ref, "%s salt %d/%s" % (case, R.UNSEEN_SALTS[case], precision))


def _got(res):
    out = dict(yseq=res.yseq, lengths=res.lengths, scores=res.scores, n_hyps=res.n_hyps)
    out.update(zip(("hist_tok", "hist_par", "hist_score", "hist_flag"), res.history))
    return {k: v.cpu().numpy() for k, v in out.items()}


def _beam(m, g, x, lens, **kw):
    c = R.config(g)
    with torch.no_grad():
        enc, _ = m._encode(x.to(DEV), lens)
        res = m.decoder.beam_search_len(enc, lens, c["beam_size"], c["nbest"], c["decode_max_len"], B.log_prior(g).to(DEV), **kw)
    torch.cuda.synchronize()
    return _got(res)


def _check_beam(got, ref, lengths, T, tag):
    why = lambda: "%s: %s" % (tag, B.first_divergence(got, ref))      # noqa: E731
    d = np.abs(np.where(np.isfinite(ref["scores"]), got["scores"] - ref["scores"], 0.0)).max()
    print("%s: max|dscore| %.2e (bound %.0e)" % (tag, d, B.score_tol(T)))
    assert np.array_equal(got["n_hyps"], ref["n_hyps"]), why()
    assert np.array_equal(got["lengths"], ref["lengths"]), why()
    assert np.array_equal(got["yseq"], ref["yseq"]), why()
    assert np.array_equal(np.isfinite(got["scores"]), np.isfinite(ref["scores"])) and d <= B.score_tol(T), why()
    assert np.array_equal(got["hist_flag"], ref["hist_flag"]), why()
    for n, l in enumerate(lengths):          # behind its last step a clip keeps nothing
        assert not got["hist_flag"][n, l:].any() and np.all(got["hist_score"][n, l:] == NEG)
        assert np.all(got["hist_flag"][n, l - 1][got["hist_flag"][n, l - 1] != 0] == 2)


def test_beam_matches_reference_fixture(precision):  # noqa: F811
    g = load_golden("ragged_s2s_beam.npz")
    c = R.config(g)
    m = gpu_model(g, train=False)
    x = torch.from_numpy(g["clips"])
    ref = {k: g[k] for k in ("yseq", "scores", "n_hyps", "hist_tok", "hist_par", "hist_score", "hist_flag")}
    ref["lengths"] = g["hyp_lengths"]
    got = _beam(m, g, x, _lens(g))
    _check_beam(got, ref, c["lengths"], c["T"], "ragged_s2s_beam/" + precision)
    with torch.no_grad():
        enc, _ = m._encode(x.to(DEV), _lens(g))
    assert float(np.abs(enc.cpu().numpy() - g["enc"]).max()) < 1e-3
    assert np.array_equal(_beam(m, g, x, None)["yseq"][:, 0], g["yseq_padded"])


def test_beam_matches_oracle_on_unseen_inputs(precision):  # noqa: F811
    case = "ragged_s2s_beam"
    g, x, ref = R.oracle_case(case, R.UNSEEN_SALTS[case])
    c = R.config(g)
    _check_beam(_beam(gpu_model(g, train=False), g, x, _lens(g)), ref, c["lengths"], c["T"],
                "%s salt %d/%s" % (case, R.UNSEEN_SALTS[case], precision))


# --------------------------------------------------------------------------- 4. cross-path equalities
def _lexicon(g):
    """Forty random words of 1..4 tokens over the fixture's vocabulary."""
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    V = int(g["meta"][2])
    rng = np.random.RandomState(3)
    words = sorted({tuple(int(t) for t in rng.randint(2, V, size=rng.randint(1, 5))) for _ in range(40)})
    lex = Lexicon(words, device=DEV, vocab=V, sos_id=0, eos_id=1)
    lex.trie()          # built before any capture
    return lex


def _all_paths(m, g, x, lens, lex, enc=None):
    """Every decode path with lengths -> dict of host arrays.  enc: decode these encoder rows instead of encoding x."""
    c = R.config(g)
    lp = B.log_prior(g).to(DEV) if "freq" in g else None
    W, nb = c.get("beam_size", 3), c.get("nbest", 2)
    d = m.decoder
    with torch.no_grad():
        if enc is None:
            enc, _ = m._encode(x.to(DEV), m._lengths(x, lens))
        out = dict(greedy=d.recognize_beam(enc, encoder_input_lengths=lens),
                   recompute=d.recognize_beam(enc, cached=False, encoder_input_lengths=lens))
        for name, res in (("beam", d.beam_search_len(enc, lens, W, nb, 0, lp)), ("beam_len5", d.beam_search_len(enc, lens, W, nb, 5, lp)),
                          ("lex", d.beam_search_len(enc, lens, W, nb, 0, lp, lex))):
            out.update({name + "." + k: v for k, v in _got(res).items()})
        wr = d.recognize_words_len(enc, lens, lex, W, nb, lp)
        out.update(word=wr.word, word_score=wr.score)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), "%s: %s" % (what, k)


def test_cross_path_equalities(precision):  # noqa: F811
    """A host list and a device tensor give the same bits on every path; full lengths as a device tensor give the bits of no
    lengths; the cached greedy decode gives the tokens of the prefix recompute under the explicit mask; and 1e4 x noise in
    the encoder rows behind the clips' ends gives what zeros give there, on every decode path."""
    g = load_golden("ragged_s2s_beam.npz")
    c = R.config(g)
    m = gpu_model(g, train=False)
    x = torch.from_numpy(g["clips"])
    lex = _lexicon(g)
    host, dev = _all_paths(m, g, x, list(c["lengths"]), lex), _all_paths(m, g, x, _lens(g), lex)
    _same(host, dev, "list vs tensor")
    assert np.array_equal(dev["greedy"], dev["recompute"]), "cached vs recompute"
    full = torch.full((c["B"],), c["T"], dtype=torch.int32, device=DEV)
    none = _all_paths(m, g, x, None, lex)
    _same(_all_paths(m, g, x, full, lex), none, "full lengths vs None")
    assert any(not np.array_equal(none[k], dev[k]) for k in ("greedy", "beam.yseq", "lex.yseq")), "the lengths change nothing"
    with torch.no_grad():
        enc, _ = m._encode(x.to(DEV), _lens(g))
    noisy = enc.clone()
    noise = torch.randn(enc.shape, generator=torch.Generator().manual_seed(1)).to(DEV) * 1e4
    for n, l in enumerate(c["lengths"]):
        noisy[n, l:] = noise[n, l:]
    _same(_all_paths(m, g, x, _lens(g), lex, enc=noisy), _all_paths(m, g, x, _lens(g), lex, enc=enc), "noise behind the ends")


# --------------------------------------------------------------------------- 5. graph replay
def _capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()          # warm-up on the capture stream
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = fn()
    return graph, out


def test_graph_replay_follows_the_lengths():
    """validate (greedy and beam) and validate_words_len captured once each with a device lengths tensor; the tensor is
    overwritten in place; one replay equals the eager run with the new lengths, which differs from the run with the old ones
    on every path (for the word search in its scores at least)."""
    from sbl_for_multilingual_lip_reading_amd.transformer.metrics import ErrorRateMeter, WordAccuracyMeter
    g = load_golden("ragged_s2s_beam.npz")
    c = R.config(g)
    m = gpu_model(g, train=False)
    lex = _lexicon(g)
    lp = B.log_prior(g).to(DEV)
    x = torch.from_numpy(g["clips"]).to(DEV)
    tgt = torch.randint(2, c["vocab"], (c["B"], 5), generator=torch.Generator().manual_seed(2)).to(DEV)
    gold = torch.zeros(c["B"], dtype=torch.long, device=DEV)
    first, second = _lens(g), torch.tensor([c["T"], 3, c["T"], 6], dtype=torch.int32, device=DEV)
    # the word search's result as one tensor: the n-best scores (the model's own log-probabilities, which follow the keys a clip
    # sees even where the words stay) and the token rows
    words = lambda res: torch.cat([res.score.flatten(), res.yseq.flatten().float()])      # noqa: E731
    calls = {
        "validate": lambda lens, mt: m.validate(x, tgt, mt, input_lengths=lens),
        "validate_beam": lambda lens, mt: m.validate(x, tgt, mt, beam_size=c["beam_size"], log_prior=lp, input_lengths=lens),
        "validate_words": lambda lens, mt: words(m.validate_words_len(x, lens, gold, lex, mt, beam_size=c["beam_size"], nbest=2, log_prior=lp)),
    }
    with torch.no_grad():
        for name, call in calls.items():
            meter = lambda: (WordAccuracyMeter if name == "validate_words" else ErrorRateMeter)(device=DEV)      # noqa: E731
            eager = [call(l, meter()).clone() for l in (first, second)]
            torch.cuda.synchronize()
            assert not torch.equal(eager[0], eager[1]), name + ": the two sets of lengths give the same result"
            static, mt = first.clone(), meter()
            graph, out = _capture(lambda: call(static, mt))
            static.copy_(second)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager[1]), name


# --------------------------------------------------------------------------- 6. training plumbing
def test_forward_passes_the_lengths_to_encoder_and_decoder():
    """Seq2SeqTransformer.forward(..., input_lengths) equals decoder(tgt, encoder(feats, lengths), lengths) composed by
    hand, and differs from the pass without lengths."""
    g = load_golden("s2s_varied.npz")
    c = S.case_config(g)
    m = gpu_model(g, train=False)
    x, tgt = S.case_inputs(g)
    x, tgt = x.to(DEV), tgt.to(DEV)
    lengths = [c["T"], 3, 1, c["T"] - 1]
    pred, gold = m(x, tgt, lengths)
    feats = m.lipreading(x.unsqueeze(1))
    enc, *_ = m.encoder(feats, lengths)
    want, wgold = m.decoder(tgt, enc, lengths)
    assert torch.equal(pred, want) and torch.equal(gold, wgold)
    assert pred.requires_grad and not torch.equal(pred, m(x, tgt)[0])
