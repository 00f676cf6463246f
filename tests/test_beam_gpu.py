"""GPU checks of the batched beam search (csrc/beam_step.hip, the slot instantiation of the step attention in
csrc/decode_step.hip, Seq2SeqDecoder.beam_search): the three kernels alone against
float64 / host restatements, the whole search against the reference's fixtures (tests/golden/beam_*.npz) and against the
plain-torch restatement (tests/beam_oracle.py) on unseen inputs, beam 1 against the greedy fixtures, hipGraph replay, and
the validate / recognize_nbest surface."""
import types

import numpy as np
import pytest
import torch

from conftest import load_golden, maxdiff
import beam_oracle as B
import seq2seq_oracle as S
from test_seq2seq_gpu import gpu_model, precision  # noqa: F401  (precision is a fixture)

pytestmark = pytest.mark.gpu
NEG = float("-inf")


# --------------------------------------------------------------------------- attention step
@pytest.mark.parametrize("Lcap", [32, 64])
@pytest.mark.parametrize("n_prev", [0, 1, 13, 63])
@pytest.mark.parametrize("W", [1, 3, 8])
def test_beam_attn_step_kernel(W, n_prev, Lcap):
    """Self-attention through a scrambled ancestry table against float64 (1e-5): key j of slot b is row j of slot anc[b][j];
    the new row lands in row n_prev of the slot's OWN cache and every other cache element is bit-identical afterwards.
    Cross mode: N * W slots read N caches.  n_prev = 63 is the last row of Lcap = 64; Lcap = 32 takes its own last row."""
    from sbl_for_multilingual_lip_reading_amd import ops
    n_prev = min(n_prev, Lcap - 1)
    N, H = 3, 8
    S_ = N * W
    gen = torch.Generator().manual_seed(1000 * W + 10 * n_prev + Lcap)
    q, kn, vn = (torch.randn(S_, H * 64, generator=gen) for _ in range(3))
    kc, vc = (torch.randn(S_, Lcap, H * 64, generator=gen) for _ in range(2))
    anc = torch.randint(0, S_, (S_, Lcap), generator=gen, dtype=torch.int32)
    qkv = torch.cat([q, kn, vn], 1).cuda()
    kd, vd, ad = kc.cuda(), vc.cuda(), anc.cuda()
    out = torch.empty(S_, H * 64, device="cuda")
    ops.beam_attn_step(qkv[:, :512], qkv[:, 512:1024], qkv[:, 1024:], kd, vd, Lcap, ad, out, W, H, n_prev, True)
    torch.cuda.synchronize()
    kr, vr = kc.clone(), vc.clone()
    kr[:, n_prev], vr[:, n_prev] = kn, vn
    assert torch.equal(kd.cpu(), kr) and torch.equal(vd.cpu(), vr) and torch.equal(ad.cpu(), anc)

    def ref(q_, k_, v_):          # k_, v_: (S, n, 512), the keys of every slot gathered
        qh = q_.double().view(S_, H, 1, 64)
        kh = k_.double().view(S_, -1, H, 64).transpose(1, 2)
        vh = v_.double().view(S_, -1, H, 64).transpose(1, 2)
        p = torch.softmax(qh @ kh.transpose(2, 3) / 8.0, -1)
        return (p @ vh).transpose(1, 2).reshape(S_, H * 64)

    j = torch.arange(n_prev)
    gk = torch.cat([kc[anc[:, :n_prev].long(), j], kn.unsqueeze(1)], 1)
    gv = torch.cat([vc[anc[:, :n_prev].long(), j], vn.unsqueeze(1)], 1)
    assert maxdiff(out, ref(q, gk, gv)) <= 1e-5
    # cross-attention: the hoisted (N, 29, [K | V]) block, slot b reads clip b // W
    n = 29
    kv = torch.randn(N, n, 2 * H * 64, generator=gen)
    kvd = kv.cuda()
    ops.beam_attn_step(qkv[:, :512], None, None, kvd[:, :, :512], kvd[:, :, 512:], n, None, out, W, H, n, False)
    torch.cuda.synchronize()
    rep = kv.repeat_interleave(W, 0)
    assert maxdiff(out, ref(q, rep[:, :, :512], rep[:, :, 512:])) <= 1e-5 and torch.equal(kvd.cpu(), kv)


@pytest.mark.parametrize("n_prev,append", [(0, True), (1, True), (63, True), (64, False)])
def test_beam_attn_step_with_one_slot_is_the_decode_attn_step(n_prev, append):
    """ops.beam_attn_step at W = 1 with the identity ancestry table against ops.decode_attn_step on the same seeded q, new
    K / V row and cache contents: outputs and caches bitwise equal.  The edges of Lcap = 64: an empty cache, one key, the
    last lane, and a full row without an append."""
    from sbl_for_multilingual_lip_reading_amd import ops
    nb, H, Lcap = 3, 8, 64
    gen = torch.Generator().manual_seed(64 * n_prev + append)
    qkv = torch.randn(nb, 3 * H * 64, generator=gen).cuda()
    kc, vc = (torch.randn(nb, Lcap, H * 64, generator=gen) for _ in range(2))
    anc = torch.arange(nb, dtype=torch.int32).unsqueeze(1).repeat(1, Lcap).cuda() if append else None
    new = (qkv[:, 512:1024], qkv[:, 1024:]) if append else (None, None)
    got = []
    for slots in (False, True):
        kd, vd = kc.cuda(), vc.cuda()
        out = torch.full((nb, H * 64), float("nan"), device="cuda")
        if slots:
            ops.beam_attn_step(qkv[:, :512], new[0], new[1], kd, vd, Lcap, anc, out, 1, H, n_prev, append)
        else:
            ops.decode_attn_step(qkv[:, :512], new[0], new[1], kd, vd, Lcap, out, H, n_prev, append)
        got.append((out, kd, vd))
    torch.cuda.synchronize()
    assert not bool(torch.isnan(got[0][0]).any())
    for a, b in zip(*got):
        assert torch.equal(a, b)
    assert append or (torch.equal(got[0][1].cpu(), kc) and torch.equal(got[0][2].cpu(), vc))


# --------------------------------------------------------------------------- tail
def tail_ref(y, w, lp, score, last, anc_old, step, maxlen, eos, emb, pe, scale, W):
    """float64 restatement of sbl_beam_tail for N clips -> dict of expected outputs (see include/sbl_hip.h)."""
    Sn, V = y.shape[0], w.shape[0]
    N = Sn // W
    logits = y.astype(np.float64) @ w.astype(np.float64).T
    m = logits.max(1, keepdims=True)
    local = logits - m - np.log(np.exp(logits - m).sum(1, keepdims=True))
    if lp is not None:
        local = local + lp.astype(np.float64)[last]
    out = dict(tok=np.full((N, W), eos, np.int32), par=np.tile(np.arange(W, dtype=np.int32), (N, 1)),
               score=np.full((N, W), -np.inf), flag=np.zeros((N, W), np.int32), ended=[[] for _ in range(N)],
               anc=np.zeros((Sn, step + 1), np.int32), gap=np.inf)
    for n in range(N):
        cand = [(score[n * W + r] + local[n * W + r, v], r, v) for r in range(W) for v in range(V) if score[n * W + r] > -np.inf]
        cand = sorted([c for c in cand if c[0] > -np.inf], key=lambda c: (-c[0], c[1], c[2]))
        for a, b in zip(cand[:W], cand[1:W + 1]):
            if a[0] != b[0]:
                out["gap"] = min(out["gap"], a[0] - b[0])
        for r, (sc, par, v) in enumerate(cand[:W]):
            end = v == eos or step == maxlen - 1
            out["tok"][n, r], out["par"][n, r], out["score"][n, r], out["flag"][n, r] = v, par, sc, 2 if end else 1
            if end:
                out["ended"][n].append((sc, step * W + r))
        for r in range(W):
            ps = n * W + out["par"][n, r]
            out["anc"][n * W + r, :step] = anc_old[ps, :step]
            out["anc"][n * W + r, step] = ps
    out["next_score"] = np.where(out["flag"] == 1, out["score"], -np.inf)
    out["x_next"] = emb.astype(np.float64)[out["tok"].reshape(-1)] * scale + pe[step + 1].astype(np.float64) if step + 1 < maxlen else None
    return out


@pytest.mark.parametrize("V,W", [(5, 1), (5, 3), (5, 5), (42, 1), (42, 3), (42, 16), (64, 1), (64, 3), (64, 16)])
def test_beam_tail_kernel(V, W):
    """Three launches on N = 3 clips against float64: step 0 (one live slot per clip, a stale ended count that the step
    resets), a middle step (dead slots; -inf prior entries; a clip with fewer finite candidates than W; a clip whose slots
    0 and 1 and whose classes 2 and 3 are exact copies, so the documented tie order decides; <eos> endings appended behind
    earlier records), and the last step (everything kept ends, a token that already is <eos> included).  Scores 1e-5,
    everything else exact; untouched history rows, ended records and ancestry columns keep their sentinel."""
    from sbl_for_multilingual_lip_reading_amd import ops
    from sbl_for_multilingual_lip_reading_amd.transformer.module import PositionalEncoding
    N, maxlen, eos, scale = 3, 6, 1, 0.25
    Sn = N * W
    rng = np.random.RandomState(100 * V + W)
    w = (rng.randn(V, 512) * 0.05).astype(np.float32)
    emb = rng.randn(V, 512).astype(np.float32)
    if V > 3:
        w[3] = w[2]
    lp = (rng.randn(V, V) * 2).astype(np.float32)
    lp[rng.rand(V, V) < 0.3] = NEG
    lp[:, eos] = 2.0                      # <eos> is always a strong candidate: endings at every step
    lp[:, 0] = NEG                        # nothing is followed by <sos>
    if V > 3:
        lp[:, 3] = lp[:, 2]
    lp[4 % V] = NEG
    lp[4 % V, [eos, V - 1]] = [2.0, 0.5]  # a row with two finite entries: fewer candidates than W
    lp[5 % V, eos] = 12.0
    pe = PositionalEncoding(512, max_len=64).pe[0].numpy()
    wd, ed, ped, lpd = (torch.from_numpy(a).cuda() for a in (w, emb, pe, lp))
    saw = set()
    for step in (0, 2, maxlen - 1):
        y = rng.randn(Sn, 512).astype(np.float32)
        score = (-rng.rand(Sn) * 10).astype(np.float32)
        last = rng.randint(2, V, Sn).astype(np.int32)
        counts = np.array([0, 2, 5], np.int32)
        if step == 0:
            score.reshape(N, W)[:, 1:] = NEG
            last[:] = 0
            counts[:] = 7
        else:
            score.reshape(N, W)[1, 1:] = NEG          # clip 1: one live slot ...
            last[W] = 4 % V                           # ... whose prior row has two finite entries
            if W > 1:                                 # clip 2: slot 1 is an exact copy of slot 0, and the two lead
                score[2 * W] = 20.0
                y[2 * W + 1], score[2 * W + 1], last[2 * W + 1] = y[2 * W], score[2 * W], last[2 * W]
            if step == maxlen - 1:
                last[0] = 5 % V                       # clip 0, slot 0: <eos> is by far the likeliest successor
            if W > 2:
                score[2] = NEG                        # clip 0: a dead slot between live ones
        anc_old = rng.randint(0, Sn, (Sn, maxlen)).astype(np.int32)
        ref = tail_ref(y, w, lp, score, last, anc_old, step, maxlen, eos, emb, pe, scale, W)
        assert ref["gap"] > 1e-4, "test data: a near tie that float32 may order either way"
        st = ops.BeamState(N, W, maxlen, 0, "cuda")
        st.score.copy_(torch.from_numpy(score).view(N, W))
        st.last_tok.copy_(torch.from_numpy(last).view(N, W))
        st.anc[step % 2].copy_(torch.from_numpy(anc_old))
        st.anc[1 - step % 2].fill_(-7)
        for t in st.history() + (st.end_ref,):
            t.fill_(-7)
        st.end_score.fill_(-7.0)
        st.end_count.copy_(torch.from_numpy(counts))
        x_next = torch.full((Sn, 512), -7.0, device="cuda") if step + 1 < maxlen else None
        yd = torch.from_numpy(y).cuda()
        ops.beam_tail(yd, wd, lpd, st, step, eos, ed, ped, scale, x_next=x_next)
        torch.cuda.synchronize()
        tok, par, hs, flag = (t.cpu().numpy() for t in st.history())
        msg = "V=%d W=%d step=%d" % (V, W, step)
        assert np.array_equal(flag[:, step], ref["flag"]), msg
        assert np.array_equal(tok[:, step], ref["tok"]) and np.array_equal(par[:, step], ref["par"]), msg
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
        assert np.array_equal(st.anc[step % 2].cpu().numpy(), anc_old), msg
        es, er, ec = st.end_score.cpu().numpy(), st.end_ref.cpu().numpy(), st.end_count.cpu().numpy()
        for n in range(N):
            c0 = 0 if step == 0 else int(counts[n])
            k = len(ref["ended"][n])
            assert ec[n] == c0 + k, msg
            assert np.all(er[n, :c0] == -7) and np.all(er[n, c0 + k:] == -7) and np.all(es[n, c0 + k:] == -7.0), msg
            assert er[n, c0:c0 + k].tolist() == [r for _, r in ref["ended"][n]], msg
            assert k == 0 or np.abs(es[n, c0:c0 + k] - np.array([s for s, _ in ref["ended"][n]])).max() <= 1e-5, msg
        if x_next is not None:
            assert maxdiff(x_next, ref["x_next"]) <= 1e-6, msg
        # what the data was built to exercise
        if (ref["flag"] == 2).any() and step < maxlen - 1:
            saw.add("eos ending")
        if step == maxlen - 1:
            assert np.all(ref["flag"][fin] == 2)
            if (ref["tok"][fin] == eos).any():
                saw.add("already eos at the last step")
        if step == 2 and W > 2:
            assert (ref["flag"][1] == 0).sum() == W - 2, "clip 1 offers two finite candidates"
            saw.add("fewer finite candidates than W")
        if step == 2 and W > 1:
            assert any(ref["score"][2, r] == ref["score"][2, r + 1] and ref["par"][2, r] == 0 and ref["par"][2, r + 1] == 1
                       for r in range(W - 1)), "clip 2: equal candidates of slots 0 and 1 are kept, slot 0 first"
            saw.add("parent tie")
        if step == 2 and V > 3:
            both = [(n, r) for n in range(N) for r in range(W - 1) if ref["flag"][n, r] and ref["tok"][n, r] == 2
                    and ref["tok"][n, r + 1] == 3 and ref["par"][n, r] == ref["par"][n, r + 1]]
            if both:
                saw.add("token tie")
    assert "eos ending" in saw and "already eos at the last step" in saw, saw
    if W > 2:
        assert {"fewer finite candidates than W", "parent tie"} <= saw, saw


def test_beam_tail_token_tie_order():
    """Classes 2 and 3 are exact copies and dominate: they are kept as ranks 0 and 1 in token order, from the lower parent
    first when two slots tie as well."""
    from sbl_for_multilingual_lip_reading_amd import ops
    from sbl_for_multilingual_lip_reading_amd.transformer.module import PositionalEncoding
    N, W, V, maxlen = 3, 4, 42, 6
    rng = np.random.RandomState(7)
    w = (rng.randn(V, 512) * 0.01).astype(np.float32)
    y = rng.randn(N * W, 512).astype(np.float32)
    y[:] = y[0]                              # every slot is the same row ...
    w[2] = w[3] = y[0] * 0.02                # ... and classes 2 and 3 win by far
    st = ops.BeamState(N, W, maxlen, 0, "cuda")
    st.score.fill_(-1.0)
    st.score[0, 1] = -0.5                    # clip 0: slot 1 is ahead, slots 0, 2, 3 tie
    pe = PositionalEncoding(512, max_len=64).pe[0].cuda()
    ops.beam_tail(torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda(), None, st, 1, 1, torch.from_numpy(w).cuda(), pe, 1.0,
                  x_next=torch.empty(N * W, 512, device="cuda"))
    tok, par, _, flag = (t.cpu().numpy()[:, 1] for t in st.history())
    assert tok.tolist() == [[2, 3, 2, 3]] * 3 and np.all(flag == 1)
    assert par.tolist() == [[1, 1, 0, 0], [0, 0, 1, 1], [0, 0, 1, 1]]


# --------------------------------------------------------------------------- finish
def test_beam_finish_kernel():
    """Equal scores keep their list order (the stable sort of decoder.py:240), a clip with fewer ended hypotheses than nbest
    reports n_hyps and pads with length 0 / -inf / <eos>, and the back-trace follows the parents through the history."""
    from sbl_for_multilingual_lip_reading_amd import ops
    N, W, maxlen, nbest, eos = 2, 3, 4, 3, 1
    st = ops.BeamState(N, W, maxlen, 0, "cuda")
    tok = np.array([[[5, 6, 7], [8, 1, 9], [10, 11, 1], [12, 13, 14]]] * 2, np.int32)          # [step][rank]
    par = np.array([[[0, 0, 0], [2, 0, 1], [0, 2, 0], [1, 0, 0]]] * 2, np.int32)
    # clip 0: five ended entries; -0.5 twice and -1.0 twice.  ref = step * W + rank
    es = np.full((N, W * maxlen), 99.0, np.float32)
    er = np.zeros((N, W * maxlen), np.int32)
    es[0, :5] = [-1.0, -0.5, -1.0, -0.5, -2.0]
    er[0, :5] = [1 * W + 1, 2 * W + 2, 3 * W + 0, 3 * W + 1, 3 * W + 2]
    es[1, 0], er[1, 0] = -3.0, 3 * W + 2
    st.hist_tok.copy_(torch.from_numpy(tok))
    st.hist_par.copy_(torch.from_numpy(par))
    st.end_score.copy_(torch.from_numpy(es))
    st.end_ref.copy_(torch.from_numpy(er))
    st.end_count.copy_(torch.tensor([5, 1], dtype=torch.int32))
    yseq, lengths, scores, n_hyps = (t.cpu().numpy() for t in ops.beam_finish(st, nbest, eos))

    def trace(s, r):
        out = []
        for t in range(s, -1, -1):
            out.append(int(tok[0, t, r]))
            r = int(par[0, t, r])
        seq = [0] + out[::-1] + ([eos] if s == maxlen - 1 else [])
        return seq + [eos] * (maxlen + 2 - len(seq)), len(seq)

    want = [trace(2, 2), trace(3, 1), trace(1, 1)]          # -0.5 (first in the list), -0.5, then the first -1.0
    assert n_hyps.tolist() == [3, 1] and scores[0].tolist() == [-0.5, -0.5, -1.0]
    assert yseq[0].tolist() == [s for s, _ in want] and lengths[0].tolist() == [n for _, n in want]
    assert want[0][0][:4] == [0, 7, 8, 1] and want[1][1] == maxlen + 2
    assert yseq[1, 0].tolist() == trace(3, 2)[0] and lengths[1].tolist() == [maxlen + 2, 0, 0]
    assert scores[1, 0] == -3.0 and np.all(scores[1, 1:] == NEG) and np.all(yseq[1, 1:] == eos)


# --------------------------------------------------------------------------- the whole search
def _got(res):
    out = dict(yseq=res.yseq, lengths=res.lengths, scores=res.scores, n_hyps=res.n_hyps)
    out.update(zip(("hist_tok", "hist_par", "hist_score", "hist_flag"), res.history))
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(got, ref, maxlen, tag):
    """Tokens, lengths and n_hyps exact, scores within 1e-3 * maxlen; a failure names the first diverging (clip, step)."""
    why = lambda: "%s: %s" % (tag, B.first_divergence(got, ref))      # noqa: E731
    d = np.abs(np.where(np.isfinite(ref["scores"]), got["scores"] - ref["scores"], 0.0)).max()
    print("%s: max|dscore| %.2e (bound %.0e)" % (tag, d, B.score_tol(maxlen)))
    assert np.array_equal(got["n_hyps"], ref["n_hyps"]), why()
    assert np.array_equal(got["lengths"], ref["lengths"]), why()
    assert np.array_equal(got["yseq"], ref["yseq"]), why()
    assert np.array_equal(np.isfinite(got["scores"]), np.isfinite(ref["scores"])) and d <= B.score_tol(maxlen), why()


def _search(g, m):
    c = B.beam_config(g)
    lp = B.log_prior(g)
    with torch.no_grad():
        enc, _ = m._encode(B.case_clips(g).cuda())
        res = m.decoder.beam_search(enc, c["W"], c["nbest"], c["decode_max_len"], None if lp is None else lp.cuda())
    torch.cuda.synchronize()
    return c, _got(res)


@pytest.mark.parametrize("case", B.CASES)
def test_beam_search_matches_reference_fixture(case, precision):  # noqa: F811
    g = load_golden(case + ".npz")
    c, got = _search(g, gpu_model(g, train=False))
    assert got["yseq"].dtype == np.int64 and got["yseq"].shape == (c["B"], c["nbest"], c["maxlen"] + 2)
    _check(got, g, c["maxlen"], "%s/%s" % (case, precision))


@pytest.mark.parametrize("case", sorted(B.UNSEEN_SALTS))
def test_beam_search_matches_oracle_on_unseen_inputs(case, precision):  # noqa: F811
    """Other weights and clips than any fixture's; test_beam_cpu.py holds these salts to the margin floor."""
    g, ref = B.oracle_case(case, B.UNSEEN_SALTS[case])
    c, got = _search(g, gpu_model(g, train=False))
    _check(got, ref, c["maxlen"], "%s salt %d/%s" % (case, B.UNSEEN_SALTS[case], precision))


@pytest.mark.parametrize("case", ["s2s_small", "s2s_varied", "s2s_full"])
def test_beam_one_without_prior_is_the_greedy_decode(case, precision):  # noqa: F811
    """beam_size = 1, no prior: the greedy fixture's tokens up to and including the first <eos> (beyond it the greedy row
    goes on, the beam hypothesis has ended)."""
    g = load_golden(case + ".npz")
    m = gpu_model(g, train=False)
    x, _ = S.case_inputs(g)
    with torch.no_grad():
        enc, _ = m._encode(x.cuda())
        res = m.decoder.beam_search(enc, 1)
    yseq, lengths = res.yseq.cpu().numpy()[:, 0], res.lengths.cpu().numpy()[:, 0]
    T = g["tokens"].shape[1] - 1
    for n, row in enumerate(g["tokens"]):
        first = [i for i in range(1, T + 1) if row[i] == 1]
        end = first[0] if first else T
        assert yseq[n, :end + 1].tolist() == row[:end + 1].tolist(), (case, n)
        assert lengths[n] == (end + 1 if first and end < T else T + 2), (case, n)
    assert res.n_hyps.tolist() == [1] * len(yseq)


def test_beam_graph_replay():
    """beam_search captured as ONE hipGraph: two replays with different encoder outputs equal the eager calls bit for bit
    (n-best, scores and the whole history), with the prior and early endings of beam_varied."""
    g = load_golden("beam_varied.npz")
    c = B.beam_config(g)
    m = gpu_model(g, train=False)
    lp = B.log_prior(g).cuda()
    x = B.case_clips(g)
    run = lambda e: m.decoder.beam_search(e, c["W"], c["nbest"], c["decode_max_len"], lp)      # noqa: E731
    with torch.no_grad():
        encs = [m._encode(x.cuda())[0].clone(), m._encode((x.flip(0) * 0.5).cuda())[0].clone()]
        eager = [_got(run(e)) for e in encs]
        torch.cuda.synchronize()
        static = encs[0].clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            run(static)       # warm-up on the capture stream
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            res = run(static)
        for e, ref in zip(encs, eager):
            static.copy_(e)
            graph.replay()
            torch.cuda.synchronize()
            got = _got(res)
            for k in ref:
                assert np.array_equal(got[k], ref[k]), k
    _check(eager[0], g, c["maxlen"], "beam_varied eager")
    assert not np.array_equal(eager[0]["scores"], eager[1]["scores"])


def test_validate_with_beam_and_recognize_nbest():
    """validate(beam_size=W) leaves the meter with the counters of update_single on the fixture's 1-best; recognize_nbest
    returns the reference's per-clip [{'score', 'yseq'}]."""
    from sbl_for_multilingual_lip_reading_amd.transformer.metrics import ErrorRateMeter
    g = load_golden("beam_varied.npz")
    c = B.beam_config(g)
    m = gpu_model(g, train=False)
    lp = B.log_prior(g).cuda()
    x = B.case_clips(g).cuda()
    tgt = torch.full((c["B"], 13), -1, dtype=torch.long)
    for n in range(c["B"]):          # the fixture's 1-best without <sos> / <eos>, one token replaced: distances are not all 0
        ids = [t for t in g["yseq"][n, 0, :g["lengths"][n, 0]].tolist() if t > 1][:13]
        if ids:
            ids[-1] = 2 + (ids[-1] - 1) % (c["vocab"] - 2)
        tgt[n, :len(ids)] = torch.tensor(ids, dtype=torch.long)
    meter, want = ErrorRateMeter(device="cuda:0"), ErrorRateMeter(device="cuda:0")
    with torch.no_grad():
        ys = m.validate(x, tgt.cuda(), meter, beam_size=c["W"], log_prior=lp)
        want.update_single(torch.from_numpy(g["yseq"][:, 0].copy()).cuda(), tgt.cuda())
        hyps = m.recognize_nbest(x, None, types.SimpleNamespace(beam_size=c["W"], nbest=c["nbest"], decode_max_len=0), log_prior=lp)
    assert np.array_equal(ys.cpu().numpy(), g["yseq"][:, 0])
    assert torch.equal(meter.acc, want.acc) and int(meter.acc.sum()) > 0
    assert isinstance(hyps, list) and len(hyps) == c["B"]
    for n, hs in enumerate(hyps):
        assert len(hs) == int(g["n_hyps"][n])
        for k, h in enumerate(hs):
            assert sorted(h) == ["score", "yseq"] and isinstance(h["score"], float)
            assert h["yseq"] == g["yseq"][n, k, :g["lengths"][n, k]].tolist()
            assert abs(h["score"] - float(g["scores"][n, k])) <= B.score_tol(c["maxlen"])
