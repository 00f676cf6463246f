"""GPU checks of the beam search of the bidirectional SBL decoder (csrc/pair_beam.hip, sbl_attention_seg_grouped_fwd,
Decoder.beam_search): the tail kernel alone against a float64 restatement and its documented tie order, the grouped
cross-attention bit for bit against sbl_attention_seg_fwd on repeated K/V, beam 1 against the reference's greedy fixtures,
the whole search against the plain-torch restatement's checker (tests/sbl_beam_oracle.py: follow) on unseen weights, the
returned scores against a teacher-forced pass through Decoder.forward, and hipGraph replay."""
import numpy as np
import pytest
import torch

import sbl_beam_oracle as PB
from conftest import load_golden
from sbl_for_multilingual_lip_reading_amd import detfill

pytestmark = pytest.mark.gpu
NEG = float("-inf")
DEV = "cuda:0"


@pytest.fixture(params=["f32", "bf16x6"])
def precision(request):
    from sbl_for_multilingual_lip_reading_amd import ops
    ops.set_matmul_precision(request.param)
    yield request.param
    ops.set_matmul_precision("f32")


# --------------------------------------------------------------------------- tail kernel
def _tail_case(W, step, dead, seed):
    """Random state of N = 3 clips before step `step` -> (numpy inputs, the PairBeamState after one launch, ys_old copies)."""
    from sbl_for_multilingual_lip_reading_amd import ops
    N, V, maxlen, eos = 3, 58, 16, 1
    S = N * W
    rng = np.random.RandomState(seed)
    y = [rng.randn(S, 512).astype(np.float32) for _ in (0, 1)]
    w = [(rng.randn(V, 512) * 0.05).astype(np.float32) for _ in (0, 1)]
    score = (-rng.rand(N, W) * 10).astype(np.float32)
    sdir = (-rng.rand(N, W, 2) * 10).astype(np.float32)
    if step == 0:
        score[:, 1:], sdir[:, 1:] = NEG, NEG
        score[:, 0], sdir[:, 0] = 0.0, 0.0
    if dead is not None:
        score[dead], sdir[dead] = NEG, NEG
    ys_old = np.full((2, S, maxlen + 1), eos, np.int64)
    ys_old[:, :, 0] = 0
    ys_old[:, :, 1:step + 1] = rng.randint(2, V, (2, S, step))
    st = ops.PairBeamState(N, W, maxlen, 0, eos, DEV)
    st.score.copy_(torch.from_numpy(score))
    st.score_dir.copy_(torch.from_numpy(sdir))
    st.ys.fill_(-7)
    st.ys[:, step % 2].copy_(torch.from_numpy(ys_old))
    for t in st.history()[:3]:
        t.fill_(-7)
    st.hist_score.fill_(-7.0)
    ops.pair_beam_tail(*(torch.from_numpy(a).to(DEV) for a in y + w), st, step)
    torch.cuda.synchronize()
    return dict(N=N, V=V, W=W, eos=eos, maxlen=maxlen, y=y, w=w, score=score, sdir=sdir, ys_old=ys_old), st


@pytest.mark.parametrize("W", [1, 2, 5, 16])
@pytest.mark.parametrize("step", [0, 3])
def test_pair_beam_tail_kernel(W, step):
    """N = 3, V = 58.  Step 0: only slot 0 of every clip is live.  Step 3: random live slots, for W > 1 with one dead slot in
    clip 1.  Against float64 through the keep / score rule of sbl_beam_oracle.follow with the 1e-5 of test_beam_tail_kernel:
    the kept candidates are distinct, the totals fall with the rank, every score (total and per direction) is the float64
    score of that candidate within 1e-5, and no kept candidate is more than 2e-5 below the float64 W-th best.  The new
    prefixes are ys_old[parent] || token || eos exactly, the history row equals the outputs and every other row is untouched."""
    tol = 1e-5
    dead = (1, W - 1) if step and W > 1 else None
    c, st = _tail_case(W, step, dead, 100 * W + step)
    N, V, eos = c["N"], c["V"], c["eos"]
    lp = []
    for d in (0, 1):
        logits = c["y"][d].astype(np.float64) @ c["w"][d].astype(np.float64).T
        m = logits.max(1, keepdims=True)
        lp.append((logits - m - np.log(np.exp(logits - m).sum(1, keepdims=True))).reshape(N, W, V))
    tok_l, tok_r, par, hs = (t.cpu().numpy() for t in st.history())
    new = st.ys[:, 1 - step % 2].cpu().numpy()
    got_score, got_dir = st.score.cpu().numpy(), st.score_dir.cpu().numpy()
    assert np.array_equal(st.ys[:, step % 2].cpu().numpy(), c["ys_old"])
    other = [i for i in range(c["maxlen"]) if i != step]
    assert all(np.all(a[:, other] == -7) for a in (tok_l, tok_r, par, hs))
    assert np.array_equal(hs[:, step].view(np.int32), got_score.view(np.int32))
    worst = 0.0
    for n in range(N):
        live = [s for s in range(W) if c["score"][n, s] > NEG]
        total = {(s, a, b): float(c["score"][n, s]) + lp[0][n, s, a] + lp[1][n, s, b] for s in live for a in range(V) for b in range(V)}
        best = sorted(total.values(), reverse=True)
        n_keep = min(W, len(best))
        assert [r for r in range(W) if got_score[n, r] > NEG] == list(range(n_keep)), (n, got_score[n])
        seen = set()
        for r in range(W):
            msg = "W=%d step=%d clip %d rank %d" % (W, step, n, r)
            p, a, b = int(par[n, step, r]), int(tok_l[n, step, r]), int(tok_r[n, step, r])
            if r >= n_keep:
                assert (p, a, b) == (r, eos, eos) and np.all(got_dir[n, r] == NEG), msg
            else:
                assert (p, a, b) in total and (p, a, b) not in seen, msg
                seen.add((p, a, b))
                worst = max(worst, abs(got_score[n, r] - total[p, a, b]))
                assert abs(got_score[n, r] - total[p, a, b]) <= tol, msg
                assert r == 0 or got_score[n, r] <= got_score[n, r - 1], msg
                assert total[p, a, b] >= best[n_keep - 1] - 2 * tol, msg
                assert abs(got_dir[n, r, 0] - (float(c["sdir"][n, p, 0]) + lp[0][n, p, a])) <= tol, msg
                assert abs(got_dir[n, r, 1] - (float(c["sdir"][n, p, 1]) + lp[1][n, p, b])) <= tol, msg
            for d, t in ((0, a), (1, b)):
                want = np.full(c["maxlen"] + 1, eos, np.int64)
                want[:step + 1] = c["ys_old"][d, n * W + p, :step + 1]
                want[step + 1] = t
                assert np.array_equal(new[d, n * W + r], want), msg
    print("W=%d step=%d: max|dscore| %.2e (bound %.0e)" % (W, step, worst, tol))
    if step == 0:
        assert np.all(par[:, 0] == 0)
    elif dead is not None:
        assert not np.any(par[dead[0], step] == dead[1])


def test_pair_beam_tail_tie_order():
    """Every slot reads the same rows and head rows 2, 3 (l2r) and 5, 6 (r2l) are exact copies that dominate: the four
    candidates of a slot tie bit for bit and are kept in (l2r rank, r2l rank) order, the lower parent first among equal
    slots; clip 0's slot 1 is ahead of its other slots."""
    from sbl_for_multilingual_lip_reading_amd import ops
    N, W, V = 2, 6, 58
    rng = np.random.RandomState(7)
    y = [np.tile(rng.randn(1, 512).astype(np.float32), (N * W, 1)) for _ in (0, 1)]
    w = [(rng.randn(V, 512) * 0.01).astype(np.float32) for _ in (0, 1)]
    w[0][2] = w[0][3] = y[0][0] * 0.02
    w[1][5] = w[1][6] = y[1][0] * 0.02
    st = ops.PairBeamState(N, W, 16, 0, 1, DEV)
    st.score.fill_(-1.0)
    st.score_dir.fill_(-0.5)
    st.score[0, 1] = -0.5
    ops.pair_beam_tail(*(torch.from_numpy(a).to(DEV) for a in y + w), st, 1)
    tok_l, tok_r, par, hs = (t.cpu().numpy()[:, 1] for t in st.history())
    assert tok_l.tolist() == [[2, 2, 3, 3, 2, 2]] * 2 and tok_r.tolist() == [[5, 6, 5, 6, 5, 6]] * 2
    assert par.tolist() == [[1, 1, 1, 1, 0, 0], [0, 0, 0, 0, 1, 1]]
    assert len(set(hs[0, :4].tolist())) == 1 and len(set(hs[1].tolist())) == 1 and hs[0, 4] == hs[1, 0]


# --------------------------------------------------------------------------- grouped cross-attention
@pytest.mark.parametrize("L,T,drop", [(1, 29, 0.0), (5, 29, 0.0), (16, 29, 0.0), (17, 29, 0.0), (5, 40, 0.0), (5, 29, 0.3), (5, 40, 0.3)])
def test_grouped_cross_attention_is_bit_identical(L, T, drop):
    """N = 2 clips, W = 3 slots, H = 8: sequence s attends to the K/V of clip s // W.  Bit-identical to sbl_attention_seg_fwd
    on K/V repeated W-fold, for the one-wavefront kernel (L <= 16, T <= 32), its query-tile form (L = 17) and the workgroup
    kernel (T = 40); the K/V block is read in place as columns of a wider buffer and is not written.  With dropout (a module
    left in train mode) the masks are those of that call too."""
    from sbl_for_multilingual_lip_reading_amd import ops
    N, W, H = 2, 3, 8
    B, HD = N * W, H * 64
    gen = torch.Generator().manual_seed(100 * L + T)
    q = torch.randn(B * L, 3 * HD, generator=gen).to(DEV)           # the q columns of a fused projection, ldq = 3 * HD
    kv = torch.randn(N * T, 2 * HD, generator=gen).to(DEV)
    kv0 = kv.clone()
    rep = kv.view(N, T, 2 * HD).repeat_interleave(W, 0).reshape(B * T, 2 * HD).contiguous()
    seg, nseg = ops._segs((L,))
    s = torch.cuda.current_stream().cuda_stream
    o_ref, o = torch.full((B * L, HD), -7.0, device=DEV), torch.full((B * L, HD), -7.0, device=DEV)
    p = torch.empty(H * B * L * T, device=DEV)
    seed_t = torch.tensor([1234567], dtype=torch.int64, device=DEV)
    seed = seed_t.data_ptr() if drop else None
    ops.call("sbl_attention_seg_fwd", q.data_ptr(), 3 * HD, rep.data_ptr(), 2 * HD, rep[:, HD:].data_ptr(), 2 * HD, o_ref.data_ptr(), HD,
             p.data_ptr(), 0, None, B, H, seg, nseg, T, 0.125, drop, seed, 5, s)
    ops.call("sbl_attention_seg_grouped_fwd", q.data_ptr(), 3 * HD, kv.data_ptr(), 2 * HD, kv[:, HD:].data_ptr(), 2 * HD, o.data_ptr(), HD,
             B, H, seg, nseg, T, W, 0.125, drop, seed, 5, s)
    torch.cuda.synchronize()
    assert torch.equal(o, o_ref) and torch.equal(kv, kv0) and not bool((o == -7.0).any())
    if drop:
        return
    # and it is an attention: float64 on one (sequence, head)
    b, h = B - 1, 3
    qh = q[b * L:(b + 1) * L, h * 64:(h + 1) * 64].double().cpu()
    kh = kv.view(N, T, 2 * HD)[b // W, :, h * 64:(h + 1) * 64].double().cpu()
    vh = kv.view(N, T, 2 * HD)[b // W, :, HD + h * 64:HD + (h + 1) * 64].double().cpu()
    ref = torch.softmax(qh @ kh.T / 8.0, -1) @ vh
    assert float((o[b * L:(b + 1) * L, h * 64:(h + 1) * 64].double().cpu() - ref).abs().max()) <= 1e-5


# --------------------------------------------------------------------------- the whole search
def _transformer(n_enc, n_dec, gains):
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    from sbl_for_multilingual_lip_reading_amd.transformer.transformer import Transformer
    m = Transformer(Encoder(512, n_enc, 8, 64, 64, 512, 2048), Decoder(0, 1, 58, 512, n_dec, 8, 64, 64, 512, 2048), None)
    m.load_state_dict({k: (v if k.endswith("pe") else torch.from_numpy(detfill.fill_value(k, tuple(v.shape), 0, gains).copy()))
                       for k, v in m.state_dict().items()})
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    m.visual_frontend.frontend_dropout_p = 0.0
    return m.to(DEV)


@pytest.mark.parametrize("tag", ["small", "full", "varied"])
def test_beam_one_equals_the_reference_greedy_fixture(tag, precision):
    """Transformer.recognize_nbest(x, 1) spells the tokens the REFERENCE decoded (tests/golden/recognize_*.npz); on the small
    case validate(beam_size=1) leaves the meter as the greedy validate does."""
    from sbl_for_multilingual_lip_reading_amd.transformer.metrics import ErrorRateMeter
    g = load_golden("recognize_%s.npz" % tag)
    m = _transformer(int(g["n_enc"]), int(g["n_dec"]), str(g["gains"]) if "gains" in g.files else None)
    m = m.train() if "train_bn" in g.files and int(g["train_bn"]) else m.eval()      # "varied": batch-statistics BatchNorm
    x, l2r, r2l = (torch.from_numpy(a).to(DEV) for a in detfill.synthetic_batch(int(g["B"]), int(g["T"]), int(g["H"]), int(g["W"]), int(g["salt"])))
    with torch.no_grad():
        res = m.recognize_nbest(x, 1)
        assert res.ys_l2r.shape == (int(g["B"]), 1, 17) and res.ys_l2r.dtype == torch.int64 and res.scores.shape == (int(g["B"]), 1)
        assert np.array_equal(res.ys_l2r[:, 0].cpu().numpy(), g["ys_l2r"]) and np.array_equal(res.ys_r2l[:, 0].cpu().numpy(), g["ys_r2l"])
        assert bool(torch.isfinite(res.scores).all()) and float((res.scores_dir.sum(-1) - res.scores).abs().max()) < 1e-3
        if tag == "small":
            a, b = ErrorRateMeter(device=DEV), ErrorRateMeter(device=DEV)
            m.validate(x, l2r, r2l, a, beam_size=1)
            m.validate(x, l2r, r2l, b)
            assert torch.equal(a.acc, b.acc) and int(a.acc.sum()) > 0


def test_validate_with_a_wide_beam_scores_the_best_pair(precision):
    """validate(beam_size = 3) on the varied fixture's model returns and scores rank 0 of the 3-wide search: the meter equals
    one updated with recognize_nbest(x, 3, 3)'s best pair, which is not its rank-1 pair."""
    from sbl_for_multilingual_lip_reading_amd.transformer.metrics import ErrorRateMeter
    g = load_golden("recognize_varied.npz")
    m = _transformer(int(g["n_enc"]), int(g["n_dec"]), str(g["gains"])).eval()
    x, l2r, r2l = (torch.from_numpy(a).to(DEV) for a in detfill.synthetic_batch(int(g["B"]), int(g["T"]), int(g["H"]), int(g["W"]), int(g["salt"])))
    got, want = ErrorRateMeter(device=DEV), ErrorRateMeter(device=DEV)
    with torch.no_grad():
        res = m.recognize_nbest(x, 3, 3)
        ys_l, ys_r = m.validate(x, l2r, r2l, got, beam_size=3)
        want.update(res.ys_l2r[:, 0].contiguous(), res.ys_r2l[:, 0].contiguous(), l2r, r2l)
    assert torch.equal(ys_l, res.ys_l2r[:, 0]) and torch.equal(ys_r, res.ys_r2l[:, 0])
    assert bool((res.scores[:, 0] >= res.scores[:, 1]).all()) and not (torch.equal(res.ys_l2r[:, 0], res.ys_l2r[:, 1])
                                                                       and torch.equal(res.ys_r2l[:, 0], res.ys_r2l[:, 1]))
    assert torch.equal(got.acc, want.acc) and int(got.acc.sum()) > 0


_DECODERS = {}


def _decoder(salt):
    """A 2-layer SBL decoder on the GPU with the oracle's "varied" weights of `salt`, and those weights."""
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    if salt not in _DECODERS:
        sd = PB.decoder_state_dict(2, salt)
        dec = Decoder(0, 1, 58, 512, 2, 8, 64, 64, 512, 2048, dropout=0.0)
        own = dec.state_dict()
        dec.load_state_dict({k: (v if k.endswith("pe") else sd["decoder." + k]) for k, v in own.items()})
        _DECODERS[salt] = (dec.to(DEV).eval(), sd)
    return _DECODERS[salt]


def _host(res):
    out = dict(ys_l2r=res.ys_l2r, ys_r2l=res.ys_r2l, scores=res.scores, scores_dir=res.scores_dir)
    out.update(zip(("tok_l", "tok_r", "par", "score"), res.history))
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


@pytest.mark.parametrize("W,salt", [(3, 7), (5, 8)])
def test_search_passes_the_oracles_checker_and_rescoring(W, salt, precision):
    """A 2-layer decoder, N = 3 clips of 8 encoder rows, weights and inputs no fixture uses.  sbl_beam_oracle.follow passes on
    the GPU's history; the returned n-best are the last step's slots; and - an independent pin through code that is checked
    against the reference - feeding the returned pairs back teacher-forced through Decoder.forward gives, as the summed
    log-softmax at the hypothesis tokens, scores_dir within 16 * 1e-3 per direction."""
    dec, sd = _decoder(salt)
    N, nbest = 3, W - 1
    enc = PB.encoder_output(N, 8, salt)
    with torch.no_grad():
        got = _host(dec.beam_search(enc.to(DEV), W, nbest))
    hist = tuple(got[k] for k in ("tok_l", "tok_r", "par", "score"))
    st = PB.follow(hist, sd, enc, 2, W)
    print("W=%d salt %d %s: max|dscore| %.2e, max deficit %.2e (2 tol at the last step %.1e)" % (
        W, salt, precision, st["max_dscore"], st["max_deficit"], 2 * PB.step_tol(15)))
    assert got["ys_l2r"].shape == (N, nbest, 17) and got["scores"].shape == (N, nbest) and got["scores_dir"].shape == (N, nbest, 2)
    assert np.array_equal(got["ys_l2r"], st["ys_l2r"][:, :nbest]) and np.array_equal(got["ys_r2l"], st["ys_r2l"][:, :nbest])
    assert np.array_equal(got["scores"], got["score"][:, 15, :nbest]) and np.all(np.isfinite(got["scores"]))
    assert np.abs(got["scores_dir"].sum(-1) - got["scores"]).max() <= 1e-3
    assert len({tuple(r) for r in got["ys_l2r"].reshape(-1, 17).tolist()}) > N      # the beam holds different l2r hypotheses
    # teacher-forced rescoring
    ys = [torch.from_numpy(got[k].reshape(N * nbest, 17)).to(DEV) for k in ("ys_l2r", "ys_r2l")]
    dec.coins_host = [False] * 16
    try:
        with torch.no_grad():
            pl, _, pr, _ = dec(ys[0][:, 1:16].contiguous(), ys[1][:, 1:16].contiguous(), enc.repeat_interleave(nbest, 0).to(DEV), [8] * (N * nbest))
    finally:
        dec.coins_host = None
    for d, pred in enumerate((pl, pr)):
        lp = torch.log_softmax(pred.double(), -1).gather(2, ys[d][:, 1:].unsqueeze(-1)).squeeze(-1).sum(1).cpu().numpy()
        diff = np.abs(lp.reshape(N, nbest) - got["scores_dir"][:, :, d]).max()
        print("  rescoring direction %d: max|d| %.2e (bound %.1e)" % (d, diff, 16 * PB.LOGIT_TOL))
        assert diff <= 16 * PB.LOGIT_TOL


def test_search_graph_replay(precision):
    """beam_search captured as ONE hipGraph, in both matmul modes: two replays on different encoder outputs equal the eager
    calls bit for bit (n-best, scores and the whole history)."""
    dec, _ = _decoder(7)
    W, nbest = 3, 2
    encs = [PB.encoder_output(3, 8, s).to(DEV) for s in (21, 22)]
    with torch.no_grad():
        eager = [_host(dec.beam_search(e, W, nbest)) for e in encs]
        torch.cuda.synchronize()
        static = encs[0].clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            dec.beam_search(static, W, nbest)       # warm-up on the capture stream
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            res = dec.beam_search(static, W, nbest)
        for e, ref in zip(encs, eager):
            static.copy_(e)
            graph.replay()
            torch.cuda.synchronize()
            got = _host(res)
            for k in ref:
                assert np.array_equal(got[k], ref[k]), k
    assert not np.array_equal(eager[0]["scores"], eager[1]["scores"])


def test_sbl_decode_launch_sequences(monkeypatch):
    """The library calls of recognize_beam, beam_search(W = 2), beam_search_lex(W = 2) and recognize_words(shortlist = 2) on a
    2-layer SBL decoder, N = 2 clips of T = 3 encoder rows, in order.  Every decode hoists the cross-attention K/V (one GEMM per
    layer and direction) and then runs one stage per step: the two embeddings, per layer the 11 launches of either direction's
    layer (QKV GEMM, self-attention, fc GEMM, add + LayerNorm, Q GEMM, cross-attention, fc GEMM, add + LayerNorm, the two FFN
    GEMMs, add + LayerNorm) and the fusion, then the two gathers of the rows the heads read; a step ends with the two head GEMMs
    and the two arg-max launches (greedy) or with the search's tail.  recognize_words follows the greedy decode with the
    shortlist, a second K/V hoist, ONE stage over all 16 prefixes and the scoring tail.  The W slots (K candidates) of a clip
    share its K/V through the grouped cross-attention.  With encoder_input_lengths every cross-attention, grouped or not,
    is sbl_attention_seg_len_fwd and nothing else changes."""
    from sbl_for_multilingual_lip_reading_amd import _lib, ops
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    n_layers, N, T, W, steps = 2, 2, 3, 2, 16
    torch.manual_seed(11)
    dec = Decoder(0, 1, 58, 512, n_layers, 8, 64, 64, 512, 2048, dropout=0.0).to(DEV).eval()
    enc = torch.randn(N, T, 512, device=DEV)
    lex = Lexicon([[5, 9], [7], [9, 5]], device=DEV, vocab=58, sos_id=0, eos_id=1)
    assert lex.max_len == 2
    lex.pair_trie()
    names = []
    monkeypatch.setattr(ops, "call", lambda name, *a: names.append(name) or _lib.call(name, *a))
    gemm, ln, seg = "sbl_gemm_f32", "sbl_add_layernorm_fwd", "sbl_attention_seg_fwd"
    grouped, seg_len = "sbl_attention_seg_grouped_fwd", "sbl_attention_seg_len_fwd"

    def stage(cross):
        layer = [gemm, seg, gemm, ln, gemm, cross, gemm, ln, gemm, gemm, ln]
        return 2 * ["sbl_embed_pe_seg_fwd"] + n_layers * (2 * layer + ["sbl_fusion_seg_fwd"]) + 2 * ["sbl_gather_last_fwd"]

    hoist = 2 * n_layers * [gemm]

    def expected(cross, cross_w):
        """cross: the cross-attention entry of one sequence per clip, cross_w: that of several slots per clip."""
        greedy = hoist + steps * (stage(cross) + 2 * [gemm] + 2 * ["sbl_argmax_select"])
        return dict(
            greedy=greedy,
            beam=hoist + steps * (stage(cross_w) + ["sbl_pair_beam_tail"]),
            beam_lex=hoist + (lex.max_len + 1) * (stage(cross_w) + ["sbl_pair_beam_tail_lex"]),
            words=greedy + ["sbl_lexicon_shortlist"] + hoist + stage(cross_w) + ["sbl_pair_score_tail"])

    lengths = torch.tensor([3, 1], dtype=torch.int32, device=DEV)
    for lens, want in ((None, expected(seg, grouped)), (lengths, expected(seg_len, seg_len))):
        runs = dict(
            greedy=lambda: dec.recognize_beam(enc, encoder_input_lengths=lens),
            beam=lambda: dec.beam_search(enc, W, encoder_input_lengths=lens),
            beam_lex=lambda: dec.beam_search_lex(enc, lex, W, encoder_input_lengths=lens),
            words=lambda: dec.recognize_words(enc, lex, shortlist=2, encoder_input_lengths=lens))
        for key, run in runs.items():
            del names[:]
            run()
            assert names == want[key], (key, lens is not None)
    torch.cuda.synchronize()
