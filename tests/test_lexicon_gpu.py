"""GPU checks of the closed-vocabulary word decode (csrc/lexicon.hip, Decoder.score_pairs / recognize_words,
Transformer.validate_words, metrics.WordAccuracyMeter): the shortlist kernel in exact integers against the brute-force
restatement (tests/lexicon_oracle.py), the tail kernel alone against float64, score_pairs against the plain-torch decoder of
tests/sbl_beam_oracle.py and against the merged beam search's own totals, the whole decode margin-free, hipGraph replay, and
the meter's counters."""
import numpy as np
import pytest
import torch

import lexicon_cases as LC
import lexicon_oracle as LO
import sbl_beam_oracle as PB
from sbl_for_multilingual_lip_reading_amd import detfill

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEG = float("-inf")


@pytest.fixture(params=["f32", "bf16x6"])
def precision(request):
    from sbl_for_multilingual_lip_reading_amd import ops
    ops.set_matmul_precision(request.param)
    yield request.param
    ops.set_matmul_precision("f32")


def _lexicon(words):
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    return Lexicon(words, device=DEV)


# --------------------------------------------------------------------------- 1. shortlist kernel
_SHORT = {}


def _short_case(H, Wn):
    """Seeded lexicon and hypotheses of N = 3 clips (tests/lexicon_cases.py), and the restatement's full ranking, once per
    (H, Wn): the shortlist for K is its first K entries."""
    if (H, Wn) not in _SHORT:
        words = LC.make_lexicon(Wn, 10 + Wn)
        ys_l, ys_r = LC.make_hyps(words, H, 20 + H + Wn)
        _SHORT[H, Wn] = (words, ys_l, ys_r, LO.shortlist(ys_l, ys_r, words, min(Wn, 16)))
    return _SHORT[H, Wn]


@pytest.mark.parametrize("Wn,K", [(1, 1), (5, 1), (5, 5), (257, 1), (257, 5), (257, 16), (1000, 1), (1000, 5), (1000, 16)])
@pytest.mark.parametrize("H", [1, 3])
def test_shortlist_kernel_equals_the_restatement(H, Wn, K):
    """N = 3.  Wn = 1000 is one word per lane, 257 leaves most lanes without one, 1 and 5 force K = Wn; the inputs hold an
    empty and a 16-token hypothesis, a 15-token word, identical lexicon rows, D = 0 hits and (H = 3) equal D from two
    hypotheses.  Every output is an integer and must be equal.  The hypotheses are passed as the strided views that
    beam_search returns (rows of a wider table)."""
    from sbl_for_multilingual_lip_reading_amd import ops
    words, ys_l, ys_r, full = _short_case(H, Wn)
    Kf = min(Wn, 16)      # the shortlist for K is the first K ranks of the one for min(Wn, 16)
    per_slot = lambda v: v.reshape((3, Kf) + v.shape[1:])[:, :K].reshape((3 * K,) + v.shape[1:])      # noqa: E731
    want = {k: per_slot(v) if k in ("cand_ys_l2r", "cand_ys_r2l", "n_pos") else v[:, :K] for k, v in full.items()}
    wide = [torch.full((3, H + 2, 17), 5, dtype=torch.int64, device=DEV) for _ in (0, 1)]
    for t, y in zip(wide, (ys_l, ys_r)):
        t[:, :H] = torch.from_numpy(y).to(DEV)
    got = ops.lexicon_shortlist(wide[0][:, :H], wide[1][:, :H], _lexicon(words).packed, K, LC.SOS, LC.EOS, LC.IGN)
    for k in want:
        g = getattr(got, k)
        assert g.dtype == (torch.int64 if k.startswith("cand_ys") else torch.int32) and g.shape == want[k].shape, k
        assert np.array_equal(g.cpu().numpy(), want[k]), (k, H, Wn, K)
    if H == 1:      # (N, 17) rows, as recognize returns them
        flat = ops.lexicon_shortlist(torch.from_numpy(ys_l[:, 0]).to(DEV), torch.from_numpy(ys_r[:, 0]).to(DEV), _lexicon(words).packed, K,
                                     LC.SOS, LC.EOS, LC.IGN)
        assert all(torch.equal(a, b) for a, b in zip(flat, got))


@pytest.mark.parametrize("Wn", [1025, 20000])
def test_shortlist_kernel_with_several_words_per_lane(Wn):
    """The kernel's 1024 lanes stride over the words, so up to 1000 words every lane holds one key at most.  Wn = 1025 gives
    one lane two words, 20000 gives every lane 19 or 20 (more than its 16-entry list keeps), and the lexicon
    (lexicon_cases.make_strided_lexicon) repeats words 1 and 0, exact or slightly edited, at every index 1 + 1024 k and 1024 k:
    lane 1 owns 14 of the 16 best words of clip 2 and lane 0 all 16 of clip 1, so the sorted insert displaces entries and the
    selection pops one lane's list round after round, with word indices far above 1024.  N = 3, H = 3, K = 16; exact."""
    from sbl_for_multilingual_lip_reading_amd import ops
    words = LC.make_strided_lexicon(Wn, 10 + Wn)
    ys_l, ys_r = LC.make_hyps(words, 3, 23 + Wn)
    want = LO.shortlist(ys_l, ys_r, words, 16)
    lane = want["cand"] % 1024
    assert max(int((lane[n] == k).sum()) for n in range(3) for k in (0, 1)) >= (14 if Wn == 20000 else 2) and want["cand"].max() >= 1024
    got = ops.lexicon_shortlist(torch.from_numpy(ys_l).to(DEV), torch.from_numpy(ys_r).to(DEV), _lexicon(words).packed, 16, LC.SOS, LC.EOS, LC.IGN)
    for k in want:
        assert np.array_equal(getattr(got, k).cpu().numpy(), want[k]), (k, Wn)


# --------------------------------------------------------------------------- 2. tail kernel
def _tail(y, w, ys, n_pos, G):
    from sbl_for_multilingual_lip_reading_amd import ops
    S = ys[0].shape[0]
    out = (torch.full((S, 16, 2), -7.0, device=DEV), torch.full((S, 2), -7.0, device=DEV), torch.full((S,), -7.0, device=DEV),
           torch.full((S // G,), -7, dtype=torch.int32, device=DEV))
    ops.pair_score_tail(*(torch.from_numpy(a).to(DEV) for a in y + w), *(torch.from_numpy(a).to(DEV) for a in ys),
                        None if n_pos is None else torch.tensor(n_pos, dtype=torch.int32, device=DEV), G, *out)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _tail_ref(y, w, ys, n_pos):
    """float64: logp (S, 16, 2), score_dir (S, 2), score (S), and the full log-softmax lp[d] (16, S, V)."""
    S = ys[0].shape[0]
    n_pos = [16] * S if n_pos is None else n_pos
    lp = []
    for d in (0, 1):
        logits = (y[d].astype(np.float64) @ w[d].astype(np.float64).T).reshape(16, S, -1)
        m = logits.max(-1, keepdims=True)
        lp.append(logits - m - np.log(np.exp(logits - m).sum(-1, keepdims=True)))
    logp = np.zeros((S, 16, 2))
    for s in range(S):
        for i in range(n_pos[s]):
            logp[s, i] = (lp[0][i, s, ys[0][s, i + 1]], lp[1][i, s, ys[1][s, i + 1]])
    return logp, logp.sum(1), logp.sum((1, 2)), lp


@pytest.mark.parametrize("S,G", [(1, 1), (5, 5), (24, 8)])
@pytest.mark.parametrize("npos", ["mixed", "one", None])
def test_pair_score_tail_kernel(S, G, npos):
    """Random rows of LayerNorm scale, V = 58, random tokens; n_pos cycles through 1, 16 and values between ("mixed"), is 1
    everywhere, or NULL (16 everywhere).  Every logp within 1e-5 of float64 (the bound test_pair_beam_tail_kernel holds the
    same arithmetic to), score_dir within n_pos * 1e-5, score within 2 * n_pos * 1e-5, entries at i >= n_pos exactly 0, and
    the float64 score of the chosen slot within 2 * 2 * 16 * 1e-5 of the float64 maximum of its group."""
    tol, V = 1e-5, 58
    rng = np.random.RandomState(100 * S + G)
    y = [rng.randn(16 * S, 512).astype(np.float32) for _ in (0, 1)]
    w = [(rng.randn(V, 512) * 0.05).astype(np.float32) for _ in (0, 1)]
    ys = [rng.randint(0, V, (S, 17)).astype(np.int64) for _ in (0, 1)]
    n_pos = {"mixed": ([1, 16, 7, 2, 15, 9, 16, 1] * 3)[:S], "one": [1] * S, None: None}[npos]
    logp, sdir, score, best = _tail(y, w, ys, n_pos, G)
    rl, rd, rs, _ = _tail_ref(y, w, ys, n_pos)
    np_ = np.array([16] * S if n_pos is None else n_pos)
    print("S=%d G=%d n_pos=%s: max|dlogp| %.2e (bound %.0e), max|dscore| %.2e" % (S, G, npos, np.abs(logp - rl).max(), tol, np.abs(score - rs).max()))
    assert np.abs(logp - rl).max() <= tol
    assert np.all(np.abs(sdir - rd) <= np_[:, None] * tol) and np.all(np.abs(score - rs) <= 2 * np_ * tol)
    for s in range(S):
        assert np.all(logp[s, np_[s]:] == 0.0) and np.all(logp[s, :np_[s]] < 0.0)
    assert best.dtype == np.int32 and best.shape == (S // G,)
    for g in range(S // G):
        grp = rs[g * G:(g + 1) * G]
        assert 0 <= best[g] < G and grp[best[g]] >= grp.max() - 2 * 2 * 16 * tol
        assert score[g * G + best[g]] == score[g * G:(g + 1) * G].max()      # ... and it is the largest of the device's own scores


def test_pair_score_tail_exact_tie_goes_to_the_lower_rank():
    """S = G = 5: slot 1 carries the float64 arg-max token at every step (the largest score by a wide margin) and slot 3 is an
    exact copy of it - rows, tokens and n_pos - so the two scores are equal bit for bit and rank 1 is chosen.  A token outside
    the classes has no probability: that slot's score is -inf and it is never chosen."""
    S, G, V = 5, 5, 58
    rng = np.random.RandomState(77)
    y = [rng.randn(16 * S, 512).astype(np.float32) for _ in (0, 1)]
    w = [(rng.randn(V, 512) * 0.05).astype(np.float32) for _ in (0, 1)]
    ys = [rng.randint(0, V, (S, 17)).astype(np.int64) for _ in (0, 1)]
    for d in (0, 1):
        y[d].reshape(16, S, 512)[:, 3] = y[d].reshape(16, S, 512)[:, 1]
    lp = _tail_ref(y, w, ys, None)[3]
    for d in (0, 1):
        ys[d][1, 1:] = lp[d][:, 1].argmax(-1)
        ys[d][3] = ys[d][1]
    ys[0][0, 4] = V      # no class
    logp, sdir, score, best = _tail(y, w, ys, [12] * S, G)
    assert score[1] == score[3] and np.array_equal(logp[1], logp[3]) and score[1] > max(score[0], score[2], score[4])
    assert best.tolist() == [1]
    assert score[0] == NEG and sdir[0, 0] == NEG and np.isfinite(sdir[0, 1]) and logp[0, 3, 0] == NEG


# --------------------------------------------------------------------------- 3. score_pairs against the oracle
_DECODERS = {}


def _decoder(n_layers, salt):
    """An n_layers + n_layers SBL decoder on the GPU with the oracle's "varied" weights of `salt`, and those weights."""
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    if (n_layers, salt) not in _DECODERS:
        sd = PB.decoder_state_dict(n_layers, salt)
        dec = Decoder(0, 1, 58, 512, n_layers, 8, 64, 64, 512, 2048, dropout=0.0)
        own = dec.state_dict()
        dec.load_state_dict({k: (v if k.endswith("pe") else sd["decoder." + k]) for k, v in own.items()})
        _DECODERS[n_layers, salt] = (dec.to(DEV).eval(), sd)
    return _DECODERS[n_layers, salt]


_PAIRS = {}


def _pairs_case(n_layers, group):
    """N = 2 clips of 5 encoder rows; random words of lengths 1, 7 and 15 as candidate rows (n_pos = length + 1), and the
    oracle's scores of them, once per (n_layers, group)."""
    if (n_layers, group) not in _PAIRS:
        _, sd = _decoder(n_layers, 11)
        rng = np.random.RandomState(31 * n_layers + group)
        lens = {1: [15, 1], 3: [1, 7, 15, 15, 7, 1]}[group]
        words = [rng.randint(2, 58, size=c).tolist() for c in lens]
        ys = [torch.tensor([LC.row(w[::-1] if d else w) for w in words], dtype=torch.int64) for d in (0, 1)]
        n_pos = [c + 1 for c in lens]
        enc = PB.encoder_output(2, 5, 40 + group)
        _PAIRS[n_layers, group] = (enc, ys, n_pos, LO.pair_scores(sd, enc, ys[0], ys[1], n_pos, group, n_layers))
    return _PAIRS[n_layers, group]


@pytest.mark.parametrize("group", [1, 3])
@pytest.mark.parametrize("n_layers", [1, 2])
def test_score_pairs_against_the_oracle(n_layers, group, precision):
    """Every logp within the project's logit tolerance of the plain-torch decoder run prefix by prefix, the scores within that
    tolerance once per direction and position (2 * LOGIT_TOL * n_pos, as step_tol uses it), zeros behind n_pos, and best = the
    arg-max of the device's scores."""
    dec, _ = _decoder(n_layers, 11)
    enc, ys, n_pos, (rl, rd, rs) = _pairs_case(n_layers, group)
    got = dec.score_pairs(enc.to(DEV), ys[0].to(DEV), ys[1].to(DEV), torch.tensor(n_pos, dtype=torch.int32, device=DEV), group=group)
    logp, sdir, score, best = got.logp.cpu().numpy(), got.score_dir.cpu().numpy(), got.score.cpu().numpy(), got.best.cpu().numpy()
    np_ = np.array(n_pos)
    print("%d layers, group %d, %s: max|dlogp| %.2e (bound %.0e), max|dscore| %.2e" % (
        n_layers, group, precision, np.abs(logp - rl).max(), PB.LOGIT_TOL, np.abs(score - rs).max()))
    assert logp.shape == (2 * group, 16, 2) and best.shape == (2,) and best.dtype == np.int32
    assert np.abs(logp - rl).max() <= PB.LOGIT_TOL
    assert np.all(np.abs(score - rs) <= 2 * PB.LOGIT_TOL * np_) and np.all(np.abs(sdir - rd) <= PB.LOGIT_TOL * np_[:, None])
    for s in range(2 * group):
        assert np.all(logp[s, n_pos[s]:] == 0.0) and np.all(logp[s, :n_pos[s]] < 0.0)
    assert best.tolist() == [int(score[n * group:(n + 1) * group].argmax()) for n in range(2)]


def test_score_pairs_in_chunks_of_clips(monkeypatch):
    """N = 3 clips in groups of 3 with the row limit lowered to two clips' rows: score_pairs runs a chunk of two clips and one of
    one (its own _begin, output slices and tail launch each).  The stage of a chunk sees other row counts than the whole batch,
    so the GEMMs may take other routes: both results are within LOGIT_TOL of the same oracle per log-probability
    (test_score_pairs_against_the_oracle), hence within 2 * LOGIT_TOL of each other, the scores within that per position."""
    from sbl_for_multilingual_lip_reading_amd.transformer import decoder as D
    dec, _ = _decoder(2, 11)
    N, G = 3, 3
    rng = np.random.RandomState(5)
    lens = [4, 15, 1, 9, 2, 12, 7, 7, 3]
    words = [rng.randint(2, 58, size=c).tolist() for c in lens]
    ys = [torch.tensor([LC.row(w[::-1] if d else w) for w in words], dtype=torch.int64, device=DEV) for d in (0, 1)]
    n_pos = torch.tensor([c + 1 for c in lens], dtype=torch.int32, device=DEV)
    enc = PB.encoder_output(N, 5, 61).to(DEV)
    whole = dec.score_pairs(enc, ys[0], ys[1], n_pos, group=G)
    monkeypatch.setattr(D, "SCORE_PAIRS_MAX_ROWS", 2 * 136 * G)
    begins = []
    monkeypatch.setattr(dec, "_begin", lambda e, _b=dec._begin: begins.append(e.size(0)) or _b(e))
    parts = dec.score_pairs(enc, ys[0], ys[1], n_pos, group=G)
    assert begins == [2, 1]
    np_ = n_pos.cpu().numpy()
    d_logp = (parts.logp - whole.logp).abs().max().item()
    print("chunks of 2 + 1 clips: max|dlogp| %.2e (bound %.0e)" % (d_logp, 2 * PB.LOGIT_TOL))
    assert d_logp <= 2 * PB.LOGIT_TOL and bool(torch.isfinite(parts.score).all())
    assert np.all((parts.score - whole.score).abs().cpu().numpy() <= 2 * 2 * PB.LOGIT_TOL * np_)
    assert np.all((parts.score_dir - whole.score_dir).abs().cpu().numpy() <= 2 * PB.LOGIT_TOL * np_[:, None])
    assert torch.equal(parts.logp == 0, whole.logp == 0)
    assert parts.best.tolist() == parts.score.view(N, G).argmax(1).tolist() and parts.best.shape == (N,)


# --------------------------------------------------------------------------- 4. consistency with the merged beam search
def test_score_pairs_reproduces_the_beam_searchs_totals(precision):
    """score_pairs(n_pos = None, group = W) on the n-best of beam_search(W = 3, nbest = 3) re-derives that search's scores
    within 2 * step_tol(15).  Bit equality is not expected: the search runs 16 stages of one prefix length, score_pairs one
    ragged stage of all 16, so the GEMMs see other row counts and take other routes; each path is within step_tol(15) of the
    same oracle (test_search_passes_the_oracles_checker_and_rescoring holds the search to it)."""
    dec, _ = _decoder(2, 7)
    N, W = 3, 3
    enc = PB.encoder_output(N, 8, 7).to(DEV)
    res = dec.beam_search(enc, W, W)
    got = dec.score_pairs(enc, res.ys_l2r, res.ys_r2l, n_pos=None, group=W)
    d_score = float((got.score.view(N, W) - res.scores).abs().max())
    d_dir = float((got.score_dir.view(N, W, 2) - res.scores_dir).abs().max())
    print("%s: max|dscore| %.2e, max|dscore_dir| %.2e (bound %.1e)" % (precision, d_score, d_dir, 2 * PB.step_tol(15)))
    assert bool(torch.isfinite(res.scores).all()) and d_score <= 2 * PB.step_tol(15) and d_dir <= 2 * PB.step_tol(15)
    assert bool((got.logp < 0).all())
    assert got.best.tolist() == got.score.view(N, W).argmax(1).tolist()


# --------------------------------------------------------------------------- 5. end to end, 7. meter
_E2E = {}


def _e2e(beam):
    """Decoder.recognize_words at 2 + 2 layers, N = 3, Wn = 40, K = 5, greedy (beam = None) or W = 3, nbest = 3, in f32.  The
    lexicon is built around the greedy hypotheses: clip 0's own phoneme string is left out (only strings one edit away are
    words), the other clips' strings are words, the rest is random."""
    if beam not in _E2E:
        dec, sd = _decoder(2, 9)
        N, Wn, K = 3, 40, 5
        enc = PB.encoder_output(N, 8, 9)
        ys_l, _ = dec.recognize_beam(enc.to(DEV))
        rng = np.random.RandomState(3)
        greedy = [[t for t in LO.strip(r) if t != 1][:15] or [2] for r in ys_l.cpu().tolist()]
        words = []
        for n, g in enumerate(greedy):
            if n:
                words.append(list(g))
            words.append([int(rng.randint(2, 58))] + g[1:])                    # a substitution
            words.append((g[:-1] if len(g) > 1 else g + [3]))                   # a deletion (or an insertion behind one token)
        words = [w for w in words if w != greedy[0]]
        while len(words) < Wn:
            w = rng.randint(2, 58, size=rng.randint(1, 16)).tolist()
            if w != greedy[0]:
                words.append(w)
        from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
        lex = Lexicon(words, device=DEV)
        if beam is None:
            hyp = dec.recognize_beam(enc.to(DEV))
            hyp = tuple(h.unsqueeze(1) for h in hyp)
        else:
            r = dec.beam_search(enc.to(DEV), 3, 3)
            hyp = (r.ys_l2r, r.ys_r2l)
        res = dec.recognize_words(enc.to(DEV), lex, beam_size=beam, nbest=1 if beam is None else 3, shortlist=K)
        torch.cuda.synchronize()
        _E2E[beam] = dict(words=words, greedy=greedy, enc=enc, sd=sd, res=res, hyp=[h.cpu().numpy() for h in hyp], K=K, N=N)
    return _E2E[beam]


@pytest.mark.parametrize("beam", [None, 3])
def test_recognize_words_end_to_end(beam):
    """Margin-free, in the manner of sbl_beam_oracle.follow: the device's shortlist equals, exactly, the restatement's shortlist
    of the hypotheses the device itself produced (the decode is deterministic, so a second call gives the same ones), and the
    ORACLE's score of the chosen word is within 2 * LOGIT_TOL * (n_pos of the chosen + n_pos of the oracle's best) - both
    device scores are within 2 * LOGIT_TOL * n_pos of the oracle's - of the oracle's best over the shortlist.  The greedy
    phoneme string of clip 0 is not a lexicon word, so string equality would miss it."""
    c = _e2e(beam)
    N, K, res, words = c["N"], c["K"], c["res"], c["words"]
    assert c["greedy"][0] not in words and len(words) == 40
    want = LO.shortlist(c["hyp"][0], c["hyp"][1], words, K)
    cand = res.cand.cpu().numpy()
    assert np.array_equal(cand, want["cand"]) and np.array_equal(res.cand_dist.cpu().numpy(), want["cand_dist"])
    assert np.array_equal(res.cand_hyp.cpu().numpy(), want["cand_hyp"])
    assert res.word.dtype == torch.int64 and res.word.shape == (N,) and res.score.shape == (N, K) and res.score_dir.shape == (N, K, 2)
    if beam is None:      # no word spells clip 0's greedy hypothesis: string equality would call it a miss
        assert LO.strip(c["hyp"][0][0, 0]) not in words and want["cand_dist"][0, 0] > 0
    score = res.score.cpu().numpy()
    word = res.word.cpu().numpy()
    assert np.array_equal(word, cand[np.arange(N), score.argmax(1)]) and np.all(np.isfinite(score))
    _, _, oracle = LO.pair_scores(c["sd"], c["enc"], torch.from_numpy(want["cand_ys_l2r"]), torch.from_numpy(want["cand_ys_r2l"]),
                                  want["n_pos"], K, 2)
    oracle, n_pos = oracle.reshape(N, K), want["n_pos"].reshape(N, K)
    print("beam %s: max|dscore| %.2e" % (beam, np.abs(score - oracle).max()))
    assert np.all(np.abs(score - oracle) <= 2 * PB.LOGIT_TOL * n_pos)
    for n in range(N):
        r, b = int(score[n].argmax()), int(oracle[n].argmax())
        assert oracle[n, r] >= oracle[n, b] - 2 * PB.LOGIT_TOL * (n_pos[n, r] + n_pos[n, b]), (n, r, b)


def test_word_accuracy_meter_on_the_decodes(tmp_path):
    """n, n_correct and n_in_shortlist against Python counts on the two decodes above, with gold words that are chosen, merely
    shortlisted, and absent; valid_rows masks the tail; all_reduce over a single-rank group leaves the counters as they are."""
    import torch.distributed as dist
    from sbl_for_multilingual_lip_reading_amd.transformer.metrics import WordAccuracyMeter
    meter = WordAccuracyMeter(device=DEV)
    n = ok = among = 0
    for beam, valid in ((None, None), (3, None), (3, 2)):
        res = _e2e(beam)["res"]
        cand, word = res.cand.cpu().numpy(), res.word.cpu().numpy()
        other = [int(w) for w in cand[1] if w != word[1]][0]
        absent = [w for w in range(40) if w not in cand[2]][0]
        gold = np.array([word[0], other, absent], np.int64)
        meter.update(res, torch.from_numpy(gold).to(DEV), None if valid is None else torch.tensor([valid], dtype=torch.int32, device=DEV))
        live = 3 if valid is None else valid
        n += live
        ok += int((word[:live] == gold[:live]).sum())
        among += sum(int(gold[i] in cand[i]) for i in range(live))
    assert (n, ok, among) == (8, 3, 6)
    r = meter.result()
    assert (r["n"], r["n_correct"], r["n_in_shortlist"]) == (n, ok, among) and r["accuracy"] == ok / n
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "rdv"), rank=0, world_size=1)
    try:
        meter.all_reduce()
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert meter.acc.tolist() == [n, ok, among]
    meter.reset()
    assert meter.acc.tolist() == [0, 0, 0]


# --------------------------------------------------------------------------- 6. graph replay
def _transformer():
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    from sbl_for_multilingual_lip_reading_amd.transformer.transformer import Transformer
    m = Transformer(Encoder(512, 2, 8, 64, 64, 512, 2048), Decoder(0, 1, 58, 512, 2, 8, 64, 64, 512, 2048), None)
    m.load_state_dict({k: (v if k.endswith("pe") else torch.from_numpy(detfill.fill_value(k, tuple(v.shape), 0, "varied").copy()))
                       for k, v in m.state_dict().items()})
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    m.visual_frontend.frontend_dropout_p = 0.0
    return m.to(DEV)


@pytest.mark.parametrize("beam", [None, 3])
def test_validate_words_graph_replay(beam):
    """Transformer.validate_words in eval() under no_grad, captured as ONE hipGraph on the default queue count, as
    test_search_graph_replay captures the search: two replays on different clips equal the eager calls bit for bit (word,
    shortlist, scores), and the meter's counters after replays with valid_rows = N - 1 equal the eager counters."""
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    from sbl_for_multilingual_lip_reading_amd.transformer.metrics import WordAccuracyMeter
    B, T, Hh, Ww = 3, 8, 24, 24
    m = _transformer().eval()
    batches = [detfill.synthetic_batch(B, T, Hh, Ww, salt) for salt in (51, 52)]
    lex, gold = Lexicon.from_targets(torch.from_numpy(np.concatenate([b[1] for b in batches] + [detfill.synthetic_batch(8, T, Hh, Ww, 53)[1]])),
                                     device=DEV)
    xs = [torch.from_numpy(b[0]).to(DEV) for b in batches]
    golds = [gold[:B].to(DEV), gold[B:2 * B].to(DEV)]
    K = min(4, len(lex))
    kw = dict(beam_size=beam, nbest=1 if beam is None else 3, shortlist=K)
    vr = torch.tensor([B - 1], dtype=torch.int32, device=DEV)
    eager, meter = WordAccuracyMeter(device=DEV), WordAccuracyMeter(device=DEV)
    host = lambda r: [t.cpu().numpy().copy() for t in r]      # noqa: E731
    with torch.no_grad():
        want = [host(m.validate_words(x, g, lex, eager, valid_rows=vr, **kw)) for x, g in zip(xs, golds)]
        torch.cuda.synchronize()
        static_x, static_g = xs[0].clone(), golds[0].clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m.validate_words(static_x, static_g, lex, meter, valid_rows=vr, **kw)      # warm-up on the capture stream
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            res = m.validate_words(static_x, static_g, lex, meter, valid_rows=vr, **kw)
        meter.reset()
        for x, g, ref in zip(xs, golds, want):
            static_x.copy_(x)
            static_g.copy_(g)
            graph.replay()
            torch.cuda.synchronize()
            for a, b, name in zip(host(res), ref, res._fields):
                assert np.array_equal(a, b), name
    assert eager.acc.tolist() == meter.acc.tolist() and eager.acc[0].item() == 2 * (B - 1)
    assert np.all(np.isfinite(want[0][4])) and not np.array_equal(want[0][4], want[1][4])
