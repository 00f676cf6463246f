"""CPU checks of the closed-vocabulary word decode: the restatement (tests/lexicon_oracle.py) against hand-worked cases, the
Lexicon container, the word-accuracy meter's counting, and the C-ABI surface of the two new entry points (declared, bound
with the header's arity, argument checks before any launch).  No GPU compute."""
import re
import types

import numpy as np
import pytest
import torch

import lexicon_cases as LC
import lexicon_oracle as LO
import sbl_beam_oracle as PB


@pytest.mark.parametrize("case", LC.HAND, ids=[c[0] for c in LC.HAND])
def test_restatement_on_hand_worked_cases(case):
    _, words, ys_l, ys_r, K, cand, dist, hyp = case
    got = LO.shortlist(np.array([ys_l]), np.array([ys_r]), words, K)
    assert got["cand"].tolist() == [cand] and got["cand_dist"].tolist() == [dist] and got["cand_hyp"].tolist() == [hyp]
    for r, w in enumerate(cand):
        c = len(words[w])
        assert got["n_pos"][r] == c + 1
        assert got["cand_ys_l2r"][r].tolist() == [0] + words[w] + [1] * (16 - c)
        assert got["cand_ys_r2l"][r].tolist() == [0] + words[w][::-1] + [1] * (16 - c)


def test_strip_and_distance():
    assert LO.strip([0, 1] + [5] * 15) == [] and LO.strip(LC.row(LC.LONG)) == LC.LONG
    assert LO.strip([7, 7, -1, 0, 8, 1, 9] + [1] * 10) == [7, 8]          # column 0 is never read
    assert LO.lev([], [3, 4]) == 2 and LO.lev([3, 4], []) == 2 and LO.lev([3, 4, 5], [3, 5]) == 1 and LO.lev([1, 2, 3], [2, 3, 4]) == 2
    # kitten / sitting as ids
    a, b = [ord(c) for c in "kitten"], [ord(c) for c in "sitting"]
    assert LO.lev(a, b) == 3 and LO.lev(b, a) == 3
    assert LO.distances([7, 8], [8, 7], [[7, 8], [8, 7]]) == [0, 4]


def test_seeded_cases_hold_what_they_promise():
    """The seeded inputs of the GPU test embed the hand cases: an empty and a 16-token hypothesis, a 15-token word, two
    identical rows ranked by index, a D = 0 hit, and (H = 3) two hypotheses with equal D."""
    words = LC.make_lexicon(257, 3)
    assert len(words[0]) == 15 and words[1] == words[3] and all(1 <= len(w) <= 15 for w in words)
    ys_l, ys_r = LC.make_hyps(words, 3, 4)
    assert LO.strip(ys_l[0, 0]) == [] and len(LO.strip(ys_l[1, 0])) == 16 and LO.strip(ys_l[2, 0]) == words[1]
    got = LO.shortlist(ys_l, ys_r, words, 5)
    assert got["cand"][2, :2].tolist() == [1, 3] and got["cand_dist"][2, :2].tolist() == [0, 0] and got["cand_hyp"][2, :2].tolist() == [0, 0]
    assert np.array_equal(ys_l[0, 1], ys_l[0, 2]) and np.array_equal(ys_r[0, 1], ys_r[0, 2])
    assert got["cand"][0, :2].tolist() == [1, 3] and got["cand_dist"][0, :2].tolist() == [0, 0] and got["cand_hyp"][0, :2].tolist() == [1, 1]
    assert (got["cand"][1, 0], got["cand_dist"][1, 0], got["cand_hyp"][1, 0]) == (0, 0, 2)      # through the ignore / sos entries


def test_table_distances_and_strided_lexicon():
    """The all-words-at-once table the restatement uses for large lexicons gives lev's distances, and the strided lexicon puts
    several of a clip's 16 best words at indices that differ by multiples of 1024."""
    words = LC.make_strided_lexicon(4100, 8)
    ys_l, ys_r = LC.make_hyps(words, 3, 9)
    for n, h in ((0, 0), (1, 0), (1, 2), (2, 1)):
        p_l, p_r = LO.strip(ys_l[n, h]), LO.strip(ys_r[n, h])
        assert LO.distances_table(p_l, p_r, words[:300] + words[1024:1030]) == LO.distances(p_l, p_r, words[:300] + words[1024:1030])
    got = LO.shortlist(ys_l, ys_r, words, 16)
    for n, lane in ((0, 1), (2, 1), (1, 0)):
        assert sum(1 for w in got["cand"][n] if w % 1024 == lane) >= 3, (n, got["cand"][n])
    assert got["cand"].max() >= 4096


def test_lexicon_packing_and_validation():
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    words = [[5, 6, 7], list(range(2, 17)), [57], [5, 6, 7]]
    lx = Lexicon(words, names=["a", "b", "c", "a2"], device="cpu")
    assert len(lx) == 4 and lx.lengths.tolist() == [3, 15, 1, 3] and lx.names[3] == "a2"
    assert lx.packed.dtype == torch.uint8 and lx.packed.shape == (4, 16) and lx.packed.is_contiguous()
    assert lx.packed[0].tolist() == [5, 6, 7] + [0] * 12 + [3] and lx.packed[1].tolist() == list(range(2, 17)) + [15]
    assert lx.tokens.shape == (4, 15) and lx.tokens[2].tolist() == [57] + [-1] * 14 and lx.word(1) == list(range(2, 17))
    for bad, msg in (([], "0 words"), ([[]], "0 tokens"), ([list(range(2, 18))], "16 tokens"), ([[5, 58]], "id 58"),
                     ([[5, 0]], "id 0"), ([[1]], "id 1"), ([[-1]], "id -1")):
        with pytest.raises(ValueError, match=msg):
            Lexicon(bad, device="cpu")
    with pytest.raises(ValueError, match="1 names for 2 words"):
        Lexicon([[5], [6]], names=["x"], device="cpu")
    with pytest.raises(ValueError, match="vocab = 65"):
        Lexicon([[5]], device="cpu", vocab=65)


def test_lexicon_from_targets():
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    gold = torch.tensor([[5, 6, -1, -1], [7, -1, -1, -1], [5, 6, -1, -1], [5, -1, 6, 7], [7, -1, -1, -1]])
    lx, idx = Lexicon.from_targets(gold, device="cpu")
    assert [lx.word(w) for w in range(len(lx))] == [[5, 6], [7], [5, 6, 7]] and idx.tolist() == [0, 1, 0, 2, 1] and idx.dtype == torch.int64
    with pytest.raises(ValueError, match="word 1 has 0 tokens"):
        Lexicon.from_targets(torch.tensor([[5, -1], [-1, -1]]), device="cpu")


def test_word_accuracy_meter_counts():
    """The meter's integer ops on CPU tensors (they are device-agnostic torch ops) against Python counts, with and without
    valid_rows, across a change of batch shape, and reset."""
    from sbl_for_multilingual_lip_reading_amd.transformer.metrics import WordAccuracyMeter
    rng = np.random.RandomState(5)
    meter = WordAccuracyMeter(device="cpu")
    n = ok = among = 0
    for N, K, valid in ((7, 4, None), (7, 4, 3), (7, 4, 0), (5, 2, 9), (1, 1, None)):
        cand = np.stack([rng.permutation(12)[:K] for _ in range(N)]).astype(np.int32)
        word = cand[np.arange(N), rng.randint(0, K, N)].astype(np.int64)
        gold = np.where(rng.rand(N) < 0.5, word, rng.randint(0, 12, N)).astype(np.int64)
        res = types.SimpleNamespace(word=torch.from_numpy(word), cand=torch.from_numpy(cand))
        meter.update(res, torch.from_numpy(gold), None if valid is None else torch.tensor([valid], dtype=torch.int32))
        live = N if valid is None else min(valid, N)
        n += live
        ok += int((word[:live] == gold[:live]).sum())
        among += sum(int(gold[i] in cand[i]) for i in range(live))
    r = meter.result()
    assert (r["n"], r["n_correct"], r["n_in_shortlist"]) == (n, ok, among) and 0 < ok < among <= n
    assert r["accuracy"] == ok / n and r["shortlist_recall"] == among / n
    meter.reset()
    assert meter.result()["n"] == 0 and np.isnan(meter.result()["accuracy"])
    with pytest.raises(ValueError, match="gold_word"):
        meter.update(res, torch.zeros(3, dtype=torch.int64))


def test_pair_scores_restatement_is_the_beam_oracles_total():
    """With n_pos = None on the pairs a width-1 search of the beam oracle decoded, pair_scores re-derives that search's totals
    (the same primitives on other batch shapes: 1e-4), and n_pos cuts the sums where it says."""
    sd = PB.decoder_state_dict(1, 3)
    enc = PB.encoder_output(2, 5, 3)
    ref = PB.pair_beam(sd, enc, 1, 1)
    ys = [torch.from_numpy(ref[k].reshape(2, 17)) for k in ("ys_l2r", "ys_r2l")]
    logp, sdir, score = LO.pair_scores(sd, enc, ys[0], ys[1], None, 1, 1)
    assert np.abs(score - ref["scores"][:, 0]).max() <= 1e-4 and np.abs(sdir - ref["scores_dir"][:, 0]).max() <= 1e-4
    logp2, sdir2, score2 = LO.pair_scores(sd, enc, ys[0], ys[1], [3, 16], 1, 1)
    assert np.array_equal(logp2[0, :3], logp[0, :3]) and np.all(logp2[0, 3:] == 0) and np.array_equal(logp2[1], logp[1])
    assert abs(float(score2[0]) - float(logp[0, :3].sum())) <= 1e-5 and score2[1] == score[1] and np.all(logp < 0)


# --------------------------------------------------------------------------- the C ABI of the two entry points
def test_abi_surface_of_the_new_entry_points():
    """Through the mechanism of tests/test_abi_cpu.py: declared in include/sbl_hip.h (with the reference lines they replace),
    bound in the ctypes table with the declared arity, exported by the library."""
    import test_abi_cpu as ABI
    from sbl_for_multilingual_lip_reading_amd import _lib
    lib = _lib.load()
    src = open(ABI.HEADER).read()
    assert "train.py:28-38" in src and "test.py:185-218" in src
    stripped = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in (("sbl_lexicon_shortlist", 20), ("sbl_pair_score_tail", 18)):
        assert name in ABI._declared() and hasattr(lib, name)
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, stripped, flags=re.S)
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs == len(_lib.SIGNATURES[name])


def test_new_entry_points_check_their_arguments_on_the_host():
    """Refusals happen before any launch, and N == 0 / S == 0 return early: safe without a GPU."""
    import ctypes
    from sbl_for_multilingual_lip_reading_amd import _lib
    buf = ctypes.create_string_buffer(256)
    a = (ctypes.addressof(buf) + 15) & ~15

    def shortlist(Ly=17, Wn=10, N=2, H=1, K=3, ld_h=17, lex=a, sos=0):
        _lib.call("sbl_lexicon_shortlist", a, a, 17 * H, ld_h, Ly, lex, Wn, N, H, K, sos, 1, -1, a, a, a, a, a, a, None)

    for kw, msg in ((dict(Ly=16), "rows of 16 entries"), (dict(H=0), "H=0"), (dict(H=17), "H=17"), (dict(Wn=0), "Wn=0"),
                    (dict(Wn=65537), "Wn=65537"), (dict(K=0), "K=0"), (dict(K=17, Wn=100), "K=17"), (dict(K=11), "K=11 outside 1..min\\(Wn=10"),
                    (dict(N=-1), "N=-1"), (dict(H=2, ld_h=3), "strides"), (dict(sos=1), "sos and eos"), (dict(lex=a + 4), "16-byte aligned"),
                    (dict(lex=None), "null input")):
        with pytest.raises(_lib.SblHipError, match=msg):
            shortlist(**kw)
    shortlist(N=0, lex=None)      # a successful no-op

    def tail(S=8, G=4, V=58, D=512, ldy=512, ldys=17, y=a, out=a):
        _lib.call("sbl_pair_score_tail", y, a, ldy, a, a, a, a, ldys, None, out, a, a, a, S, G, V, D, None)

    for kw, msg in ((dict(D=256), "D=256"), (dict(V=65), "V=65"), (dict(G=0), "G=0"), (dict(G=17), "G=17"), (dict(S=9), "S=9 slots"),
                    (dict(ldys=16), "token rows of 16"), (dict(ldy=510), "row stride 510"), (dict(y=None), "null input"),
                    (dict(out=None), "null output"), (dict(y=a + 4), "unaligned")):
        with pytest.raises(_lib.SblHipError, match=msg):
            tail(**kw)
    tail(S=0, y=None, out=None)


def test_word_decode_refuses_cpu_tensors():
    from sbl_for_multilingual_lip_reading_amd import _lib
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    dec = Decoder(0, 1, 58, 512, 1, 8, 64, 64, 512, 2048)
    enc = torch.zeros(1, 4, 512)
    ys = torch.ones(1, 17, dtype=torch.int64)
    with pytest.raises(_lib.SblHipError, match="score_pairs needs the encoder output on the GPU \\(got a cpu tensor\\)"):
        dec.score_pairs(enc, ys, ys)
    with pytest.raises(_lib.SblHipError, match="recognize_words needs the encoder output on the GPU \\(got a cpu tensor\\)"):
        dec.recognize_words(enc, Lexicon([[5]], device="cpu"))
