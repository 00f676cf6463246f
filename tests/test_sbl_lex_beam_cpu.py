"""CPU-side checks of the lexicon-constrained pair beam search of the SBL decoder: Lexicon.pair_trie() against the dict trie
of tests/sbl_lex_beam_oracle.py and the invariants include/sbl_hip.h states, the restatement (pair_lex_beam) against the
teacher-forced brute force over every word, the checker follow_lex on the restatement's own history and on a broken one, and
the new public names."""
import os
import re

import numpy as np
import pytest
import torch

import lex_beam_oracle as LB
import sbl_beam_oracle as PB
import sbl_lex_beam_oracle as PL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, SOS, EOS = 58, 0, 1

WORD_SETS = {
    "random 5": LB.make_words(5, V, 1),
    "random 40": LB.make_words(40, V, 2),
    "random 300, short": LB.make_words(300, V, 3, 1, 3),
    "one word": [[7, 3, 9]],
    "duplicate rows": [[4, 5], [6], [4, 5], [6], [4, 5, 6]],
    "aa / aaa": [[2, 2], [2, 2, 2], [2]],
    "palindrome": [[3, 4, 3], [3, 4, 4, 3], [3, 5, 3]],
    "reverses": [[3, 4, 5], [5, 4, 3], [3, 4], [4, 3]],
    "15 tokens": [list(range(2, 17)), list(range(2, 16)), [57] * 15],
}


def _lexicon(words):
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    return Lexicon(words, device="cpu", vocab=V, sos_id=SOS, eos_id=EOS)


def _keys(w):
    c = len(w)
    return [w[t] * 64 + w[c - 1 - t] for t in range(c)] + [EOS * 64 + EOS]


@pytest.mark.parametrize("name", sorted(WORD_SETS))
def test_pair_trie_equals_the_dict_trie(name):
    words = WORD_SETS[name]
    lex = _lexicon(words)
    begin, key, word = lex.pair_trie()
    assert lex.pair_trie()[0] is begin      # cached
    assert all(t.dtype == torch.int32 and t.dim() == 1 for t in (begin, key, word))
    ref_begin, ref_key, ref_word, _ = PL.pair_tables(words, EOS)
    assert begin.tolist() == ref_begin and key.tolist() == ref_key and word.tolist() == ref_word
    P = word.numel()
    assert begin.numel() == P + 1 and key.numel() == P - 1 and P <= 2 + sum(len(w) + 1 for w in words)


@pytest.mark.parametrize("name", sorted(WORD_SETS))
def test_pair_trie_invariants(name):
    """Keys ascend inside a node and stay below 4096; the terminal nodes are exactly the nodes with word >= 0, one per
    distinct word, with empty ranges; the child of entry e is node e + 1 - every node but the root is the child of exactly
    one entry - so walking any word's key sequence from the root ends on the terminal that carries its lowest index."""
    words = WORD_SETS[name]
    begin, key, word = (t.tolist() for t in _lexicon(words).pair_trie())
    P = len(word)
    assert begin[0] == 0 and begin[-1] == len(key) == P - 1 and all(a <= b for a, b in zip(begin, begin[1:]))
    for p in range(P):
        ks = key[begin[p]:begin[p + 1]]
        assert all(0 <= k < 4096 for k in ks) and all(a < b for a, b in zip(ks, ks[1:]))
        assert (word[p] >= 0) == (begin[p] == begin[p + 1]), p      # a node without children is a terminal and the reverse
        if p:
            assert key[p - 1] == EOS * 64 + EOS if word[p] >= 0 else key[p - 1] != EOS * 64 + EOS
    first = {}
    for i, w in enumerate(words):
        first.setdefault(tuple(w), i)
    assert sorted(x for x in word if x >= 0) == sorted(first.values())
    for i, w in enumerate(words):
        p = 0
        for k in _keys(w):
            ks = key[begin[p]:begin[p + 1]]
            assert k in ks, (i, p, k)
            p = begin[p] + ks.index(k) + 1
        assert word[p] == first[tuple(w)]


def test_states_are_shared_across_lengths_and_reverses():
    begin, key, word = (t.tolist() for t in _lexicon(WORD_SETS["aa / aaa"]).pair_trie())
    # root -> (a, a) -> {eos of "a", (a, a)} -> {eos of "aa", (a, a)} -> eos of "aaa"
    a, e = 2 * 64 + 2, EOS * 64 + EOS
    assert key == [a, e, a, e, a, e] and word == [-1, -1, 2, -1, 0, -1, 1]
    assert key[begin[3]:begin[4]] == [e, a]      # the depth-2 node of "aa" and "aaa": an (eos, eos) child and a token child
    # two words that are reverses of each other never share a node below the root: their first keys differ
    begin, key, word = (t.tolist() for t in _lexicon([[3, 4, 5], [5, 4, 3]]).pair_trie())
    assert key[begin[0]:begin[1]] == [3 * 64 + 5, 5 * 64 + 3] and len(word) == 1 + 2 * 4
    # a palindrome's l2r and r2l tokens agree at every step
    begin, key, word = (t.tolist() for t in _lexicon([[3, 4, 3]]).pair_trie())
    assert key == [3 * 64 + 3, 4 * 64 + 4, 3 * 64 + 3, EOS * 64 + EOS]


# --------------------------------------------------------------------------- the restatement
WORDS6 = PL.WORDS6


@pytest.fixture(scope="module")
def searched():
    sd = PB.decoder_state_dict(2, 5)
    enc = PB.encoder_output(2, 8, 5)
    return sd, enc, PL.pair_lex_beam(sd, enc, 2, WORDS6, 8), PL.brute_force(sd, enc, 2, WORDS6)


def _history(out):
    return tuple(out[k].copy() for k in ("tok_l", "tok_r", "par", "score", "node"))


def test_exhaustive_search_equals_brute_force(searched):
    """W = 8 >= 6 words: nothing is pruned, so the search returns every word exactly once with its teacher-forced score."""
    sd, enc, out, brute = searched
    steps = out["steps"]
    assert steps == 6 and out["score"].shape == (2, steps, 8)
    rows = PL.word_rows(WORDS6, SOS, EOS)
    for n in range(2):
        assert sorted(out["cand"][n, :6].tolist()) == list(range(6)) and out["cand"][n, 6:].tolist() == [-1, -1]
        assert np.all(out["scores"][n, 6:] == -np.inf)
        for r in range(6):
            w = out["cand"][n, r]
            assert abs(out["scores"][n, r] - brute[n, w]) <= PB.step_tol(len(WORDS6[w])), (n, r, w)
            assert abs(out["scores_dir"][n, r].sum() - out["scores"][n, r]) <= 1e-4
            assert np.array_equal(out["ys_l2r"][n, r], rows[0][w]) and np.array_equal(out["ys_r2l"][n, r], rows[1][w])
            assert r == 0 or out["scores"][n, r] <= out["scores"][n, r - 1] + PB.step_tol(steps - 1)
        assert out["cand"][n, 0] == int(np.argmax(brute[n]))


def test_follow_lex_accepts_the_restatements_own_history(searched):
    sd, enc, out, _ = searched
    st = PL.follow_lex(_history(out), sd, enc, 2, WORDS6, 8)
    assert st["max_dscore"] == 0.0 and st["max_deficit"] <= 0.0
    assert np.array_equal(st["ys_l2r"], out["ys_l2r"]) and np.array_equal(st["ys_r2l"], out["ys_r2l"])
    assert np.array_equal(st["cand"], out["cand"])


def test_follow_lex_rejects_a_token_that_is_no_edge(searched):
    sd, enc, out, _ = searched
    tok_l, tok_r, par, score, node = _history(out)
    assert tok_l[1, 1, 0] != 13
    tok_l[1, 1, 0] = 13      # no word holds token 13
    with pytest.raises(AssertionError, match="clip 1 step 1 rank 0"):
        PL.follow_lex((tok_l, tok_r, par, score, node), sd, enc, 2, WORDS6, 8)
    tok_l, tok_r, par, score, node = _history(out)
    node[0, 2, 1] += 1      # the right edge, another node
    with pytest.raises(AssertionError, match="clip 0 step 2 rank 1: reported node"):
        PL.follow_lex((tok_l, tok_r, par, score, node), sd, enc, 2, WORDS6, 8)


# --------------------------------------------------------------------------- the public names
def test_the_new_surface_exists():
    from sbl_for_multilingual_lip_reading_amd import _lib, ops
    from sbl_for_multilingual_lip_reading_amd.transformer import decoder, transformer
    assert callable(decoder.Decoder.beam_search_lex) and callable(ops.pair_beam_tail_lex)
    assert callable(transformer.Transformer.recognize_words_lex) and callable(transformer.Transformer.validate_words_lex)
    assert decoder.PairWordBeamResult._fields == ("word", "cand", "score", "score_dir", "ys_l2r", "ys_r2l", "history")
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbl_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+sbl_pair_beam_tail_lex\s*\(", src) and "sbl_pair_beam_tail_lex" in _lib.SIGNATURES


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from sbl_for_multilingual_lip_reading_amd import _lib
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    dec = Decoder(SOS, EOS, V, 512, 1, 8, 64, 64, 512, 2048)
    lex = _lexicon(WORDS6)
    enc = torch.zeros(2, 8, 512)
    with pytest.raises(_lib.SblHipError, match="no CPU path"):
        dec.beam_search_lex(enc, lex, 3)
    for W in (0, 17):
        with pytest.raises(_lib.SblHipError, match="beam_size"):
            dec.beam_search_lex(enc, lex, W)
    with pytest.raises(_lib.SblHipError, match="nbest"):
        dec.beam_search_lex(enc, lex, 3, 4)
    # the C entry point's own checks come before the launch: aliased node buffers, an empty table
    import ctypes
    buf = ctypes.create_string_buffer(64)
    a = (ctypes.addressof(buf) + 15) & ~15
    args = [a, a, 512, a, a, a, a, a, a, a + 16, a + 16, 17, a, a, a, a, 0, 6, EOS, 1, 3, V, 512, a, a, a, 4, 3, a, a, a, None]
    with pytest.raises(_lib.SblHipError, match="aliased node buffers"):
        _lib.call("sbl_pair_beam_tail_lex", *args)
    args[26] = 0
    with pytest.raises(_lib.SblHipError, match="P=0"):
        _lib.call("sbl_pair_beam_tail_lex", *args)
