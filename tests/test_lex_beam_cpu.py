"""CPU-side checks of the lexicon-constrained beam search: Lexicon.trie() against a plain dict trie, the restatement
(tests/lex_beam_oracle.py) against beam_oracle.beam_clip (every candidate allowed) and against the brute-force ranking of a
lexicon the beam covers, the margins of every case the GPU tests run, and the host-side refusals.  Nothing here launches."""
import inspect

import numpy as np
import pytest
import torch

import beam_oracle as B
import lex_beam_oracle as L
import seq2seq_oracle as S
from test_seq2seq_cpu import build_model

LONG = list(range(2, 17))          # 15 tokens


def _random_words(n, V, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(2, V, size=rng.randint(1, 16)).tolist() for _ in range(n)]


# (name, words, vocab, sos, eos)
TRIE_CASES = [
    ("a single word", [[5, 6, 7]], 48, 0, 1),
    ("words that are prefixes of words", [[5], [5, 6], [5, 6, 7]], 48, 0, 1),
    ("duplicate rows", [[7, 8], [9], [7, 8], [9]], 48, 0, 1),
    ("a 15-token word", [LONG, LONG[:7] + [30], [40]], 48, 0, 1),
    ("token 63 with V = 64", [[63], [2, 63], [63, 63], [62, 63, 2]], 64, 0, 1),
    ("eos = V - 1", [[1, 2], [1, 2, 8], [8], [3, 1]], 10, 0, 9),
    ("eos = 63", [[1, 62], [62], [1]], 64, 0, 63),
    ("1000 random words over V = 48", _random_words(1000, 48, 11), 48, 0, 1),
]


def _lexicon(words, V=48, sos=0, eos=1, device="cpu"):
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    return Lexicon(words, device=device, vocab=V, sos_id=sos, eos_id=eos)


@pytest.mark.parametrize("name,words,V,sos,eos", TRIE_CASES, ids=[c[0] for c in TRIE_CASES])
def test_trie_tables_match_a_dict_trie(name, words, V, sos, eos):
    """P, the breadth-first numbering (siblings in ascending token id), every (node, token) child by the popcount formula,
    the eos bit of every node and word = the lowest index, against tests/lex_beam_oracle.dict_trie."""
    lex = _lexicon(words, V, sos, eos)
    mask, first, word = (t.tolist() for t in lex.trie())
    assert lex.trie()[0].dtype == torch.int64 and lex.trie()[1].dtype == torch.int32 and lex.trie()[2].dtype == torch.int32
    assert lex.trie() is lex.trie()                       # built once
    children, owner = L.dict_trie(words)
    order = L.bfs_order(children)
    P = len(order)
    assert len(mask) == len(first) == len(word) == P and P <= 1 + sum(len(w) for w in words)
    ident = {p: k for k, p in enumerate(order)}
    assert ident[()] == 0
    for p, k in ident.items():
        m = mask[k] & (2 ** 64 - 1)
        for v in range(64):
            want = (p in owner) if v == eos else (v in children[p])
            assert bool((m >> v) & 1) == want, (name, p, v)
            if want and v != eos:
                assert L.child_by_formula(mask, first, k, v, eos) == ident[p + (v,)], (name, p, v)
        if children[p]:
            assert first[k] == ident[p + (min(children[p]),)]
            kids = [ident[p + (v,)] for v in sorted(children[p])]
            assert kids == list(range(kids[0], kids[0] + len(kids))), "a node's children are consecutive"
        assert word[k] == owner.get(p, -1), (name, p)
    assert lex.max_len == max(len(w) for w in words)


@pytest.mark.parametrize("case", ["beam_small", "beam_varied", "beam_varied_len5"])
def test_restatement_with_every_candidate_allowed_is_beam_clip(case):
    """lex_beam_clip(allowed = None) equals beam_oracle.beam_clip, the restatement the reference's fixtures pin, in every
    field: n-best scores and tokens, the whole history, the margin and the counters."""
    g = B.load_golden(case + ".npz")
    c = B.beam_config(g)
    sd = S.case_state(g)
    with torch.no_grad():
        enc = S.encode(sd, B.case_clips(g), c["ne"], training=False)
        for e in enc:
            a = B.beam_clip(sd, e, c["nd"], c["scale"], c["W"], c["nbest"], c["maxlen"], B.log_prior(g))
            b = L.lex_beam_clip(sd, e, c["nd"], c["scale"], c["W"], c["nbest"], c["maxlen"], B.log_prior(g), None)
            assert sorted(a) == sorted(b)
            for k in a:
                if isinstance(a[k], np.ndarray):
                    assert np.array_equal(a[k], b[k]), k
                else:
                    assert a[k] == b[k], k


@pytest.mark.parametrize("prior", [False, True])
@pytest.mark.parametrize("shape", L.E2E_SHAPES)
def test_exhaustive_search_is_the_brute_force_ranking(shape, prior):
    """Five words, beam 5: no depth of the trie has more than W nodes, so nothing is ever pruned and the n-best is the
    ranking of all distinct words by their teacher-forced score (sum of the log-softmax at the tokens and the eos, plus
    the prior's bigram terms).  Words exact, scores within beam_oracle.score_tol."""
    salt = L.e2e_pick(shape, 5, 5, False)[0]
    sd, enc = L.e2e_encoded(shape, salt)
    c = S.case_config(L.e2e_fixture(shape, salt))
    words = L.e2e_words(shape, 5, 5, False)
    children, owner = L.dict_trie(words)
    depth = {}
    for p in children:
        depth[len(p)] = depth.get(len(p), 0) + 1
    assert max(depth.values()) <= 5 and len(owner) == 4          # one duplicate row
    lp = L.e2e_prior(shape) if prior else None
    o = L.lex_beam_search(sd, enc, c["nd"], c["scale"], words, 5, 5, lp)
    for n, e in enumerate(enc):
        rank = L.brute_force(sd, e, c["nd"], c["scale"], words, lp)
        rank = [r for r in rank if r[0] > -np.inf]
        assert o["n_hyps"][n] == len(rank)
        assert o["cand"][n, :len(rank)].tolist() == [w for _, w in rank] and np.all(o["cand"][n, len(rank):] == -1)
        assert np.abs(o["scores"][n, :len(rank)] - np.array([s for s, _ in rank])).max() <= B.score_tol(o["maxlen"])
        assert len(set(o["cand"][n, :len(rank)].tolist())) == len(rank)


@pytest.mark.parametrize("shape,Wn,W,prior", L.E2E_CASES)
def test_gpu_cases_meet_the_margin_floor(shape, Wn, W, prior):
    """Every (shape, salt, lexicon, W) of tests/test_lex_beam_gpu.py: the smallest decision gap of the oracle (adjacent kept
    ranks at every step, rank W against W + 1, adjacent final ranks up to nbest = 5 against the next) is at least
    margin_floor(maxlen), so the exact token comparisons on the GPU never have to be skipped or loosened."""
    o = L.e2e_oracle(shape, Wn, W, prior)
    words = L.e2e_words(shape, Wn, W, prior)
    assert o["maxlen"] == max(len(w) for w in words) + 1 <= 16
    assert o["margin"] >= B.margin_floor(o["maxlen"]), (shape, Wn, W, prior, o["margin"])
    assert (o["n_hyps"] >= 1).all()
    for n in range(len(o["cand"])):
        got = o["cand"][n, :o["n_hyps"][n]].tolist()
        assert len(set(got)) == len(got) and min(got) >= 0


def test_gpu_cases_cover_what_they_are_for():
    """The unseen salts differ from the fixtures', a wide beam over the big lexicons is really pruned, some clip offers
    fewer candidates than W at a step, and the Wn = 1 word has 15 tokens (maxlen = 16, the longest search)."""
    for shape in L.E2E_SHAPES:
        own = int(B.load_golden(shape + ".npz")["meta"][8])
        assert all(L.e2e_pick(*c)[0] not in (own, B.UNSEEN_SALTS[shape]) for c in L.E2E_CASES if c[0] == shape)
        assert {(c[1], c[2]) for c in L.E2E_CASES if c[0] == shape} >= {(1, 1), (5, 5)} | {(n, w) for n in (257, 1000) for w in (1, 3, 8, 16)}
        assert any(c[3] for c in L.E2E_CASES if c[0] == shape)
        assert L.e2e_oracle(shape, 1, 1, False)["maxlen"] == 16
        wide = L.e2e_oracle(shape, 1000, 16, shape == "beam_varied")
        assert (wide["hist_flag"][:, 1] != 0).all(), "step 1 fills all 16 ranks"
        assert (wide["hist_flag"][:, -1] == 0).any(), "the last step keeps fewer than W"
        narrow = L.e2e_oracle(shape, 1000, 3, False)
        assert (narrow["n_ended"] >= 3).all()


@pytest.mark.parametrize("V,W", L.TAIL_SHAPES)
def test_planted_tail_cases_show_what_they_are_for(V, W):
    """lex_beam_oracle.tail_case asserts, on the float64 expectation, that every planted situation occurs; here without a GPU."""
    saw = set().union(*(c["saw"] for c in L.tail_case(V, W)["steps"]))
    assert {"all-zero mask", "node out of range", "only eos", "only child V - 1"} <= saw
    assert W == 1 or {"dead slot", "fewer candidates than W", "parent tie"} <= saw


def test_bad_arguments_are_refused_on_the_host():
    """P = 0, a null table and the base tail's range checks stop sbl_beam_tail_lex before any launch; sbl_lexicon_lookup
    refuses short strides and P = 0, and R = 0 is a successful no-op: safe without a GPU."""
    import ctypes
    from sbl_for_multilingual_lip_reading_amd import _lib
    buf = ctypes.create_string_buffer(64)
    a = (ctypes.addressof(buf) + 15) & ~15

    def tail(W, V, maxlen, P, mask=a, node=a):
        _lib.call("sbl_beam_tail_lex", None, 512, None, None, None, None, None, None, 64, None, None, None, None, None, None, None,
                  0, maxlen, 1, None, None, 100, 1.0, None, 2, W, V, 512, mask, a, P, node, None)

    with pytest.raises(_lib.SblHipError, match="P=0"):
        tail(4, 42, 8, 0)
    with pytest.raises(_lib.SblHipError, match="null trie table"):
        tail(4, 42, 8, 3, mask=None)
    with pytest.raises(_lib.SblHipError, match="null trie table"):
        tail(4, 42, 8, 3, node=None)
    with pytest.raises(_lib.SblHipError, match="sbl_beam_tail_lex: beam W=17"):
        tail(17, 42, 8, 3)
    with pytest.raises(_lib.SblHipError, match="V=65"):
        tail(4, 65, 8, 3)
    with pytest.raises(_lib.SblHipError, match="null or aliased"):
        tail(16, 64, 64, 3)

    def lookup(R, Ly, ld, P):
        _lib.call("sbl_lexicon_lookup", None, ld, Ly, R, a, a, a, P, 0, 1, -1, None, None, None)

    with pytest.raises(_lib.SblHipError, match="stride 16"):
        lookup(2, 17, 16, 3)
    with pytest.raises(_lib.SblHipError, match="P=0"):
        lookup(2, 17, 17, 0)
    with pytest.raises(_lib.SblHipError, match="null input"):
        lookup(2, 17, 17, 3)
    lookup(0, 17, 17, 3)


def test_lexicon_guards_and_surface():
    """beam_search_lex refuses a lexicon of another vocab or eos, one on another device and decode_max_len != 0 before any
    device work (a meta tensor stands in for the encoder output); beam_search keeps its signature."""
    from sbl_for_multilingual_lip_reading_amd import _lib, ops
    from sbl_for_multilingual_lip_reading_amd.transformer import seq2seq
    m = build_model(B.load_golden("beam_small.npz")).eval()
    m.decoder._check_encoder = lambda e: None
    fake = torch.zeros(2, 6, 512, device="meta")
    for lex, kw, pat in ((_lexicon([[5, 6]], V=48), {}, "vocab / sos / eos"), (_lexicon([[5, 6]], V=42, eos=3), {}, "vocab / sos / eos"),
                         (_lexicon([[5, 6]], V=42), {}, "the lexicon is on cpu"),
                         (_lexicon([[5, 6]], V=42, device="meta"), dict(decode_max_len=5), "decode_max_len = 5 with a lexicon")):
        with pytest.raises(_lib.SblHipError, match=pat):
            m.decoder.beam_search_lex(fake, 3, lexicon=lex, **kw)
    with pytest.raises(_lib.SblHipError, match="no CPU path"):
        ops.lexicon_lookup(torch.zeros(2, 17, dtype=torch.long), _lexicon([[5, 6]]).trie(), 0, 1, -1)
    assert seq2seq.WordBeamResult._fields == ("word", "cand", "score", "n_hyps", "yseq")
    sig = inspect.signature(seq2seq.Seq2SeqDecoder.beam_search_lex).parameters
    assert list(sig)[1:] == ["encoder_outputs", "beam_size", "nbest", "decode_max_len", "log_prior", "lexicon"] and sig["lexicon"].default is None
    for cls in (seq2seq.Seq2SeqDecoder, seq2seq.Seq2SeqTransformer):
        r = inspect.signature(cls.recognize_words).parameters
        assert list(r)[2:] == ["lexicon", "beam_size", "nbest", "log_prior"] and r["beam_size"].default == 8 and r["nbest"].default == 1
    v = inspect.signature(seq2seq.Seq2SeqTransformer.validate_words).parameters
    assert list(v)[1:] == ["padded_input", "gold_word", "lexicon", "meter", "valid_rows", "beam_size", "nbest", "log_prior"]
    st = inspect.signature(ops.BeamState.__init__).parameters
    assert st["lex"].default is False and inspect.signature(ops.beam_tail).parameters["trie"].default is None
