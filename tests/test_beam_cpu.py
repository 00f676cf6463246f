"""CPU-side checks of the beam search: the plain-torch restatement (tests/beam_oracle.py) reproduces every fixture the
REFERENCE wrote (tests/golden/beam_*.npz, tools/make_beam_goldens.py), the inputs the GPU tests draw themselves meet the
margin floor, the new entry points refuse bad arguments before any launch, and nothing computes without a GPU."""
import numpy as np
import pytest
import torch

import beam_oracle as B
from test_seq2seq_cpu import build_model


@pytest.mark.parametrize("case", B.CASES)
def test_oracle_reproduces_reference_fixture(case):
    """Tokens, lengths and n_hyps exact, scores within 1e-4; the stored per-step history is the oracle's, and every decision
    gap is at least 10x the score tolerance (the generator's assert, re-checked)."""
    g, o = B.oracle_case(case)
    c = B.beam_config(g)
    assert g["yseq"].shape == (c["B"], c["nbest"], c["maxlen"] + 2)
    assert np.array_equal(o["yseq"], g["yseq"]) and np.array_equal(o["lengths"], g["lengths"])
    assert np.array_equal(o["n_hyps"], g["n_hyps"])
    assert float(np.abs(o["scores"] - g["scores"]).max()) < 1e-4
    for k in ("hist_tok", "hist_par", "hist_flag"):
        assert np.array_equal(o[k], g[k]), k
    fin = g["hist_flag"] != 0
    assert np.array_equal(np.isfinite(o["hist_score"]), fin) and float(np.abs(o["hist_score"][fin] - g["hist_score"][fin]).max()) < 1e-4
    assert o["margin"] >= B.margin_floor(c["maxlen"]) and abs(o["margin"] - float(g["margin"])) < 1e-3
    # the quirk of decoder.py:213-218: a hypothesis that ends at the last step has length maxlen + 2
    assert g["lengths"].max() == c["maxlen"] + 2
    if "freq" in g:
        lp = B.log_prior(g)
        assert lp.dtype == torch.float32 and bool(torch.isinf(lp).any())
        assert (o["early"] > 0).any() and (o["min_live"] < c["W"]).any()


@pytest.mark.parametrize("case", sorted(B.UNSEEN_SALTS))
def test_unseen_salts_meet_the_margin_floor(case):
    g, o = B.oracle_case(case, B.UNSEEN_SALTS[case])
    c = B.beam_config(g)
    assert int(g["meta"][8]) != int(B.load_golden(case + ".npz")["meta"][8])
    assert o["margin"] >= B.margin_floor(c["maxlen"]), (case, o["margin"])
    assert (o["n_hyps"] == c["nbest"]).all()


def test_bad_arguments_are_refused_on_the_host():
    """W = 17, W > V, V = 65, nbest = 0 and maxlen = 65 stop at the argument checks of the entry points: no pointer is
    read and nothing is launched, so this is safe without a GPU."""
    from sbl_for_multilingual_lip_reading_amd import _lib

    def tail(W, V, maxlen):
        _lib.call("sbl_beam_tail", None, 512, None, None, None, None, None, None, 64, None, None, None, None, None, None, None,
                  0, maxlen, 1, None, None, 100, 1.0, None, 2, W, V, 512, None)

    def attn(W):
        _lib.call("sbl_beam_attn_step", None, 512, None, None, 512, None, None, 512, 32, None, 32, None, 512, 2 * W, W, 8, 0, 1,
                  0.125, None)

    def finish(W, maxlen, nbest):
        _lib.call("sbl_beam_finish", None, None, None, None, None, None, None, None, None, 2, W, maxlen, nbest, 0, 1, None)

    with pytest.raises(_lib.SblHipError, match="W=17"):
        tail(17, 42, 8)
    with pytest.raises(_lib.SblHipError, match="W=17"):
        attn(17)
    with pytest.raises(_lib.SblHipError, match="W=17"):
        finish(17, 8, 1)
    with pytest.raises(_lib.SblHipError, match="W=6 above V=5"):
        tail(6, 5, 8)
    with pytest.raises(_lib.SblHipError, match="V=65"):
        tail(4, 65, 8)
    with pytest.raises(_lib.SblHipError, match="nbest=0"):
        finish(4, 8, 0)
    with pytest.raises(_lib.SblHipError, match="nbest=17"):
        finish(4, 8, 17)
    with pytest.raises(_lib.SblHipError, match="maxlen=65"):
        tail(4, 42, 65)
    with pytest.raises(_lib.SblHipError, match="maxlen=65"):
        finish(4, 65, 1)
    with pytest.raises(_lib.SblHipError, match="Lcap=65"):
        _lib.call("sbl_beam_attn_step", None, 512, None, None, 512, None, None, 512, 65, None, 65, None, 512, 4, 2, 8, 0, 1,
                  0.125, None)
    # in range: the same calls get past these checks and stop at the null pointers
    with pytest.raises(_lib.SblHipError, match="null"):
        tail(16, 64, 64)
    with pytest.raises(_lib.SblHipError, match="null"):
        finish(16, 64, 16)


def test_beam_search_has_no_cpu_path_and_checks_its_arguments():
    from sbl_for_multilingual_lip_reading_amd import _lib
    m = build_model(B.load_golden("beam_small.npz")).eval()
    enc = torch.zeros(2, 6, 512)
    with pytest.raises(_lib.SblHipError, match="no CPU path"):
        m.decoder.beam_search(enc, 3)
    with pytest.raises(_lib.SblHipError):
        m.recognize_nbest(torch.zeros(2, 6, 32, 32), None, None)
    # argument checks come before any device work; a meta tensor stands in for a device tensor here
    fake = torch.zeros(2, 6, 512, device="meta")
    m.decoder._check_encoder = lambda e: None
    for kw, pat in ((dict(beam_size=17), "beam_size = 17"), (dict(beam_size=43), "beam_size = 43"), (dict(beam_size=0), "beam_size = 0"),
                    (dict(beam_size=3, nbest=0), "nbest = 0"), (dict(beam_size=3, decode_max_len=65), "65 decode steps"),
                    (dict(beam_size=3, log_prior=torch.zeros(42, 41)), "log_prior")):
        with pytest.raises(_lib.SblHipError, match=pat):
            m.decoder.beam_search(fake, **kw)
    m.train()
    m.decoder.dropout.p = 0.1
    with pytest.raises(_lib.SblHipError, match="no dropout"):
        m.decoder.beam_search(fake, 3)


def test_surface():
    from sbl_for_multilingual_lip_reading_amd.transformer import seq2seq
    import inspect
    assert seq2seq.BeamResult._fields[:4] == ("yseq", "lengths", "scores", "n_hyps")
    sig = inspect.signature(seq2seq.Seq2SeqDecoder.beam_search)
    assert list(sig.parameters)[1:] == ["encoder_outputs", "beam_size", "nbest", "decode_max_len", "log_prior"]
    assert sig.parameters["nbest"].default == 1 and sig.parameters["decode_max_len"].default == 0
    v = inspect.signature(seq2seq.Seq2SeqTransformer.validate).parameters
    assert v["beam_size"].default is None and v["log_prior"].default is None
