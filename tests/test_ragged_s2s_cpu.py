"""CPU-side checks of ragged clips in the single-direction baseline: the new entry points are declared and
bound, their host refusals come before any launch, the reference fixtures are what tools/make_ragged_s2s_goldens.py promises,
the restatement (tests/ragged_s2s_oracle.py) reproduces them, the unseen salts of the GPU tests meet the margin floors, and
the model methods take the lengths and check them before anything runs.  No launch."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import beam_oracle as B
import ragged_s2s_oracle as R
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"sbl_decode_attn_step_len": (18, 16, "const int32_t* kv_len"), "sbl_beam_attn_step_len": (21, 19, "const int32_t* kv_len"),
           "sbl_beam_tail_len": (30, 28, "const int32_t* clip_steps"), "sbl_beam_finish_len": (17, 15, "const int32_t* clip_steps")}


def test_header_declares_and_ctypes_binds_the_entries():
    from sbl_for_multilingual_lip_reading_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbl_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, (nargs, at, decl) in ENTRIES.items():
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert m, "include/sbl_hip.h does not declare " + name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs == len(_lib.SIGNATURES[name]) and args[at] == decl, name
        # the arguments of the entry without counts, then the counts, then the stream
        base = _lib.SIGNATURES[name[:-4]]
        assert _lib.SIGNATURES[name] == base[:-1] + [ctypes.c_void_p] + base[-1:] and hasattr(lib, name)
    assert lib.sbl_abi_version() == 1


def test_host_refusals_come_before_any_launch():
    """Through _lib.call with host dummies: nothing is dereferenced or launched."""
    from sbl_for_multilingual_lip_reading_amd import _lib
    buf = ctypes.create_string_buffer(64)
    a = (ctypes.addressof(buf) + 15) & ~15

    def dec(q=a, ldq=512, ldc=512, Lcap=29, o=a, ldo=512, B_=4, Hh=8, n_prev=29, append=0, kv_len=a):
        _lib.call("sbl_decode_attn_step_len", q, ldq, None, None, 0, a, a, ldc, Lcap, o, ldo, B_, Hh, n_prev, append, 0.125, kv_len, None)

    def beam(S=6, W=3, Lcap=29, n_prev=29, append=0, kv_len=a, ldq=512):
        _lib.call("sbl_beam_attn_step_len", a, ldq, None, None, 0, a, a, 512, Lcap, None, 0, a, 512, S, W, 8, n_prev, append, 0.125, kv_len,
                  None)

    for fn, kw, msg in ((dec, dict(kv_len=None), "sbl_decode_attn_step_len: kv_len is NULL"),
                        (dec, dict(append=1), "sbl_decode_attn_step_len: append=1"),
                        (dec, dict(Lcap=65), "Lcap=65"), (dec, dict(n_prev=30), "do not fit Lcap=29"), (dec, dict(n_prev=0), "do not fit"),
                        (dec, dict(q=None), "null pointer"), (dec, dict(ldo=256), "row stride below H\\*64"),
                        (dec, dict(ldq=514), "unaligned"), (dec, dict(q=a + 4), "unaligned"), (dec, dict(B_=0), "B=0"),
                        (beam, dict(kv_len=None), "sbl_beam_attn_step_len: kv_len is NULL"),
                        (beam, dict(append=1), "sbl_beam_attn_step_len: append=1"),
                        (beam, dict(W=17, S=17), "beam W=17"), (beam, dict(S=7), "S a multiple of W=3"), (beam, dict(Lcap=0), "Lcap=0")):
        with pytest.raises(_lib.SblHipError, match=msg):
            fn(**kw)

    def tail(clip_steps=a, W=3, maxlen=8, step=0, V=48):
        _lib.call("sbl_beam_tail_len", a, 512, a, None, a, a, a, a + 16, 64, a, a, a, a, a, a, a, step, maxlen, 1, None, None, 0, 1.0, None,
                  2, W, V, 512, clip_steps, None)

    def finish(clip_steps=a, W=3, maxlen=8, nbest=2):
        _lib.call("sbl_beam_finish_len", a, a, a, a, a, a, a, a, a, 2, W, maxlen, nbest, 0, 1, clip_steps, None)

    for fn, kw, msg in ((tail, dict(clip_steps=None), "sbl_beam_tail_len: clip_steps is NULL"), (tail, dict(W=17), "sbl_beam_tail_len: beam W=17"),
                        (tail, dict(maxlen=65), "maxlen=65"), (tail, dict(step=8), "step 8 of 8"), (tail, dict(V=65), "V=65"),
                        (finish, dict(clip_steps=None), "sbl_beam_finish_len: clip_steps is NULL"),
                        (finish, dict(W=17), "sbl_beam_finish_len: beam W=17"), (finish, dict(nbest=17), "nbest=17"),
                        (finish, dict(maxlen=0), "maxlen=0")):
        with pytest.raises(_lib.SblHipError, match=msg):
            fn(**kw)


def test_greedy_fixture_is_what_the_tool_promises_and_the_restatement_reproduces_it():
    g = load_golden("ragged_s2s_small.npz")
    assert tuple(g["meta"][:8].tolist()) == (1, 1, 42, 1, 4, 8, 32, 32) and tuple(g["lengths"].tolist()) == (8, 5, 1, 3)
    assert g["lengths"].dtype == np.int32
    Bn, T, V = 4, 8, 42
    assert g["clips"].shape == (Bn, T, 32, 32) and g["enc"].shape == (Bn, T, 512) and g["logits"].shape == (Bn, T, V)
    assert g["tokens"].shape == (Bn, T + 1) and g["margins"].shape == (Bn, T)
    for n, l in enumerate(g["lengths"]):
        assert not g["clips"][n, l:].any() and not g["enc"][n, l:].any() and g["clips"][n, :l].any() and g["enc"][n, :l].any()
        assert not g["logits"][n, l:].any() and np.all(g["tokens"][n, l + 1:] == 1) and g["tokens"][n, 0] == 0
        assert np.array_equal(g["logits"][n, :l].argmax(-1), g["tokens"][n, 1:l + 1]) and np.all(np.isinf(g["margins"][n, l:]))
        top2 = np.sort(g["logits"][n, :l], -1)[:, -2:]
        assert np.array_equal(g["margins"][n, :l], top2[:, 1] - top2[:, 0])
    assert float(g["margins"].min()) >= R.MIN_MARGIN
    assert len({tuple(t.tolist()) for t in g["tokens"]}) == Bn, "two clips decode alike"
    assert any(l < T and not np.array_equal(g["tokens_padded"][n, :l + 1], g["tokens"][n, :l + 1]) for n, l in enumerate(g["lengths"]))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ragged_s2s_small.npz")) < 200 * 1024
    _, x, o = R.oracle_case("ragged_s2s_small")
    assert np.array_equal(x.numpy(), g["clips"]) and np.array_equal(o["tokens"], g["tokens"])
    assert float(np.abs(o["logits"] - g["logits"]).max()) < 1e-3 and float(np.abs(o["enc"] - g["enc"]).max()) < 1e-3


def test_beam_fixture_is_what_the_tool_promises_and_the_restatement_reproduces_it():
    g = load_golden("ragged_s2s_beam.npz")
    assert tuple(g["meta"][:8].tolist()) == (1, 2, 48, 0, 4, 8, 32, 32) and tuple(g["lengths"].tolist()) == (8, 5, 2, 3)
    assert tuple(g["beam"].tolist()) == (5, 2, 0) and g["freq"].shape == (48, 48)
    Bn, T, W, nbest = 4, 8, 5, 2
    assert g["yseq"].shape == (Bn, nbest, T + 2) and g["hist_flag"].shape == (Bn, T, W)
    assert float(g["margin"]) >= B.margin_floor(T)
    for n, l in enumerate(g["lengths"]):
        assert not g["clips"][n, l:].any() and not g["enc"][n, l:].any()
        assert not g["hist_flag"][n, l:].any() and np.all(np.isneginf(g["hist_score"][n, l:]))
        last = g["hist_flag"][n, l - 1]
        assert np.all(last[last != 0] == 2)
        for k in range(int(g["n_hyps"][n])):
            hl = int(g["hyp_lengths"][n, k])
            assert 2 <= hl <= l + 2 and np.all(g["yseq"][n, k, hl:] == 1) and g["yseq"][n, k, hl - 1] == 1
    assert (g["hyp_lengths"][:, 0] == g["lengths"] + 2).any(), "no 1-best was ended by its clip's last step"
    for a in range(Bn):
        for b in range(a):
            assert not np.array_equal(g["yseq"][a, 0], g["yseq"][b, 0]) or np.abs(g["scores"][a] - g["scores"][b]).max() > B.margin_floor(T)
    assert any(l < T and not np.array_equal(g["yseq_padded"][n], g["yseq"][n, 0]) for n, l in enumerate(g["lengths"]))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ragged_s2s_beam.npz")) < 200 * 1024
    _, x, o = R.oracle_case("ragged_s2s_beam")
    assert np.array_equal(x.numpy(), g["clips"])
    for k in ("yseq", "n_hyps", "hist_tok", "hist_par", "hist_flag"):
        assert np.array_equal(o[k], g[k]), k
    assert np.array_equal(o["lengths"], g["hyp_lengths"])
    assert float(np.abs(np.where(np.isfinite(g["scores"]), o["scores"] - g["scores"], 0)).max()) < 1e-4
    assert float(np.abs(o["enc"] - g["enc"]).max()) < 1e-3


def test_unseen_salts_meet_the_margin_floors():
    """So that no GPU case is ever skipped: the re-salted cases of test_ragged_s2s_gpu.py are decided by gaps of at least ten
    tolerances, their clips decode differently, and an n-best hypothesis is ended by its clip's last step."""
    g, _, o = R.oracle_case("ragged_s2s_small", R.UNSEEN_SALTS["ragged_s2s_small"])
    assert float(o["margins"].min()) >= R.MIN_MARGIN and len({tuple(t.tolist()) for t in o["tokens"]}) == 4
    g, _, o = R.oracle_case("ragged_s2s_beam", R.UNSEEN_SALTS["ragged_s2s_beam"])
    assert float(o["margin"]) >= B.margin_floor(8)
    assert (o["lengths"] == g["lengths"][:, None] + 2).any()


def test_methods_take_the_lengths():
    from sbl_for_multilingual_lip_reading_amd import ops
    from sbl_for_multilingual_lip_reading_amd.transformer.seq2seq import Seq2SeqDecoder, Seq2SeqTransformer
    for n in ("recognize", "recognize_nbest", "validate", "forward", "_encode", "recognize_words_len", "validate_words_len"):
        p = inspect.signature(getattr(Seq2SeqTransformer, n)).parameters
        assert "input_lengths" in p, n
        assert n.endswith("_len") or p["input_lengths"].default is None, n
    p = inspect.signature(Seq2SeqDecoder.recognize_beam).parameters
    assert p["encoder_input_lengths"].default is None and p["cached"].default is True
    for n in ("beam_search_len", "recognize_words_len"):
        assert list(inspect.signature(getattr(Seq2SeqDecoder, n)).parameters)[2] == "encoder_input_lengths", n
    for f in (ops.decode_attn_step, ops.beam_attn_step):
        assert inspect.signature(f).parameters["kv_len"].default is None
    for f in (ops.beam_tail, ops.beam_finish):
        assert inspect.signature(f).parameters["clip_steps"].default is None
    assert list(inspect.signature(ops.BeamState.__init__).parameters) == ["self", "N", "W", "maxlen", "sos_id", "device", "lex"]


def test_host_lengths_are_checked_before_anything_runs():
    from sbl_for_multilingual_lip_reading_amd import _lib
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    from sbl_for_multilingual_lip_reading_amd.transformer.seq2seq import Seq2SeqDecoder, Seq2SeqTransformer
    m = Seq2SeqTransformer(Encoder(512, 1, 8, 64, 64, 512, 2048), Seq2SeqDecoder(0, 1, 42, 512, 1, 8, 64, 64, 512, 2048)).eval()
    x = torch.zeros(3, 8, 32, 32)
    with torch.no_grad():
        for bad in ([8, 5], [8, 5, 1, 3], [8, 0, 3], [8, 9, 3], torch.tensor([8, -1, 3]), torch.tensor([9, 8, 8], dtype=torch.int32)):
            for call in (lambda: m.recognize(x, input_lengths=bad), lambda: m.recognize(x, cached=False, input_lengths=bad),
                         lambda: m.recognize_nbest(x, None, None, input_lengths=bad), lambda: m.validate(x, None, None, input_lengths=bad),
                         lambda: m.validate(x, None, None, beam_size=3, input_lengths=bad),
                         lambda: m.recognize_words_len(x, bad, None), lambda: m.validate_words_len(x, bad, None, None, None)):
                with pytest.raises(ValueError, match="input_lengths"):
                    call()
        with pytest.raises(_lib.SblHipError, match="no CPU path"):      # good lengths get as far as the first kernel
            m.recognize(x, input_lengths=[8, 5, 1])
    with pytest.raises(_lib.SblHipError, match="key counts go with the cross-attention"):
        from sbl_for_multilingual_lip_reading_amd import ops
        t = torch.zeros(2, 512, device="meta")
        ops.decode_attn_step(t, t, t, torch.zeros(2, 4, 512, device="meta"), torch.zeros(2, 4, 512, device="meta"), 4, t, 8, 0, True,
                             kv_len=torch.zeros(2, dtype=torch.int32, device="meta"))
