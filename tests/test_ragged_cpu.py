"""CPU-side checks of ragged clips at inference: the new entry point is declared and bound, its host refusals
come before any launch, the reference fixtures are what tools/make_ragged_goldens.py promises, the float64 restatement
(tests/ragged_reference.py) is consistent with itself, and the model methods take the lengths and check them.  No launch."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import attention_routes as A
import ragged_reference as R
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sbl_attention_seg_len_fwd"
LENGTHS = {"ragged_small": ((1, 1, 4, 8, 32, 32), (8, 5, 1, 3)), "ragged_full": ((6, 6, 3, 8, 32, 32), (8, 2, 6))}


def test_header_declares_and_ctypes_binds_the_entry():
    from sbl_for_multilingual_lip_reading_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbl_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % NAME, src, flags=re.S)
    assert m, "include/sbl_hip.h does not declare " + NAME
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 20 and len(_lib.SIGNATURES[NAME]) == 20
    assert args[14] == "const int32_t* kv_len" and args[12] == "int Lk_fixed" and args[13] == "int kv_group"
    assert _lib.SIGNATURES[NAME][14] is ctypes.c_void_p
    assert hasattr(_lib.load(), NAME)


def test_host_refusals_come_before_any_launch():
    """Every refusal the header lists, through _lib.call with host dummies: nothing is dereferenced or launched."""
    from sbl_for_multilingual_lip_reading_amd import _lib
    buf = ctypes.create_string_buffer(64)
    a = (ctypes.addressof(buf) + 15) & ~15
    one, two = (ctypes.c_int * 1)(5), (ctypes.c_int * 2)(5, 3)

    def call(q=a, ldq=128, k=a, ldk=128, v=a, ldv=128, o=a, ldo=128, B=4, H=2, seg=one, nseg=1, Lk=29, kvg=1, kv_len=a, drop_p=0.0):
        _lib.call(NAME, q, ldq, k, ldk, v, ldv, o, ldo, B, H, seg, nseg, Lk, kvg, kv_len, 0.125, drop_p, None, 0, None)

    for kw, msg in ((dict(kv_len=None), "kv_len is NULL"),
                    (dict(Lk=0, seg=two, nseg=2), "one segment and kv_group 1"),
                    (dict(Lk=0, B=4, kvg=2), "one segment and kv_group 1"),
                    (dict(B=4, kvg=3), "no multiple of the group size"),
                    (dict(kvg=0), "no multiple of the group size"),
                    (dict(Lk=65), "Lk <= 64"),
                    (dict(Lk=-1), "Lk=-1"),
                    (dict(seg=(ctypes.c_int * 1)(65)), "segment 0 has L=65"),
                    (dict(seg=(ctypes.c_int * 1)(0)), "bad segment list"),
                    (dict(nseg=17), "bad segment list"),
                    (dict(ldk=64), "row stride smaller than H\\*64"),
                    (dict(ldo=130), "multiples of 4 floats"),
                    (dict(q=None), "null/unaligned pointer"),
                    (dict(v=a + 4), "null/unaligned pointer"),
                    (dict(o=a + 8), "null/unaligned pointer"),
                    (dict(drop_p=0.5), "bad dropout args")):
        with pytest.raises(_lib.SblHipError, match=msg):
            call(**kw)


@pytest.mark.parametrize("name", sorted(LENGTHS))
def test_fixture_is_what_the_tool_promises(name):
    g = load_golden(name + ".npz")
    meta, lengths = LENGTHS[name]
    assert tuple(g["meta"][:6].tolist()) == meta and tuple(g["lengths"].tolist()) == lengths and g["lengths"].dtype == np.int32
    ne, nd, B, T, H, W = meta
    assert g["clips"].shape == (B, T, H, W) and g["enc"].shape == (B, T, 512) and g["logits"].shape == (B, 2, 16, 58)
    assert g["tokens"].shape == (B, 2, 17) and g["margins"].shape == (B, 2, 16)
    for n, l in enumerate(lengths):
        assert not g["clips"][n, l:].any() and not g["enc"][n, l:].any() and g["clips"][n, :l].any() and g["enc"][n, :l].any()
    top2 = np.sort(g["logits"], -1)[..., -2:]
    assert np.array_equal(g["margins"], top2[..., 1] - top2[..., 0]) and float(g["margins"].min()) >= 10 * 1e-3
    assert np.array_equal(g["logits"].argmax(-1), g["tokens"][:, :, 1:]) and np.all(g["tokens"][:, :, 0] == 0)
    assert len({tuple(t.reshape(-1).tolist()) for t in g["tokens"]}) == B, "two clips decode alike"
    assert any(l < T and not np.array_equal(g["tokens_padded"][n], g["tokens"][n]) for n, l in enumerate(lengths))
    for f in (name + ".npz",):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "e2e_varied.npz"))


CASES = [(R.case("cpu_cross", 6, 3, (1, 2, 5), 29), (29, 1, 16, 17, 28, 2)),
         (R.case("cpu_cross_g3", 12, 3, (1, 2, 5), 29, 3), (29, 1, 16, 17)),
         (R.case("cpu_self29", 4, 2, (29,), 0), (1, 16, 17, 29)),
         (R.case("cpu_wg_cross", 3, 2, (5,), 64), (32, 33, 64)),
         (R.case("cpu_wg_self", 3, 2, (33,), 0), (33, 1, 32))]


@pytest.mark.parametrize("c,kv_len", CASES, ids=lambda v: v.name if hasattr(v, "name") else None)
def test_restatement_equals_itself_on_trimmed_kv(c, kv_len):
    """The float64 restatement with counts == the restatement of every entry alone on its K/V cut to the count, exactly, also
    when the cut rows hold NaN; it stays within its own bounds of the unragged float64 reference with a mask written out."""
    inp = R.make_inputs(c)
    o, eo = R.reference(c, inp, kv_len)
    poisoned = {n: a.copy() for n, a in inp.items()}
    for pr in A.problems(c):
        n = R.clamp(kv_len, c, pr)
        cols = slice(pr["h"] * 64, pr["h"] * 64 + 64)
        poisoned["k"][pr["krows"][n:], cols] = np.nan
        poisoned["v"][pr["krows"][n:], cols] = np.nan
    if not c.Lk:
        poisoned["q"] = inp["q"]
    o2, _ = R.reference(c, poisoned, kv_len)
    assert np.array_equal(o, o2) and np.all(np.isfinite(o))
    for e in range(R.n_entries(c)):
        sub, sinp, rows = R.trimmed(c, inp, kv_len, e)
        so, seo = R.reference(sub, sinp, (sub.Lk,) * R.n_entries(sub))
        assert np.array_equal(o[rows], so) and np.array_equal(eo[rows], seo)
    # against attention_routes.reference under an explicit mask (the whole-row float64 sums of the unragged code)
    if c.Lk and len(c.segL) == 1 and c.kvg == 1:
        m = A.Case(c.name, "seg", c.B, c.H, c.segL, c.Lk, "tensor", 1, (), None, None)
        mask = (np.arange(c.Lk)[None, None, :] >= np.array(kv_len)[:, None, None]).astype(np.uint8).repeat(c.segL[0], 1)
        full = A.reference(m, dict(inp, mask=mask, do=np.zeros_like(inp["q"])))["o"]
        assert np.all(np.abs(full[0] - o) <= full[1] + eo)


def test_counts_clamp_and_zero():
    c = R.case("cpu_clamp", 6, 2, (3,), 29)
    inp = R.make_inputs(c)
    o, eo = R.reference(c, inp, (0, -3, 40, 29, 16, 1))
    want, _ = R.reference(c, inp, (0, 0, 29, 29, 16, 1))
    assert np.array_equal(o, want)
    assert not o[:6].any() and not eo[:6].any() and o[6:].any()      # sequences 0 and 1 (3 rows each): exact zeros


def test_routes_of_the_gpu_cases():
    """The shapes tests/test_ragged_gpu.py uses land on the kernel they are meant for (host dispatch restated in
    attention_routes.py; the new entry dispatches as the grouped one, self-attention by seg_L[0])."""
    for segL, Lk, want in (((1, 2, 5), 29, "small"), ((16,), 0, "small"), ((29,), 0, "qtile"), ((32,), 0, "qtile"),
                           ((5,), 33, "workgroup"), ((5,), 64, "workgroup"), ((33,), 0, "workgroup")):
        assert R.route(R.case("r", 6, 3, segL, Lk)) == want, (segL, Lk)


def test_methods_take_the_lengths():
    from sbl_for_multilingual_lip_reading_amd import ops
    from sbl_for_multilingual_lip_reading_amd.transformer.attention import MultiHeadAttention
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    from sbl_for_multilingual_lip_reading_amd.transformer.transformer import Transformer
    for n in ("recognize", "recognize_nbest", "validate", "recognize_words", "validate_words", "recognize_words_lex", "validate_words_lex"):
        p = inspect.signature(getattr(Transformer, n)).parameters
        assert "input_lengths" in p and p["input_lengths"].default is None, n
    for n in ("recognize_beam", "beam_search", "score_pairs", "recognize_words", "beam_search_lex"):
        p = inspect.signature(getattr(Decoder, n)).parameters
        assert "encoder_input_lengths" in p and p["encoder_input_lengths"].default is None, n
    assert "input_lengths" not in inspect.signature(Transformer.forward).parameters      # training is not changed
    for f in (ops.attn_fwd, MultiHeadAttention.forward_rows):
        assert inspect.signature(f).parameters["kv_len"].default is None


def test_host_lengths_are_checked_before_anything_runs():
    from sbl_for_multilingual_lip_reading_amd import _lib
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    from sbl_for_multilingual_lip_reading_amd.transformer.transformer import Transformer
    m = Transformer(Encoder(512, 1, 8, 64, 64, 512, 2048), Decoder(0, 1, 58, 512, 1, 8, 64, 64, 512, 2048), None).eval()
    x = torch.zeros(3, 8, 32, 32)
    with torch.no_grad():
        for bad in ([8, 5], [8, 5, 1, 3], [8, 0, 3], [8, 9, 3], torch.tensor([8, -1, 3]), torch.tensor([9, 8, 8], dtype=torch.int32)):
            with pytest.raises(ValueError, match="input_lengths"):
                m.recognize(x, bad)
            with pytest.raises(ValueError, match="input_lengths"):
                m.validate_words_lex(x, None, None, None, input_lengths=bad)
        with pytest.raises(_lib.SblHipError, match="no CPU path"):      # good lengths get as far as the first kernel
            m.recognize(x, [8, 5, 1])
