"""CPU-side checks of the single-direction seq2seq model: the plain-torch restatement (tests/seq2seq_oracle.py) reproduces
every fixture the REFERENCE wrote (tests/golden/s2s_*.npz, tools/make_seq2seq_goldens.py), the model's surface equals the
reference's recorded key list, the tied weight is one parameter and one flat-buffer slot, the header declares the new
entry points, and nothing computes without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden, maxdiff
import seq2seq_oracle as S
from oracle import sbl_oracle as O

CASES = ("s2s_small", "s2s_varied", "s2s_full")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_model(g):
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    from sbl_for_multilingual_lip_reading_amd.transformer.seq2seq import Seq2SeqDecoder, Seq2SeqTransformer
    c = S.case_config(g)
    return Seq2SeqTransformer(Encoder(512, c["ne"], 8, 64, 64, 512, 2048, dropout=0.0),
                              Seq2SeqDecoder(0, 1, c["vocab"], 512, c["nd"], 8, 64, 64, 512, 2048, dropout=0.0,
                                             tgt_emb_prj_weight_sharing=c["share"]))


@pytest.mark.parametrize("case", CASES)
def test_oracle_reproduces_reference_fixture(case):
    """Logits < 2e-4 and loss < 2e-5, the bounds of tests/test_oracle_golden.py for the SBL end-to-end fixtures; preprocess
    and greedy tokens exact.  The generator's margin assert is re-checked on the stored margins."""
    g = load_golden(case + ".npz")
    c = S.case_config(g)
    assert float(g["margins"].min()) >= 10 * 1e-3 and g["margins"].shape == (c["B"], c["T"])
    lens = (g["tgt"] != -1).sum(1)
    assert lens[0] == 1 and lens[1] == 13 and g["tgt"].shape[1] == 13
    x, tgt = S.case_inputs(g)
    ys_in, ys_out = S.preprocess(tgt)
    assert np.array_equal(ys_in.numpy(), g["ys_in"]) and np.array_equal(ys_out.numpy(), g["ys_out"])
    with torch.no_grad():
        sd = S.case_state(g)
        ys, logits = S.recognize_beam(sd, S.encode(sd, x, c["ne"], training=False), c["nd"], c["scale"])
    assert np.array_equal(ys.numpy(), g["tokens"])
    top2 = logits.topk(2, dim=-1).values
    assert maxdiff(top2[..., 0] - top2[..., 1], g["margins"]) < 2e-4
    sd = S.case_state(g, requires_grad=True)
    pred, gold = S.decoder_forward(sd, tgt, S.encode(sd, x, c["ne"], training=True), c["nd"], c["scale"])
    assert np.array_equal(gold.numpy(), g["gold"])
    assert maxdiff(pred, g["pred"]) < 2e-4
    loss, n_correct = O.cal_performance(pred, gold, 0.1)
    assert abs(loss.item() - float(g["loss"])) < 2e-5 and int(n_correct) == int(g["n_correct"])
    loss.backward()
    for k in g.files:
        if k.startswith("grad:decoder") or k.startswith("grad:encoder"):
            ref = g[k]
            assert maxdiff(S.sub(sd[k[5:]].grad), ref) < 2e-3 * float(np.abs(ref).max()) + 2e-6, k


@pytest.mark.parametrize("case", CASES)
def test_state_dict_surface_and_preprocess(case):
    g = load_golden(case + ".npz")
    m = build_model(g)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    for k, shp in zip(g["keys"], g["shapes"]):
        assert ",".join(str(d) for d in sd[str(k)].shape) == str(shp), str(k)
    assert [n for n, _ in m.named_parameters()] == [str(n) for n in g["param_names"]]
    ys_in, ys_out = m.decoder.preprocess(torch.from_numpy(g["tgt"]))
    assert np.array_equal(ys_in.numpy(), g["ys_in"]) and np.array_equal(ys_out.numpy(), g["ys_out"])
    # interior IGNORE_IDs are stripped too (y[y != IGNORE_ID])
    yi, yo = m.decoder.preprocess(torch.tensor([[5, -1, 7, -1, -1, 9, -1, -1, -1, -1, -1, -1, -1]]))
    assert yi[0].tolist() == [0, 5, 7, 9] + [1] * 10 and yo[0].tolist() == [5, 7, 9, 1] + [-1] * 10


def test_tied_weight_is_one_parameter_and_one_flat_slot():
    from sbl_for_multilingual_lip_reading_amd import dp
    m = build_model(load_golden("s2s_small.npz"))
    dec = m.decoder
    assert dec.tgt_word_prj.weight is dec.tgt_word_emb.weight and dec.x_logit_scale == 512 ** -0.5
    n_params = len(list(m.parameters()))
    flat = dp.FlatModel(m)
    assert flat.segments[0] == "decoder." and flat.segments[-1] == "lipreading."
    assert len(flat.slots) == n_params and sum(1 for p, _, _ in flat.slots if p is dec.tgt_word_emb.weight) == 1
    assert dec.tgt_word_prj.weight.data_ptr() == dec.tgt_word_emb.weight.data_ptr()
    a, b = flat.ranges["decoder."]
    off = next(o for p, o, _ in flat.slots if p is dec.tgt_word_emb.weight)
    assert a <= off < b
    # the cross-attention K/V rows of all layers are one block
    mods = dec.cross_attention_modules()
    ws = [w for mod in mods for w in (mod.w_ks.weight, mod.w_vs.weight)]
    assert all(y.data_ptr() == x.data_ptr() + x.numel() * 4 for x, y in zip(ws, ws[1:]))
    # untied: two parameters, scale 1
    m2 = build_model(load_golden("s2s_varied.npz"))
    assert m2.decoder.tgt_word_prj.weight is not m2.decoder.tgt_word_emb.weight and m2.decoder.x_logit_scale == 1.0
    assert len(dp.FlatModel(m2).slots) == len(list(m2.parameters()))


def test_header_declares_new_entry_points():
    from sbl_for_multilingual_lip_reading_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbl_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("sbl_decode_attn_step", "sbl_decode_tail", "sbl_embed_scale_pe_fwd", "sbl_embed_scale_bwd", "sbl_seq_score1"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    # host-side validation, before any launch
    with pytest.raises(_lib.SblHipError, match="Lcap=65"):
        _lib.call("sbl_decode_attn_step", None, 512, None, None, 512, None, None, 512, 65, None, 512, 1, 8, 0, 1, 0.125, None)
    with pytest.raises(_lib.SblHipError, match="do not fit"):
        _lib.call("sbl_decode_attn_step", None, 512, None, None, 512, None, None, 512, 32, None, 512, 1, 8, 32, 1, 0.125, None)
    with pytest.raises(_lib.SblHipError, match="V <= 64"):
        _lib.call("sbl_decode_tail", None, 512, None, None, 0, None, 30, 0, None, None, 0, 1.0, None, 2, 65, 512, None)


def test_no_cpu_path_and_host_checks():
    from sbl_for_multilingual_lip_reading_amd import _lib
    from sbl_for_multilingual_lip_reading_amd.transformer.seq2seq import Seq2SeqDecoder
    g = load_golden("s2s_small.npz")
    m = build_model(g)
    x, tgt = S.case_inputs(g)
    with pytest.raises(_lib.SblHipError):
        m(x, tgt)
    with pytest.raises(_lib.SblHipError):
        m.recognize(x)
    with pytest.raises(_lib.SblHipError, match="no CPU path"):
        m.decoder(tgt, torch.zeros(4, 6, 512), [6] * 4)
    with pytest.raises(_lib.SblHipError, match="no CPU path"):
        m.decoder.recognize_beam(torch.zeros(4, 6, 512))
    with pytest.raises(_lib.SblHipError, match="d_model"):
        Seq2SeqDecoder(0, 1, 42, 256, 1, 8, 64, 64, 256, 2048)
    with pytest.raises(_lib.SblHipError, match="at most 13"):
        m.decoder.preprocess(torch.zeros(2, 14, dtype=torch.long))


def test_single_direction_meter_matches_two_direction_rows():
    """update_single scores exactly what the first row of the two-direction update scores (CPU definition)."""
    from sbl_for_multilingual_lip_reading_amd.transformer.metrics import ErrorRateMeter
    torch.manual_seed(3)
    ys = torch.randint(0, 42, (9, 30))
    gold = torch.randint(2, 42, (9, 13))
    gold[torch.arange(13).unsqueeze(0) >= torch.randint(0, 14, (9, 1))] = -1
    a, b = ErrorRateMeter(device="cpu"), ErrorRateMeter(device="cpu")
    a.update_single(ys, gold)
    b.update(ys, ys, gold, gold)
    assert torch.equal(a.acc[0], b.acc[0]) and int(a.acc[1].sum()) == 0
    r = a.result()
    assert r["wer"] == r["l2r_wer"] and r["per"] == r["l2r_per"] and r["per_corpus"] == r["l2r_per_corpus"]
    assert r["n"] + r["n_empty"] == 9 and "wer" not in b.result()


def test_checkpoint_round_trip_and_stage1_hand_off(tmp_path):
    """save / load keeps every entry and the tie; a stage-1 classifier checkpoint initialises frontend and encoder through
    prefix_map={"visual_frontend.": "lipreading.", "encoder_v.": "encoder."}."""
    from sbl_for_multilingual_lip_reading_amd import checkpoint
    from sbl_for_multilingual_lip_reading_amd.transformer.classifier import ClassifierTransformer
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    g = load_golden("s2s_small.npz")
    torch.manual_seed(1)
    a = build_model(g)
    torch.manual_seed(2)
    b = build_model(g)
    path = str(tmp_path / "s2s.pt")
    checkpoint.save_checkpoint(path, a, epoch=3)
    assert checkpoint.load_checkpoint(path, b)["epoch"] == 3
    for (k, v), (_, w) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(v, w), k
    assert b.decoder.tgt_word_prj.weight is b.decoder.tgt_word_emb.weight
    cls = ClassifierTransformer(Encoder(512, 1, 8, 64, 64, 512, 2048), None)
    path1 = str(tmp_path / "stage1.pt")
    checkpoint.save_checkpoint(path1, cls)
    checkpoint.load_checkpoint(path1, b, strict=False, prefix_map={"visual_frontend.": "lipreading.", "encoder_v.": "encoder."})
    sd_b, sd_c = b.state_dict(), cls.state_dict()
    for k, v in sd_c.items():
        if k.startswith("visual_frontend."):
            assert torch.equal(sd_b["lipreading." + k[len("visual_frontend."):]], v), k
        elif k.startswith("encoder_v."):
            assert torch.equal(sd_b["encoder." + k[len("encoder_v."):]], v), k
    assert torch.equal(sd_b["decoder.tgt_word_emb.weight"], a.state_dict()["decoder.tgt_word_emb.weight"])
