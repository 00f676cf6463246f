"""Stage-1 classification pre-training without a GPU: the classifier model's surface, the host-side argument checks of the
head entry points, the flat-buffer layouts of both models, and the stage 1 -> 2 checkpoint hand-off."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import sbl_oracle as O


def _cls_shapes(n_enc):
    """The CLS state-dict shapes test_oracle_golden.test_cls_config1 derives from the oracle, in registration order:
    frontend, encoder_v, fc_1500, fc_2 (the computed `pe` buffer aside)."""
    shapes = {k: v for k, v in O.state_dict_shapes(n_enc, 1).items() if k.startswith("visual_frontend.")}
    for k, v in O.state_dict_shapes(n_enc, 1).items():
        if k.startswith("encoder."):
            shapes["encoder_v." + k[len("encoder."):]] = v
    shapes.update({"fc_1500.weight": (1500, 512), "fc_1500.bias": (1500,), "fc_2.weight": (2, 512), "fc_2.bias": (2,)})
    return shapes


def _classifier(n_enc, seed=0):
    from sbl_for_multilingual_lip_reading_amd.transformer.classifier import ClassifierTransformer
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    torch.manual_seed(seed)
    return ClassifierTransformer(Encoder(512, n_enc, 8, 64, 64, 512, 2048), None)


def _sbl(n_enc, n_dec, seed=0):
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    from sbl_for_multilingual_lip_reading_amd.transformer.transformer import Transformer
    torch.manual_seed(seed)
    return Transformer(Encoder(512, n_enc, 8, 64, 64, 512, 2048), Decoder(0, 1, 58, 512, n_dec, 8, 64, 64, 512, 2048), None)


@pytest.mark.parametrize("n_enc", [6, 3])
def test_classifier_state_dict_matches_cls_shapes(n_enc):
    m = _classifier(n_enc)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items() if not k.endswith(".pe")]
    assert got == [(k, tuple(v)) for k, v in _cls_shapes(n_enc).items()]
    assert tuple(m.state_dict()["encoder_v.positional_encoding.pe"].shape) == (1, 5000, 512)


def test_classifier_keeps_its_own_initialisation():
    """The CLS reference re-draws nothing after construction (the SBL Transformer re-draws Xavier): fc_1500 keeps
    nn.Linear's own uniform(+-1/sqrt(512)) bias, which a Xavier re-draw of rank >= 2 tensors would not touch, and its
    weight stays inside nn.Linear's bound, tighter than Xavier's for a 512 x 1500 matrix."""
    m = _classifier(1, seed=3)
    bound = 1 / 512 ** 0.5
    w, b = m.fc_1500.weight.detach(), m.fc_1500.bias.detach()
    assert 0.9 * bound < float(w.abs().max()) <= bound
    assert float(b.abs().max()) <= bound


def test_new_symbols_are_exported_and_bound():
    from sbl_for_multilingual_lip_reading_amd import _lib, transformer
    from sbl_for_multilingual_lip_reading_amd.transformer import ClassifierTransformer, cal_cls_loss, cls_accuracy  # noqa: F401
    assert set(transformer.__all__) >= {"ClassifierTransformer", "cal_cls_loss", "cls_accuracy"}
    lib = _lib.load()
    assert lib.sbl_abi_version() == 1
    for name in ("sbl_cls_head_fwd", "sbl_cls_loss_fwd", "sbl_cls_loss_bwd", "sbl_cls_head_bwd"):
        assert name in _lib.SIGNATURES and getattr(lib, name).restype is not None


def _ptr():
    """A fake, 16-byte aligned device address: the calls below must fail validation before anything dereferences it."""
    return 1 << 20


def test_head_entry_points_reject_bad_arguments_on_the_host():
    from sbl_for_multilingual_lip_reading_amd import _lib
    p = _ptr()
    fwd = lambda N, T, li, ptr=p: _lib.call("sbl_cls_head_fwd", *([ptr] * 9), N, T, 512, 1500, 2, li, None)
    with pytest.raises(_lib.SblHipError, match="N = 0"):
        fwd(0, 31, 30)
    with pytest.raises(_lib.SblHipError, match="N = -3"):
        fwd(-3, 31, 30)
    with pytest.raises(_lib.SblHipError, match=r"lang_index = 31 outside \[0, T = 31\)"):
        fwd(4, 31, 31)
    with pytest.raises(_lib.SblHipError, match="lang_index = -1"):
        fwd(4, 31, -1)
    with pytest.raises(_lib.SblHipError, match="null pointer"):
        fwd(4, 31, 30, None)
    with pytest.raises(_lib.SblHipError, match="D = 256"):
        _lib.call("sbl_cls_head_fwd", *([p] * 9), 4, 31, 256, 1500, 2, 30, None)
    bwd = lambda N, T, li, ptr=p: _lib.call("sbl_cls_head_bwd", *([ptr] * 11), N, T, 512, 1500, 2, li, 1, None)
    with pytest.raises(_lib.SblHipError, match="N = 0"):
        bwd(0, 31, 30)
    with pytest.raises(_lib.SblHipError, match="lang_index = 31"):
        bwd(2, 31, 31)
    with pytest.raises(_lib.SblHipError, match="null pointer"):
        bwd(2, 31, 30, None)
    loss_fwd = lambda N, ptr=p: _lib.call("sbl_cls_loss_fwd", *([ptr] * 4), N, 1500, 2, 0.1, -100, ptr, ptr, None)
    loss_bwd = lambda N, ptr=p: _lib.call("sbl_cls_loss_bwd", *([ptr] * 8), N, 1500, 2, 0.1, -100, None)
    for call in (loss_fwd, loss_bwd):
        with pytest.raises(_lib.SblHipError, match="N = 0"):
            call(0)
        with pytest.raises(_lib.SblHipError, match="null pointer"):
            call(3, None)


def test_head_entry_points_reject_documented_limits_on_the_host():
    """The rejections include/sbl_hip.h documents beyond N, lang_index and D: the class counts (C2 <= 16), T, accumulate, the
    16-byte alignment of the operands read or written as vectors, and the inputs each requested gradient needs."""
    from sbl_for_multilingual_lip_reading_amd import _lib
    p = _ptr()

    def fwd(T=31, C1=1500, C2=2, li=0, **ptr):
        a = {k: ptr.get(k, p) for k in ("enc", "w1", "b1", "w2", "b2", "pooled", "pooled_t", "l1", "l2")}
        return _lib.call("sbl_cls_head_fwd", *a.values(), 4, T, 512, C1, C2, li, None)

    def bwd(T=31, C1=1500, C2=2, li=0, acc=1, **ptr):
        a = {k: ptr.get(k, p) for k in ("enc", "pooled", "d1", "d2", "w1", "w2", "d_enc", "dw1", "db1", "dw2", "db2")}
        return _lib.call("sbl_cls_head_bwd", *a.values(), 4, T, 512, C1, C2, li, acc, None)

    for call in (fwd, bwd):
        with pytest.raises(_lib.SblHipError, match=r"C1 = 1500, C2 = 17 classes \(need C1 >= 1, 1 <= C2 <= 16\)"):
            call(C2=17)
        with pytest.raises(_lib.SblHipError, match="C1 = 1500, C2 = 0 classes"):
            call(C2=0)
        with pytest.raises(_lib.SblHipError, match="C1 = 0, C2 = 2 classes"):
            call(C1=0)
        with pytest.raises(_lib.SblHipError, match="T = 0 frames"):
            call(T=0)
    for name in ("enc", "w1", "pooled"):
        with pytest.raises(_lib.SblHipError, match="sbl_cls_head_fwd: enc, w1, w2 and pooled must be 16-byte aligned"):
            fwd(**{name: p + 4})
    for name in ("enc", "w1", "pooled", "dw1"):
        with pytest.raises(_lib.SblHipError, match="sbl_cls_head_bwd: enc, pooled, w1, dw1 and dw2 must be 16-byte aligned"):
            bwd(**{name: p + 8})
    with pytest.raises(_lib.SblHipError, match=r"accumulate = 2 \(0 or 1\)"):
        bwd(acc=2)
    with pytest.raises(_lib.SblHipError, match=r"null pointer \(pooled, needed for dW1 / db1\)"):
        bwd(pooled=None, db1=None, dw2=None, db2=None, d_enc=None)            # dw1 alone asks for it
    with pytest.raises(_lib.SblHipError, match=r"null pointer \(enc, needed for dW2 / db2\)"):
        bwd(enc=None, dw1=None, db1=None, db2=None, d_enc=None)
    with pytest.raises(_lib.SblHipError, match=r"null pointer \(w1 / w2, needed for d_enc\)"):
        bwd(w1=None, dw1=None, db1=None, dw2=None, db2=None)
    # nothing asked for: nothing launched, nothing needed but the two gradients' addresses
    none = dict(d_enc=None, dw1=None, db1=None, dw2=None, db2=None)
    assert bwd(**none) is None
    assert bwd(enc=None, pooled=None, w1=None, w2=None, acc=0, **none) is None
    with pytest.raises(_lib.SblHipError, match=r"null pointer \(dlogits1 / dlogits2\)"):
        bwd(d1=None, **none)
    loss_fwd = lambda C1, C2: _lib.call("sbl_cls_loss_fwd", *([p] * 4), 3, C1, C2, 0.1, -100, p, p, None)
    loss_bwd = lambda C1, C2: _lib.call("sbl_cls_loss_bwd", *([p] * 8), 3, C1, C2, 0.1, -100, None)
    for call in (loss_fwd, loss_bwd):
        with pytest.raises(_lib.SblHipError, match=r"C1 = 0, C2 = 2 classes \(must be >= 1\)"):
            call(0, 2)
        with pytest.raises(_lib.SblHipError, match="C1 = 9, C2 = 0 classes"):
            call(9, 0)


def test_autograd_functions_refuse_cpu_tensors():
    from sbl_for_multilingual_lip_reading_amd import _lib, ops
    enc = torch.zeros(2, 3, 512)
    with pytest.raises(_lib.SblHipError, match="no CPU path"):
        ops.ClsHeadFn.apply(enc, torch.zeros(1500, 512), torch.zeros(1500), torch.zeros(2, 512), torch.zeros(2), 2)
    with pytest.raises(_lib.SblHipError, match="no CPU path"):
        ops.ClsLossFn.apply(torch.zeros(2, 1500), torch.zeros(2, 2), torch.zeros(2, dtype=torch.long),
                            torch.zeros(2, dtype=torch.long), 0.1, -100)


def test_sbl_flat_layout_is_unchanged():
    """The SBL model's flat buffers, slot by slot, as the base commit laid them out (tests/golden/flat_layout_sbl.npz:
    475 slots, 80,898,240 elements)."""
    from sbl_for_multilingual_lip_reading_amd import dp
    g = load_golden("flat_layout_sbl.npz")
    m = _sbl(6, 6)
    flat = dp.FlatModel(m)
    names = {id(p): n for n, p in m.named_parameters()}
    assert flat.segments == dp.FlatModel.SEGMENTS
    assert [names[id(p)] for p, _, _ in flat.slots] == [str(n) for n in g["names"]]
    assert [o for _, o, _ in flat.slots] == g["offsets"].tolist()
    assert [n for _, _, n in flat.slots] == g["sizes"].tolist()
    assert [p.numel() for p, _, _ in flat.slots] == g["numels"].tolist()
    assert list(flat.ranges) == [str(s) for s in g["segments"]] == list(dp.FlatModel.SEGMENTS)
    assert [list(v) for v in flat.ranges.values()] == g["seg_bounds"].tolist()
    assert flat.numel == 80898240 and len(flat.slots) == 475
    assert flat.ranges["encoder."] == (50537472, 69715456)


def test_classifier_flat_layout():
    from sbl_for_multilingual_lip_reading_amd import dp
    from sbl_for_multilingual_lip_reading_amd.transformer.classifier import ClassifierTransformer
    m = _classifier(3)
    flat = dp.FlatModel(m)
    assert flat.segments == ClassifierTransformer.FLAT_SEGMENTS
    assert list(flat.ranges) == ["fc_", "encoder_v.", "visual_frontend.resnet18.layer4.", "visual_frontend.resnet18.layer3.",
                                 "visual_frontend.resnet18.layer2.", "visual_frontend."]
    names = {id(p): n for n, p in m.named_parameters()}
    for seg, (a, b) in flat.ranges.items():
        inside = [names[id(p)] for p, off, _ in flat.slots if a <= off < b]
        assert inside and all(n.startswith(seg) for n in inside), seg
    assert [names[id(p)] for p, _, _ in flat.slots[:4]] == ["fc_1500.weight", "fc_1500.bias", "fc_2.weight", "fc_2.bias"]
    assert flat.numel == sum((p.numel() + 3) // 4 * 4 for p in m.parameters())
    assert flat.span("visual_frontend.") == (flat.ranges["visual_frontend.resnet18.layer4."][0], flat.numel)
    # what is left to exchange after backward: ResNet layer1 + the stem
    a, b = flat.ranges["visual_frontend."]
    assert b - a < 200000
    # q/k/v of encoder_v stay adjacent rows of one fused buffer
    mha = m.encoder_v.layer_stack[0].slf_attn
    assert mha.w_ks.weight.data_ptr() == mha.w_qs.weight.data_ptr() + mha.w_qs.weight.numel() * 4


def test_classifier_gradient_exchange_hooks():
    from sbl_for_multilingual_lip_reading_amd import dp
    m = _classifier(1)
    flat = dp.FlatModel(m)
    ex = dp.GradientExchange.__new__(dp.GradientExchange)
    ex.flat, ex.world, ex._hooks, ex._pending, ex.launches, ex.cuda = flat, 2, [], [], [], False
    ex._install()
    assert len(ex._hooks) == 5          # encoder_v out, frontend out, inputs of ResNet stages 4, 3, 2
    ex.close()


def test_stage1_to_stage2_checkpoint_hand_off(tmp_path):
    from sbl_for_multilingual_lip_reading_amd import checkpoint
    cls = _classifier(1, seed=1)
    checkpoint.save_checkpoint(tmp_path / "cls.pt", cls, epoch=5)
    # strict=False, no map: what SBL/train.py:92-103 does - the frontend loads by name, encoder_v.* / fc_* are dropped
    sbl = _sbl(1, 1, seed=2)
    enc_before = {k: v.clone() for k, v in sbl.encoder.state_dict().items()}
    meta = checkpoint.load_checkpoint(tmp_path / "cls.pt", sbl, strict=False)
    assert meta["epoch"] == 5
    for k, v in cls.visual_frontend.state_dict().items():
        assert torch.equal(sbl.visual_frontend.state_dict()[k], v), k
    for k, v in sbl.encoder.state_dict().items():
        assert torch.equal(v, enc_before[k]), k
    assert not torch.equal(sbl.encoder.linear_in.weight, cls.encoder_v.linear_in.weight)
    # with the prefix map the pre-trained encoder comes along (README stage 2)
    sbl2 = _sbl(1, 1, seed=3)
    dec_before = {k: v.clone() for k, v in sbl2.decoder.state_dict().items()}
    checkpoint.load_checkpoint(tmp_path / "cls.pt", sbl2, strict=False, prefix_map={"encoder_v.": "encoder."})
    for k, v in cls.visual_frontend.state_dict().items():
        assert torch.equal(sbl2.visual_frontend.state_dict()[k], v), k
    for k, v in cls.encoder_v.state_dict().items():
        assert torch.equal(sbl2.encoder.state_dict()[k], v), k
    for k, v in sbl2.decoder.state_dict().items():
        assert torch.equal(v, dec_before[k]), k
    # strict: the keys do not match
    with pytest.raises(KeyError):
        checkpoint.load_checkpoint(tmp_path / "cls.pt", _sbl(1, 1, seed=4))
    with pytest.raises(KeyError):
        checkpoint.load_checkpoint(tmp_path / "cls.pt", _sbl(1, 1, seed=4), prefix_map={"encoder_v.": "encoder."})
    # and the classifier's own round trip
    cls2 = _classifier(1, seed=9)
    checkpoint.load_checkpoint(tmp_path / "cls.pt", cls2)
    for (k, a), (_, b) in zip(cls.state_dict().items(), cls2.state_dict().items()):
        assert torch.equal(a, b), k


def test_cls_accuracy_from_stats():
    from sbl_for_multilingual_lip_reading_amd.transformer.classifier import cls_accuracy
    acc_w, acc_l = cls_accuracy(torch.tensor([10.0, 4.0, 3.0, 1.0, 5.0, 5.0]))
    assert acc_w == 0.75 and acc_l == 1.0
    assert np.isnan(cls_accuracy(torch.zeros(6))[0])
