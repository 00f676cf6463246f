"""uint8 frames straight into the stem (sbl_stem_conv_fwd_u8 / sbl_stem_wgrad_u8, ops.RawClips) against the path it
replaces: ops.preprocess_clips followed by the fp32-source entry points, in the same arithmetic mode.  The raw source stages
the same floats into the same contraction, so the convolution output has to be bit-identical; whatever is reduced with
atomics (BatchNorm statistics, the weight gradient) is held to the bounds the existing tests use for "same values, another
order".  Every figure is printed before it is asserted."""
import random

import numpy as np
import pytest
import torch

from sbl_for_multilingual_lip_reading_amd import detfill

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (N, Tin, Hin, Win, Tout, Hc, Wc): the production shape (44x44 maps: partial 8x16 tiles), the partial-tile shape of
# test_stem_weight_gradient_kernels_agree, and frames that are the crop
SHAPES = [(3, 29, 96, 96, 30, 88, 88), (2, 3, 48, 64, 3, 40, 56), (2, 6, 32, 32, 6, 32, 32)]


@pytest.fixture(scope="module", params=["f32", "bf16x6", "bf16x3", "bf16"])
def ops(request):
    """test_hip_parity.py's precision fixture over all four arithmetics of the tile engine: the raw source goes through the
    same sbl_set_matmul_precision dispatch as the fp32 source."""
    from sbl_for_multilingual_lip_reading_amd import _lib, ops as _ops
    _lib.load()
    assert torch.cuda.is_available()
    _ops.set_matmul_precision(request.param)
    yield _ops
    _ops.set_matmul_precision("f32")


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def raw_case(ops, seed, N, Tin, Hin, Win, Tout, Hc, Wc, zero_clip=True):
    """Random bytes, crops at random origins, mixed flips, src_frame rows with repeated frames and a -1 tail, and (zero_clip)
    a last clip whose row is all -1 - the inputs of test_device_input_pipeline_bit_exact."""
    rng = np.random.RandomState(seed)
    frames = rng.randint(0, 256, size=(N, Tin, Hin, Win)).astype(np.uint8)
    y1 = rng.randint(0, Hin - Hc + 1, size=N).astype(np.int32)
    x1 = rng.randint(0, Win - Wc + 1, size=N).astype(np.int32)
    flip = ((np.arange(N) + seed) % 2).astype(np.int32)              # both values in every batch of two or more
    src = np.full((N, Tout), -1, dtype=np.int32)
    for n in range(N - 1 if zero_clip else N):
        L = int(rng.randint(max(1, Tout // 2), min(Tin, Tout - 1) + 1))
        cur = list(range(L))
        for i in range(1, L):
            if rng.rand() < 0.25:
                cur[i] = cur[i - 1]                                   # a removed frame repeats its predecessor
        src[n, :L] = cur
    t = [torch.from_numpy(a).to(DEV) for a in (frames, y1, x1, flip, src)]
    return ops.RawClips(*t, crop=(Hc, Wc))


def stem_params(seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(64, 1, 5, 7, 7, generator=g) * 0.05).to(DEV)
    gamma = (0.5 + torch.rand(64, generator=g)).to(DEV)
    beta = (0.2 * torch.randn(64, generator=g)).to(DEV)
    return w, gamma, beta


def conv_ref(ops, x, w2):
    N, T, H, W = x.shape
    conv = torch.empty(N * T, H // 2, W // 2, 64, device=DEV)
    stats = torch.empty(128, device=DEV, dtype=torch.float64)
    ops.call("sbl_stem_conv_fwd", x.data_ptr(), w2.data_ptr(), conv.data_ptr(), stats.data_ptr(), N, T, H, W, ops._s())
    torch.cuda.synchronize()
    return conv, stats


@pytest.mark.parametrize("shape", SHAPES)
def test_conv_out_is_bit_identical_to_the_two_kernel_path(ops, shape):
    raw = raw_case(ops, 7, *shape)
    N, T, H, W = raw.shape
    w2 = stem_params(3)[0].view(64, 245).contiguous()
    x = raw.materialize()
    assert float(x[-1].abs().max()) == 0.0 and float(x[0].abs().max()) > 0.0      # the all -1 clip, and a live one
    ref, st_a = conv_ref(ops, x, w2)
    _, st_b = conv_ref(ops, x, w2)
    conv = torch.full_like(ref, float("nan"))
    stats = torch.empty(128, device=DEV, dtype=torch.float64)
    ops.call("sbl_stem_conv_fwd_u8", *[t.data_ptr() for t in raw.tensors()], w2.data_ptr(), conv.data_ptr(), stats.data_ptr(),
             *raw.src_dims(), ops._s())
    torch.cuda.synchronize()
    a, b = conv.cpu().numpy(), ref.cpu().numpy()
    print("conv_out %s %s: %d of %d elements differ" % (ops.get_matmul_precision(), shape, int((a.view(np.uint32) != b.view(np.uint32)).sum()), a.size))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # the statistics: identical addends, order-dependent double atomics - what the reference path shows between two runs of
    # itself, with a floor of one ulp of the sum
    sa, sb, su = st_a.cpu().numpy(), st_b.cpu().numpy(), stats.cpu().numpy()
    tol = np.maximum(np.abs(sa - sb), np.spacing(np.abs(sa)))                # per sum
    print("stats: reference spread %.3g, raw - reference %.3g (largest sum %.6g)" % (np.abs(sa - sb).max(), np.abs(su - sa).max(), np.abs(sa).max()))
    assert np.all(np.abs(su - sa) <= tol)


def _stem(ops, x, params, rm, rv, training, nbt=None):
    w, gamma, beta = params
    return ops.StemFn.apply(x, w, gamma, beta, rm, rv, training, 0.1, 1e-5, nbt)


@pytest.mark.parametrize("shape", SHAPES)
def test_eval_mode_stem_is_bit_identical(ops, shape):
    raw = raw_case(ops, 11, *shape)
    params = stem_params(5)
    g = torch.Generator().manual_seed(9)
    rm, rv = (0.3 * torch.randn(64, generator=g)).to(DEV), (0.5 + torch.rand(64, generator=g)).to(DEV)
    with torch.no_grad():
        ref = _stem(ops, raw.materialize(), params, rm, rv, False)
        got = _stem(ops, raw, params, rm, rv, False)
    torch.cuda.synchronize()
    assert got.shape == ref.shape and torch.equal(got, ref)


@pytest.mark.parametrize("shape", SHAPES)
def test_training_mode_stem_forward_and_backward(ops, shape):
    raw = raw_case(ops, 13, *shape)
    x = raw.materialize()
    out = []
    for src in (x, raw):
        w, gamma, beta = (p.clone().requires_grad_(True) for p in stem_params(5))
        rm, rv = torch.zeros(64, device=DEV), torch.ones(64, device=DEV)
        nbt = torch.zeros((), dtype=torch.long, device=DEV)
        pooled = _stem(ops, src, (w, gamma, beta), rm, rv, True, nbt)
        dy = torch.from_numpy(detfill.uniform("stem_u8.dy", tuple(pooled.shape))).to(DEV)
        pooled.backward(dy)
        torch.cuda.synchronize()
        out.append((pooled.detach(), w.grad, gamma.grad, beta.grad, rm, rv, int(nbt)))
    ref, got = out
    figs = (float((got[0] - ref[0]).abs().max()), relerr(got[1], ref[1]), relerr(got[2], ref[2]), relerr(got[3], ref[3]),
            float((got[4] - ref[4]).abs().max()), float((got[5] - ref[5]).abs().max()))
    print("%s %s: pooled %.3g  dw %.3g  dgamma %.3g  dbeta %.3g  running mean %.3g  var %.3g" % ((ops.get_matmul_precision(), shape) + figs))
    assert figs[0] < 2e-5                                   # test_stem_fwd_bwd's forward bound: only the statistics' atomics differ
    assert figs[1] < 2e-5                                   # test_stem_weight_gradient_kernels_agree: same values, another atomic order
    assert figs[2] < 2e-5 and figs[3] < 2e-5
    assert figs[4] < 1e-6 and figs[5] < 1e-6
    assert got[6] == ref[6] == 1


def test_backward_keeps_the_bytes_not_a_float_clip(ops):
    shape = SHAPES[0]
    raw = raw_case(ops, 17, *shape)
    w, gamma, beta = (p.clone().requires_grad_(True) for p in stem_params(5))
    pooled = _stem(ops, raw, (w, gamma, beta), torch.zeros(64, device=DEV), torch.ones(64, device=DEV), True)
    saved = pooled.grad_fn.saved_tensors
    clip = raw.shape.numel()
    assert not [tuple(t.shape) for t in saved if t.dtype == torch.float32 and t.numel() == clip]
    assert any(t.data_ptr() == raw.frames_u8.data_ptr() and t.dtype == torch.uint8 for t in saved)
    # ... and the fp32 source still keeps its clip (the check above can fail)
    x = raw.materialize()
    pooled = _stem(ops, x, (w, gamma, beta), torch.zeros(64, device=DEV), torch.ones(64, device=DEV), True)
    assert [t for t in pooled.grad_fn.saved_tensors if t.dtype == torch.float32 and t.numel() == clip]


# --------------------------------------------------------------------------- whole models
def _fill(m):
    sd = m.state_dict()
    m.load_state_dict({k: (v if k.endswith("pe") else torch.from_numpy(detfill.fill_value(k, tuple(v.shape)).copy()))
                       for k, v in sd.items()})
    for mm in m.modules():
        if isinstance(mm, torch.nn.Dropout):
            mm.p = 0.0
    m.visual_frontend.frontend_dropout_p = 0.0          # FRONTEND_DROPOUT_P off
    return m.to(DEV)


def _sbl_model():
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    from sbl_for_multilingual_lip_reading_amd.transformer.transformer import Transformer
    m = _fill(Transformer(Encoder(512, 1, 8, 64, 64, 512, 2048), Decoder(0, 1, 58, 512, 1, 8, 64, 64, 512, 2048), None))
    m.decoder.coins_host = [False] * 16
    return m


def _cls_model():
    from sbl_for_multilingual_lip_reading_amd.transformer.classifier import ClassifierTransformer
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    return _fill(ClassifierTransformer(Encoder(512, 1, 8, 64, 64, 512, 2048), None))


def _compare_steps(ops, build, step, raw):
    """forward + loss + backward with the fp32 clip and with the RawClips, each on a fresh model: loss and flat gradients."""
    from sbl_for_multilingual_lip_reading_amd import dp
    runs = []
    for src in (raw.materialize(), raw):
        m = build().train()
        flat = dp.FlatModel(m)
        flat.zero_grad()
        random.seed(3)
        loss = step(m, src)
        loss.backward()
        ops.join_side_streams()
        torch.cuda.synchronize()
        runs.append((flat.flat_grad.clone(), dict(flat.ranges), float(loss.item())))
    print("%s: loss %.7f (fp32 clip) %.7f (raw)" % (ops.get_matmul_precision(), runs[0][2], runs[1][2]))
    assert abs(runs[0][2] - runs[1][2]) < 2e-5           # two fresh forward passes: BN statistics are summed with atomics
    for seg, (a, b) in runs[0][1].items():
        ref, got = runs[0][0][a:b].double(), runs[1][0][a:b].double()
        rel = float((got - ref).norm() / ref.norm())
        print("   %-40s %.3g" % (seg, rel))
        assert rel < (3e-2 if seg.startswith("visual_frontend.") else 1e-4), (seg, rel)


def test_transformer_training_step(ops):
    """1 + 1 layers, B = 2, T = 4, 24x24 crops of 32x32 frames; the bounds of
    test_backward_cut_at_frontend_features_equals_single_backward (two fresh forward passes)."""
    from sbl_for_multilingual_lip_reading_amd.transformer.loss import cal_performance_device
    raw = raw_case(ops, 23, 2, 4, 32, 32, 4, 24, 24)
    _, l2r, r2l = detfill.synthetic_batch(2, 4, 24, 24, 61)
    ld, rd = torch.from_numpy(l2r).to(DEV), torch.from_numpy(r2l).to(DEV)

    def step(m, src):
        pl, gl, pr, gr = m(src, ld, rd)
        return 0.5 * (cal_performance_device(pl, gl, 0.1)[0] + cal_performance_device(pr, gr, 0.1)[0])
    _compare_steps(ops, _sbl_model, step, raw)


def test_classifier_training_step(ops):
    """The CLS loader's all-zero last frame as a src_frame column of -1."""
    from sbl_for_multilingual_lip_reading_amd.transformer.classifier import cal_cls_loss
    raw = raw_case(ops, 29, 2, 4, 32, 32, 5, 24, 24)
    raw.src_frame[:, -1] = -1
    g = torch.Generator().manual_seed(29)
    t1, t2 = torch.randint(0, 1500, (2,), generator=g).to(DEV), torch.randint(0, 2, (2,), generator=g).to(DEV)

    def step(m, src):
        v, lang = m(src)
        assert tuple(v.shape) == (2, 1500) and tuple(lang.shape) == (2, 2)
        return cal_cls_loss(v, lang, t1, t2)[0]
    _compare_steps(ops, _cls_model, step, raw)


def test_recognize_under_graph_replay_with_static_raw_inputs(ops):
    """recognize(RawClips) captured once in eval() under no_grad; the uint8 / index buffers are the graph's static inputs:
    overwritten with a second batch and replayed, the tokens are the eager decode of that batch."""
    m = _sbl_model().eval()
    dims = (2, 4, 32, 32, 4, 24, 24)
    static = raw_case(ops, 31, *dims)
    second = raw_case(ops, 37, *dims, zero_clip=False)
    s = torch.cuda.Stream()
    with torch.no_grad():
        want = m.recognize(second)
        first = m.recognize(static)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m.recognize(static)                              # warm-up on the capture stream
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ys = m.recognize(static)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ys, first))
    for dst, src in zip(static.tensors(), second.tensors()):
        if dst.data_ptr() != src.data_ptr():                 # (the normalisation table is shared)
            dst.copy_(src)
    torch.cuda.set_sync_debug_mode("error")
    try:
        graph.replay()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ys, want))
    print("the two batches decode %s" % ("alike" if all(torch.equal(a, b) for a, b in zip(first, want)) else "differently"))


def test_validate_and_the_frontend_itself_take_rawclips(ops):
    """The two listed entry points no other test reaches: Transformer.validate scores the decode of a RawClips exactly as that
    of the materialised clips, and Lipreading.forward (the frontend called directly) returns the same features, bit for bit in
    eval mode (running statistics: nothing is reduced with atomics on the way)."""
    from sbl_for_multilingual_lip_reading_amd.transformer.metrics import ErrorRateMeter
    m = _sbl_model().eval()
    raw = raw_case(ops, 41, 2, 4, 32, 32, 4, 24, 24, zero_clip=False)
    _, l2r, r2l = detfill.synthetic_batch(2, 4, 24, 24, 43)
    ld, rd = torch.from_numpy(l2r).to(DEV), torch.from_numpy(r2l).to(DEV)
    with torch.no_grad():
        x = raw.materialize()
        f_ref, f_raw = m.visual_frontend(x.unsqueeze(1)), m.visual_frontend(raw)
        assert tuple(f_raw.shape) == (2, 4, 512) and torch.equal(f_raw, f_ref)
        meters = [ErrorRateMeter(device=DEV), ErrorRateMeter(device=DEV)]
        ys_ref = m.validate(x, ld, rd, meters[0])
        ys_raw = m.validate(raw, ld, rd, meters[1])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ys_raw, ys_ref))
    assert meters[0].result() == meters[1].result() and meters[1].result()["n"] == 2
