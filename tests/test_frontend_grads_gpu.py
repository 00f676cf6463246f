"""The composed frontend backward - stem, eight BlockFn tape nodes, average pool - against float64 UNDER THE GPU'S OWN
ReLU masks and pool arg-max codes (tests/frontend_reference.py).  A rewrite of the trunk backward is judged by this
module: given the decisions the gradient is a smooth function, so residual gradients, the compact 1x1/s2 addend, the
BatchNorm sums riding on the next block's conv1 input gradient, BlockHandoff, persistent gradient buffers and side-stream
weight gradients are held to fp32 rounding instead of the 2e-2 that one differing decision costs the end-to-end tests.

Bounds are not read off the GPU: every check evaluates the same reference in fp32 on the CPU under the same masks;
E_fwd / E_grad are its worst max|d| / max|ref| against float64 over the nine outputs / 60 parameter gradients (3e-6 to
4e-6 / 5e-6 to 8e-6), and the GPU is allowed tol = 8 * E (summation order, MFMA chains up to K = 4608, float atomics in
the stem, the bf16x6 products), never more than 2e-4.  The decisions themselves are judged by invalid_flips: they may
differ from float64's own only where float64's pre-activation is within tol_fwd of the switching point, and in at most 8
of ~5e5 places (the fp32 CPU evaluation differs in 0 to 1, tests/test_frontend_reference_cpu.py).
Measured GPU / E ratios are in DESIGN.md section 2."""
import functools
import random

import numpy as np
import pytest
import torch

import frontend_reference as R
import stem_reference as SR
from conftest import maxdiff
from sbl_for_multilingual_lip_reading_amd import detfill
from test_hip_parity import DEV, _load_det, build_model, ops      # noqa: F401  (ops: runs a test under f32 and bf16x6)

pytestmark = pytest.mark.gpu

CASES, inputs = R.CASES, R.inputs
GPU_CASES = CASES[:4]
ODD = CASES[1]
FACTOR, CAP, MAX_DIFFERING = 8.0, 2e-4, 8


# --------------------------------------------------------------------------- the GPU's decisions
class Probe:
    """Records what every ops.conv_bn_fwd call of a forward pass returns (BlockFn.forward looks the function up at call
    time) and counts the launches of the backward pass.  No library change, no extra launch."""

    def __init__(self, ops_mod):
        self.ops, self.calls, self.launches = ops_mod, [], []

    def __enter__(self):
        inner = self._fwd = self.ops.conv_bn_fwd

        def conv_bn_fwd(x, c, res, relu, training, need_dg):
            r = inner(x, c, res, relu, training, need_dg)
            self.calls.append((x, r[1], relu))
            return r
        self.ops.conv_bn_fwd = conv_bn_fwd
        return self

    def __exit__(self, *exc):
        self.ops.conv_bn_fwd = self._fwd

    def backward(self, out, dy):
        inner = self.ops.call
        self.ops.call = lambda name, *a: (self.launches.append(name), inner(name, *a))[1]
        try:
            out.backward(dy)
        finally:
            self.ops.call = inner
        self.ops.join_side_streams()
        torch.cuda.synchronize()

    def decisions(self, argmax):
        """-> (masks for frontend_reference, the eight block outputs NCHW on the CPU, the pooled stem output).  argmax: the
        stem's codes (NHWC)."""
        assert len(self.calls) == 8 * 2 + 3 and [c[2] for c in self.calls].count(False) == 3
        ys = [R.nchw(y).cpu() for _, y, relu in self.calls if relu]
        pooled = R.nchw(self.calls[0][0]).cpu()
        return {"relu": [pooled > 0] + [y > 0 for y in ys], "pool": R.nchw(argmax).cpu()}, ys[1::2], pooled


def stem_node(t):
    """The StemFn tape node upstream of tensor t (its saved tensors hold the arg-max codes)."""
    seen, todo = set(), [t.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if type(fn).__name__ == "StemFnBackward":
            return fn
        todo.extend(f for f, _ in fn.next_functions)
    raise AssertionError("no StemFn node upstream")


def new_frontend():
    from sbl_for_multilingual_lip_reading_amd.transformer.video_frontend import Lipreading
    fe = _load_det(Lipreading(), R.PREFIX)
    fe.frontend_dropout_p = 0.0
    return fe.to(DEV).train()


@functools.lru_cache(None)
def _det_sd():
    """The deterministic fill of a fresh frontend as a CPU state dict (every new_frontend() starts from it)."""
    from sbl_for_multilingual_lip_reading_amd.transformer.video_frontend import Lipreading
    return R.state_dict_of(_load_det(Lipreading(), R.PREFIX), torch.float64)


@functools.lru_cache(None)
def own64(case):
    """The float64 evaluation of a committed case under its own decisions; shared by every test, never modified."""
    x, dy = inputs(case[0], case[1])
    return R.evaluate(_det_sd(), x, dy)


# --------------------------------------------------------------------------- the checks
class Judged:
    """One forward/backward pass judged against float64 under its own decisions."""

    def __init__(self, tag, base_sd, x, dy, masks, own=None, drop=None):
        self.tag = tag
        self.own = own if own is not None else R.evaluate(base_sd, x, dy, drop=drop)
        self.s64 = R.evaluate(base_sd, x, dy, masks=masks, drop=drop)
        self.s32 = R.evaluate(base_sd, x, dy, masks=masks, dtype=torch.float32, drop=drop)
        self.e_fwd = max(R.rel(a, b) for a, b in zip(self.s32.blocks + [self.s32.out], self.s64.blocks + [self.s64.out]))
        self.e_grad = R.worst(self.s32.grads, self.s64.grads)[0]
        self.tol_fwd, self.tol_grad = FACTOR * self.e_fwd, FACTOR * self.e_grad
        assert self.tol_fwd <= CAP and self.tol_grad <= CAP, (self.tol_fwd, self.tol_grad)
        self.masks = masks

    def decisions(self):
        n = R.n_differing(self.masks, self.own)
        bad = R.invalid_flips(self.masks, self.own, self.tol_fwd)
        print("%s: %d decisions differ from float64's own, %d of them outside tol_fwd" % (self.tag, n, len(bad)))
        assert bad == [], bad[:5]
        assert n <= MAX_DIFFERING, n

    def forward(self, blocks, out):
        e = [R.rel(b, r) for b, r in zip(blocks + [out.reshape(self.s64.out.shape)], self.s64.blocks + [self.s64.out])]
        print("%s: forward %.2e = %.2f E_fwd (E_fwd %.2e)" % (self.tag, max(e), max(e) / self.e_fwd, self.e_fwd))
        assert len(e) == 9 and max(e) <= self.tol_fwd, (e, self.tol_fwd)


def check_grads(tag, grads, ref64, ref32, names=None):
    """Every gradient within 8 * E_grad * max|ref| of float64, E_grad being the fp32 CPU evaluation's worst."""
    names = list(ref64) if names is None else names
    e_grad = R.worst(ref32, ref64)[0]
    tol = FACTOR * e_grad
    assert tol <= CAP, tol
    e = {k: R.rel(grads[k], ref64[k]) for k in names}
    k = max(e, key=e.get)
    print("%s: gradients %.2e = %.2f E_grad (E_grad %.2e, %s)" % (tag, e[k], e[k] / e_grad, e_grad, k[len(R.PREFIX):]))
    assert all(v <= tol for v in e.values()), ({n: v for n, v in e.items() if v > tol}, tol)


def check_stats(module, ref_sd, prefix=R.PREFIX):
    for k, v in module.state_dict().items():
        if "running_" in k:
            assert maxdiff(v, ref_sd[prefix + k]) < 1e-5, k
        elif "num_batches" in k:
            assert int(v) == int(ref_sd[prefix + k]), k


def grads_of(module, prefix=R.PREFIX):
    return {prefix + k: p.grad.detach().cpu().clone() for k, p in module.named_parameters() if p.grad is not None}


def run(ops_mod, fe, x_dev, dy, call=None):
    """One probed forward/backward of a frontend module -> (probe, output on the CPU, the stem's arg-max codes - None when the
    stem is frozen and has no tape node)."""
    with Probe(ops_mod) as pr:
        out = (fe._frontend_forward if call is None else call)(x_dev)
    argmax = stem_node(out).saved_tensors[1].clone() if any(p.requires_grad for p in fe.frontend3D.parameters()) else None
    pr.backward(out, dy.to(DEV).view(out.shape))
    return pr, out.detach().cpu(), argmax


def judge(tag, ops_mod, fe, case, x_dev=None, call=None, drop_of=None, frozen=()):
    """Run a committed case through module `fe` and assert everything the module docstring promises."""
    x, dy = inputs(case[0], case[1])
    base = R.state_dict_of(fe, torch.float64)
    pr, out, argmax = run(ops_mod, fe, x.to(DEV) if x_dev is None else x_dev, dy, call)
    own = own64(case)
    # a frozen stem has no backward, so its codes reach no gradient: float64's own stand in for them
    masks, blocks, _ = pr.decisions(argmax if argmax is not None else R.nhwc(own.masks["pool"]))
    drop = None if drop_of is None else drop_of(out)
    j = Judged(tag, base, x, dy, masks, own if drop is None else None, drop)
    j.decisions()
    j.forward(blocks, out)
    names = [k for k in j.s64.grads if not k.startswith(frozen)] if frozen else None
    got = grads_of(fe)
    assert sorted(got) == sorted(names if names is not None else j.s64.grads)
    check_grads(tag, got, j.s64.grads, j.s32.grads, names)
    check_stats(fe, j.s64.sd)
    return pr, j


def _id(case):
    return "x".join(map(str, case[0]))


# --------------------------------------------------------------------------- the cases, plain per-tensor autograd
@pytest.mark.parametrize("case", GPU_CASES, ids=_id)
def test_frontend_gradients_under_shared_masks(ops, case):
    """(2,6,32,32): 12 images, final map 1x1; (2,3,24,40): odd maps 3x5, 2x3, 1x2, the compact shortcut gradient's
    (H+1)//2 edge; (3,5,48,32); (4,8,64,64): 32 images, final map 2x2."""
    pr, _ = judge("plain %s %s" % (_id(case), ops.get_matmul_precision()), ops, new_frontend(), case)
    n = pr.launches
    # the last block's bn2 is the only BatchNorm with a reduction pass of its own; every shortcut gradient goes compact
    assert n.count("sbl_bn_bwd_reduce") == 1 and n.count("sbl_conv1x1s2_dgrad_compact") == 3 and n.count("sbl_conv2d_dgrad") == 0


# --------------------------------------------------------------------------- host paths
def test_flat_model_and_accumulation_over_two_passes(ops):
    """dp.FlatModel: persistent gradient buffers, side-stream weight gradients, the pooled zero fill.  Then a second pass
    with another dy and no zero_grad: the flat gradient is ref(dy1, masks1) + ref(dy2, masks2)."""
    from sbl_for_multilingual_lip_reading_amd import dp
    fe = new_frontend()
    flat = dp.FlatModel(fe)
    flat.zero_grad()
    tag = "flat %s" % ops.get_matmul_precision()
    _, j1 = judge(tag, ops, fe, ODD)
    assert all(p.grad.data_ptr() == p._sbl_grad.data_ptr() for p in fe.parameters())
    x, dy1 = inputs(ODD[0], ODD[1])
    dy2 = torch.from_numpy(np.ascontiguousarray(dy1.numpy()[::-1, ::-1])) * 0.5 + 0.25
    base = R.state_dict_of(fe, torch.float64)
    pr, out, argmax = run(ops, fe, x.to(DEV), dy2)
    masks, blocks, _ = pr.decisions(argmax)
    j2 = Judged(tag + " pass 2", base, x, dy2, masks)
    j2.decisions()
    j2.forward(blocks, out)
    ref64 = {k: j1.s64.grads[k] + j2.s64.grads[k] for k in j1.s64.grads}
    ref32 = {k: j1.s32.grads[k] + j2.s32.grads[k] for k in j1.s32.grads}
    check_grads(tag + " sum of two passes", grads_of(fe), ref64, ref32)
    check_stats(fe, j2.s64.sd)
    assert int(fe.frontend3D[1].num_batches_tracked) == 2


def test_severed_handoff_takes_the_reduce_fallback(ops):
    """Every BasicBlock's output cloned by a forward hook: no block finds a hand-off, so every bn2 (8) and shortcut
    BatchNorm (3) takes sbl_bn_bwd_reduce - the counts test_basic_block_chain_fwd_bwd asserts on its 3-block chain (4
    there), under the tight bound."""
    from sbl_for_multilingual_lip_reading_amd.transformer.video_frontend import BasicBlock
    fe = new_frontend()
    blocks = [m for m in fe.modules() if isinstance(m, BasicBlock)]
    assert len(blocks) == 8
    for b in blocks:
        b.register_forward_hook(lambda mod, i, o: o.clone())
    pr, _ = judge("severed %s" % ops.get_matmul_precision(), ops, fe, ODD)
    assert pr.launches.count("sbl_bn_bwd_reduce") == 11 and pr.launches.count("sbl_conv2d_dgrad") == 0
    assert pr.launches.count("sbl_conv1x1s2_dgrad_compact") == 3


def test_frozen_stem_first_block_without_input_gradient(ops):
    fe = new_frontend()
    for p in fe.frontend3D.parameters():
        p.requires_grad_(False)
    pr, _ = judge("frozen stem %s" % ops.get_matmul_precision(), ops, fe, ODD, frozen=(R.PREFIX + "frontend3D",))
    assert all(p.grad is None for p in fe.frontend3D.parameters())
    assert not any(n.startswith("sbl_stem_bwd") or n.startswith("sbl_stem_wgrad") for n in pr.launches)
    # layer1.0 computes no input gradient: 15 convolution input gradients instead of 16 (+ 3 compact ones)
    assert sum(n.startswith("sbl_conv2d_dgrad") for n in pr.launches) == 15


def test_raw_clips_source(ops):
    """uint8 frames through ops.RawClips (crop, flip, frame map with a zero frame) against the clip
    stem_reference.materialize builds from the same arguments."""
    (N, T, H, W), _, _ = ODD
    rng = np.random.RandomState(5)
    frames = rng.randint(0, 256, size=(N, T + 2, H + 7, W + 9)).astype(np.uint8)
    y1, x1, flip = np.array([3, 7], np.int32), np.array([9, 0], np.int32), np.array([1, 0], np.int32)
    src = np.array([[0, 2, 4], [3, -1, 1]], np.int32)
    mean, std = 0.413621, 0.1700239
    lut = ((np.arange(256, dtype=np.float64) / 255. - mean) / std).astype(np.float32)
    x = torch.from_numpy(SR.materialize(frames, lut, y1, x1, flip, src, T, H, W))
    raw = ops.RawClips(*(torch.from_numpy(a).to(DEV) for a in (frames, y1, x1, flip, src)), crop=(H, W), mean=mean, std=std)
    dy = inputs(ODD[0], ODD[1])[1]
    fe = new_frontend()
    base = R.state_dict_of(fe, torch.float64)
    pr, out, argmax = run(ops, fe, raw, dy)
    assert "sbl_stem_wgrad_u8" in pr.launches
    masks, blocks, _ = pr.decisions(argmax)
    tag = "raw clips %s" % ops.get_matmul_precision()
    j = Judged(tag, base, x, dy, masks)
    j.decisions()
    j.forward(blocks, out)
    check_grads(tag, grads_of(fe), j.s64.grads, j.s32.grads)
    check_stats(fe, j.s64.sd)


def test_lipreading_forward_with_dropout(ops):
    """Lipreading.forward with the reference's always-on dropout, p = 0.5.  The keep mask is (out != 0): a feature that is
    0 before the dropout has every ReLU below it closed, so either value of its mask bit gives the same gradients.  The
    reference multiplies by 2 * mask; on the GPU the kept values are exactly twice the trunk's output."""
    fe = new_frontend()
    fe.frontend_dropout_p = 0.5
    pre = {}
    fe.resnet18.register_forward_hook(lambda mod, i, o: pre.__setitem__("y", o.detach().cpu()))
    keep = {}

    def drop_of(out):
        keep["m"] = out.reshape(-1, 512) != 0
        return 2.0 * keep["m"].double()
    judge("dropout %s" % ops.get_matmul_precision(), ops, fe, ODD, x_dev=inputs(ODD[0], ODD[1])[0].unsqueeze(1).to(DEV),
          call=fe, drop_of=drop_of)
    live = pre["y"] != 0
    frac = float((keep["m"] & live).sum()) / float(live.sum())
    assert 0.4 < frac < 0.6, frac


# --------------------------------------------------------------------------- the frontend half of a whole train step
def test_train_step_frontend_gradients(ops):
    """Transformer forward + loss + one backward (B=3, T=5, 40x24, 1+1 layers, the shape of
    test_e2e_matches_oracle_other_seed): d(loss)/d(features), captured by a tensor hook on the frontend's output during
    that backward, fed to the shared-mask reference.  The tight frontend half that check_transformer_grads leaves out; no
    ReLU decision of the transformer enters."""
    from sbl_for_multilingual_lip_reading_amd.transformer.loss import cal_performance_device
    B, T, H, W = 3, 5, 40, 24
    x, l2r, r2l = detfill.synthetic_batch(B, T, H, W, 21)
    m = build_model(1, 1).train()
    fe = m.visual_frontend
    base = R.state_dict_of(fe, torch.float64)
    seen = {}

    def hook(mod, i, o):
        seen["argmax"] = stem_node(o).saved_tensors[1].clone()
        seen["out"] = o.detach().cpu()
        o.register_hook(lambda g: seen.__setitem__("dy", g.detach().cpu().clone()))
    h = fe.register_forward_hook(hook)
    random.seed(5)
    with Probe(ops) as pr:
        pl, gl, pr_, gr = m(torch.from_numpy(x).to(DEV), torch.from_numpy(l2r).to(DEV), torch.from_numpy(r2l).to(DEV))
    h.remove()
    loss = 0.5 * (cal_performance_device(pl, gl, 0.1)[0] + cal_performance_device(pr_, gr, 0.1)[0])
    pr.backward(loss, None)
    masks, blocks, _ = pr.decisions(seen["argmax"])
    xc, dy = torch.from_numpy(x), seen["dy"].reshape(B * T, 512)
    tag = "train step %s" % ops.get_matmul_precision()
    j = Judged(tag, base, xc, dy, masks)
    j.decisions()
    j.forward(blocks, seen["out"])
    got = {k: p.grad.detach().cpu() for k, p in m.named_parameters() if k.startswith(R.PREFIX)}
    assert len(got) == 60
    check_grads(tag, got, j.s64.grads, j.s32.grads)
    check_stats(fe, j.s64.sd)
