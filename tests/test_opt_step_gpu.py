"""The device-side optimizer step on the GPU: sbl_grad_sumsq, sbl_opt_finalize and sbl_adam_step_dev against float64 at
the edges of their launch geometry, the skip rule on planted inf / NaN, the Noam schedule on the device, bit-exact replay
of the captured optimizer, one hipGraph for the whole training step, and the checkpoint round trip.

The oracle of the finalize rule is tests/test_opt_step_cpu.py::finalize_ref (checked there against torch); the helpers
u, dev, f64, check, exact, U, EW_CAP are those of tests/test_norm_elementwise_gpu.py.  A launch over n elements uses
min(2048, ceil(ceil(n / 4) / 256)) blocks, so one trip of the capped grid covers 2048 * 256 float4 = EW_CAP elements."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import maxdiff
from sbl_for_multilingual_lip_reading_amd import detfill
from test_opt_step_cpu import (CLIP_COEF, GRAD_NORM, INV_SQRT_BC2, LR, SKIP, SKIPPED, STEP, STEP_SIZE, f32, finalize_ref)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
EW_CAP = 8192 * 256          # = 2048 blocks * 256 threads * 4 elements: one trip of the capped grid of these kernels
B1, B2, EPS = 0.9, 0.98, 1e-9


@pytest.fixture(scope="module", autouse=True)
def ops():
    from sbl_for_multilingual_lip_reading_amd import _lib, ops as _ops
    _lib.load()
    assert torch.cuda.is_available()
    assert _ops.OPT_MAX_BLOCKS * 256 * 4 == EW_CAP
    prev = _ops.get_matmul_precision()
    _ops.set_matmul_precision("f32")
    yield _ops
    _ops.set_matmul_precision(prev)


# --------------------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=None)
def _u_cached(name, shape):
    return detfill.uniform(name, shape)


def u(name, shape):
    """detfill uniform in [-1, 1), float32; computed once per (name, shape) and never written to."""
    return _u_cached(name, tuple(int(s) for s in shape))


def dev(a, dtype=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.copy()).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def f64(a):
    return np.asarray(a, dtype=np.float64)


def check(what, got, ref, bound):
    """|got - ref| <= bound elementwise (bound == 0: exact).  Prints and returns the worst error / bound ratio."""
    got, ref = f64(host(got) if hasattr(got, "detach") else got), f64(ref)
    bound = np.broadcast_to(f64(bound), ref.shape)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), what + ": non-finite output"
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    worst = float(ratio.max()) if ratio.size else 0.0
    print("%-44s worst err/bound %.3f  (max err %.3e)" % (what, worst, float(err.max()) if err.size else 0.0))
    assert worst <= 1.0, "%s: err/bound %.3f at %s" % (what, worst, np.unravel_index(int(ratio.argmax()), ratio.shape))
    return worst


def exact(what, got, ref):
    got = host(got) if hasattr(got, "detach") else np.asarray(got)
    ref = host(ref) if hasattr(ref, "detach") else np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = int(np.count_nonzero(got != ref))
    assert bad == 0, "%s: %d of %d elements differ (max %.3e)" % (what, bad, ref.size, maxdiff(got, ref))


def same_bits(what, a, b):
    """Bit equality of two tensors, NaN payloads included."""
    it = torch.int64 if a.dtype == torch.float64 else torch.int32
    assert a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it)), what


def within_ulp(got, ref, k=2):
    return abs(got - ref) <= k * np.spacing(abs(ref))


def clamp64(x, c):
    """torch.clamp's rule in float64: NaN stays NaN."""
    return np.where(x < -c, -c, np.where(x > c, c, x)) if c > 0 else x


def new_state(t=0, lr=0.0):
    s = [0.0] * 8
    s[STEP], s[LR] = float(t), float(lr)
    return s


GUARD = 8


def reduce_ranges(ops, g, ranges, gscale, clip, max_norm=0.0):
    """sbl_grad_sumsq per range into a NaN-framed workspace, then sbl_opt_finalize; returns (partials, nparts, state)."""
    nparts = sum(ops.opt_blocks(b - a) for a, b in ranges)
    ws = torch.full((GUARD + nparts + GUARD,), float("nan"), device=DEV, dtype=torch.float64)
    off = GUARD
    for a, b in ranges:
        off += ops.grad_sumsq(g[a:b], ws, off, gscale, clip)
    assert off == GUARD + nparts
    st = dev(new_state(), np.float64)
    ops.opt_finalize(st, ws[GUARD:], nparts, max_norm)
    assert bool(torch.isnan(ws[:GUARD]).all()) and bool(torch.isnan(ws[GUARD + nparts:]).all()), "guard frame overwritten"
    assert bool(torch.isfinite(ws[GUARD:GUARD + nparts]).all())
    return ws[GUARD:GUARD + nparts].clone(), nparts, st


# --------------------------------------------------------------------------- 1. reduction
SUMSQ_SIZES = [1, 3, 255, 257, 4 * 256 + 1, EW_CAP + 2 * 4 + 3, 2 * EW_CAP + 3]


@pytest.mark.parametrize("n", SUMSQ_SIZES)
def test_grad_sumsq_against_float64(ops, n):
    """norm = sqrt(sum clamp(g * scale, +-c)^2) against the exactly rounded float64 sum (math.fsum of the squares, which are
    exact in double: 24-bit factors).  Both scales are powers of two, so g * scale is exact; every term is positive and
    every addition is a double addition, so whatever the order the sum is within n * 2^-53 relative of the exact one, and the
    square root adds one ulp.  Sizes: below one float4, the scalar tail alone (3), one block minus / plus a tail, two blocks
    (1025), and the capped grid plus two float4 plus 3 and two full trips plus 3 (grid-stride wrap, block cap and tail at
    once).  The clamp bound sits inside the data range.  Two runs give the same bits in every partial and in the norm, a
    two-range call (the second range not 16-byte aligned: the scalar-load variant) gives the float64 sum over both, and
    the NaN frame around the workspace stays intact.
    measured: worst err/bound below 0.0005 at every size (the norm is the exactly rounded one or its neighbour)."""
    g0 = u("opt.g", (n,))
    gd = dev(g0)
    for gscale in (1.0, 0.125):
        for clip in (0.0, 0.5 * gscale):
            x = clamp64(f64(g0) * gscale, clip)
            if clip > 0 and n >= 255:
                assert (np.abs(f64(g0) * gscale) > clip).any() and (np.abs(f64(g0) * gscale) < clip).any()
            ref = math.sqrt(math.fsum((x * x).tolist()))
            bound = ref * n * 2.0 ** -53 + np.spacing(ref)
            tag = "sumsq[n=%d gs=%g clip=%g] " % (n, gscale, clip)
            p1, np1, s1 = reduce_ranges(ops, gd, [(0, n)], gscale, clip)
            p2, _, s2 = reduce_ranges(ops, gd, [(0, n)], gscale, clip)
            assert np1 == ops.opt_blocks(n) == min(2048, -(-(-(-n // 4)) // 256))
            same_bits(tag + "partials of two runs", p1, p2)
            same_bits(tag + "state of two runs", s1, s2)
            s = host(s1)
            check(tag + "norm", s[GRAD_NORM:GRAD_NORM + 1], [ref], [bound])
            assert s[CLIP_COEF] == 1.0 and s[STEP] == 1.0 and s[SKIP] == 0.0 and s[SKIPPED] == 0.0
            if n >= 3:
                cut = n // 2 if (n // 2) % 4 else n // 2 + 1          # second range starts off a 16-byte boundary
                p3, np3, s3 = reduce_ranges(ops, gd, [(0, cut), (cut, n)], gscale, clip)
                assert np3 == ops.opt_blocks(cut) + ops.opt_blocks(n - cut)
                check(tag + "two ranges", host(s3)[GRAD_NORM:GRAD_NORM + 1], [ref], [bound])


# --------------------------------------------------------------------------- 2. Adam with clip
@pytest.mark.parametrize("n", [1, 257, EW_CAP + 333])
def test_adam_step_dev_against_float64(ops, n):
    """sbl_grad_sumsq + sbl_opt_finalize + sbl_adam_step_dev against float64 from the same fp32 p, g, m, v, at t = 1, 2 and
    10000 (t - 1 preset in the state), grad_scale 1 and 1/8, with max_norm above the norm (coef must be EXACTLY 1) and below.
    Bounds: test_adam_step's derivation (tests/test_norm_elementwise_gpu.py) with the roundings of g' counted anew.
      coef == 1 (and max_norm off): g' = g * scale * 1.0f has the one rounding it had there, so the constants are that test's:
        m 4 U, v 7 U, update 10.5 U.  This is also the "agrees with sbl_adam_step" case: same lr (a float) and step.
      coef < 1: g' = fl(fl(g * scale) * fl32(coef)): the clamp rounds nothing, the product is 1 more rounding, and the float
        cast of the coefficient (whose double differs from the reference's by ~n * 2^-53) 1 more: 3 instead of 1.
        m: 3 + (1 - b1, two products, one sum: 3) = 6 U;  v: 2 * 3 + (1 - b2, three products, one sum: 5) = 11 U;
        denominator: half of v's 11 U + 4; update: + 3 = 12.5 U; the rest as there.
    Then |g'|_2 <= max_norm: coef * norm <= max_norm in the state's own doubles (2 ulp), coef itself to n * 2^-53 + 2 ulp.
    A block of entries has g = m = v = 0: they come back bit-identical.
    measured: worst err/bound 0.998 (p: where the update is far below p's ulp the final rounding IS the bound), 0.48 (m),
    0.33 (v), below 0.0005 (norm, coef)."""
    lr = f32(1e-3)
    p0 = u("adam.p", (n,))
    g0 = u("adam.g", (n,)) * np.float32(0.01)
    m0 = u("adam.m", (n,)) * np.float32(0.01)
    v0 = (u("adam.v", (n,)) * np.float32(0.01)) ** 2
    if n > 40:
        g0, m0, v0 = g0.copy(), m0.copy(), v0.copy()
        g0[3:40] = m0[3:40] = v0[3:40] = 0
    gd = dev(g0)
    ws = torch.zeros(ops.opt_blocks(n), device=DEV, dtype=torch.float64)
    b1, b2 = f32(B1), f32(B2)
    for step in (1, 2, 10000):
        for gscale, clip in ((1.0, 0.0), (0.125, 2.0 ** -11)):          # the bound is a float: the kernel clamps to the same number
            x = clamp64(f64(g0) * gscale, clip)
            sumsq = float(np.sum(x * x))
            norm = math.sqrt(sumsq)
            for max_norm in (0.0, 2.0 * norm + 1.0, 0.5 * norm):
                pd, md, vd = dev(p0), dev(m0), dev(v0)
                st = dev(new_state(step - 1, lr), np.float64)
                nb = ops.grad_sumsq(gd, ws, 0, gscale, clip)
                ops.opt_finalize(st, ws, nb, max_norm, False, None, B1, B2)
                ops.adam_step_dev(pd, gd, md, vd, st, B1, B2, EPS, gscale, clip)
                s = host(st)
                ref = finalize_ref(new_state(step - 1, lr), sumsq, max_norm, False, None, (B1, B2))
                tag = "adam_dev[n=%d t=%d gs=%g max_norm=%.3g] " % (n, step, gscale, max_norm)
                ulp = n * 2.0 ** -53
                assert s[STEP] == step and s[SKIP] == 0.0 and s[LR] == lr
                assert within_ulp(s[STEP_SIZE], ref[STEP_SIZE]) and within_ulp(s[INV_SQRT_BC2], ref[INV_SQRT_BC2]), (tag, s, ref)
                check(tag + "norm", s[GRAD_NORM:GRAD_NORM + 1], [norm], [norm * ulp + 2 * np.spacing(norm)])
                clipped = 0.0 < max_norm < norm
                if not clipped:
                    assert s[CLIP_COEF] == 1.0, tag
                    km, kv, ku = 4, 7, 10.5
                else:
                    check(tag + "coef", s[CLIP_COEF:CLIP_COEF + 1], [ref[CLIP_COEF]], [ref[CLIP_COEF] * ulp + 2 * np.spacing(ref[CLIP_COEF])])
                    assert s[CLIP_COEF] < 1.0 and s[CLIP_COEF] * s[GRAD_NORM] <= max_norm + 2 * np.spacing(max_norm), tag
                    km, kv, ku = 6, 11, 12.5
                g = x * ref[CLIP_COEF]
                m = b1 * f64(m0) + (1 - b1) * g
                v = b2 * f64(v0) + (1 - b2) * g * g
                e_m = km * U * (np.abs(b1 * f64(m0)) + np.abs((1 - b1) * g))
                e_v = kv * U * (b2 * f64(v0) + (1 - b2) * g * g)
                den = np.sqrt(v) * ref[INV_SQRT_BC2] + EPS
                upd = ref[STEP_SIZE] * m / den
                p = f64(p0) - upd
                e_p = np.abs(upd) * ku * U + ref[STEP_SIZE] * e_m / den + U * (np.abs(f64(p0)) + np.abs(upd))
                e_p = np.where(upd == 0, 0.0, e_p)
                check(tag + "m", md, m, e_m)
                check(tag + "v", vd, v, e_v)
                check(tag + "p", pd, p, e_p)
                if n > 40:
                    exact(tag + "zero-gradient block", pd[3:40], p0[3:40])
                    exact(tag + "zero-gradient block m", md[3:40], m0[3:40])


# --------------------------------------------------------------------------- 3. Noam on the device
class _Groups:
    param_groups = []


@pytest.mark.parametrize("k,warmup", [(0.2, 4000), (0.5, 2)])
def test_noam_rate_and_bias_factors_on_the_device(ops, k, warmup):
    """The lr slot after sbl_opt_finalize at t = 1..5, warmup - 1, warmup, warmup + 1 == TransformerOptimizer._update_lr's
    host value to 2 fp64 ulp; lr / (1 - b1^t) (from the slot's own lr) and 1 / sqrt(1 - b2^t) == the host's double
    arithmetic (sbl_adam_step's: 1 - pow(beta, t)) to 2 ulp.
    measured: lr differs by 0.0 ulp at every t of both schedules."""
    from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import TransformerOptimizer
    b1, b2 = f32(B1), f32(B2)
    ws = torch.ones(1, device=DEV, dtype=torch.float64)
    for t in sorted({1, 2, 3, 4, 5, warmup - 1, warmup, warmup + 1} - {0}):
        st = dev(new_state(t - 1), np.float64)
        ops.opt_finalize(st, ws, 1, 0.0, False, (k, warmup), B1, B2)
        s = host(st)
        href = TransformerOptimizer(_Groups(), warmup_steps=warmup, k=k)
        href.step_num = t - 1
        href._update_lr()
        print("noam[k=%g warmup=%d t=%d] lr %.17g host %.17g (%+.1f ulp)" % (k, warmup, t, s[LR], href.lr, (s[LR] - href.lr) / np.spacing(href.lr)))
        assert s[STEP] == t and s[GRAD_NORM] == 1.0 and s[CLIP_COEF] == 1.0
        assert within_ulp(s[LR], href.lr), (t, s[LR], href.lr)
        ss, bc2 = s[LR] / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t)
        assert within_ulp(s[STEP_SIZE], ss), (t, s[STEP_SIZE], ss)
        assert within_ulp(s[INV_SQRT_BC2], bc2), (t, s[INV_SQRT_BC2], bc2)
        ref = finalize_ref(new_state(t - 1), 1.0, 0.0, False, (k, warmup), (B1, B2))
        assert ref[LR] == href.lr


# --------------------------------------------------------------------------- FusedAdam over a stub of dp.FlatModel
class StubFlat:
    """What FusedAdam touches of a dp.FlatModel: two flat device buffers and the trainable ranges."""

    def __init__(self, p0, ranges):
        self.model = torch.nn.Linear(1, 1)
        self.flat_param = dev(p0)
        self.flat_grad = torch.zeros_like(self.flat_param)
        self.numel = self.flat_param.numel()
        self.slots = [None] * len(ranges)
        self._ranges = list(ranges)

    def zero_grad(self):
        self.flat_grad.zero_()

    def trainable_ranges(self):
        return list(self._ranges)


N_STUB = 4 * 256 + 1          # = 1 (mod 4): the last element is the scalar tail's


def stub_grad(i):
    return u("opt.step%d" % i, (N_STUB,)) * np.float32(0.01)


def snapshot(opt):
    return [t.clone() for t in (opt.flat.flat_param, opt.exp_avg, opt.exp_avg_sq, opt.opt_state)]


# --------------------------------------------------------------------------- 4. skip
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("clip", [None, 1.0])
def test_nonfinite_gradient_is_skipped(ops, bad, clip):
    """Step 1 is normal; step 2 has +inf / NaN planted in the LAST element of a range of 1025 (the tail lane).  With
    skip_nonfinite the step leaves p, m, v bit-identical, steps_applied == 1, steps_skipped == 1, and step 3 (finite) runs
    with the bias corrections of t = 2.  With clip_value = 1.0 the planted inf is clamped to 1 and the step is APPLIED (the
    reference's clamp_ semantics); the planted NaN passes the clamp and is still SKIPPED."""
    from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import FusedAdam
    lr = 1e-3
    flat = StubFlat(u("opt.p", (N_STUB,)), [(0, N_STUB)])
    opt = FusedAdam(flat, lr=lr, betas=(B1, B2), eps=EPS, skip_nonfinite=True, clip_value=clip)
    flat.flat_grad.copy_(dev(stub_grad(1)))
    opt.step()
    assert opt.steps_applied == 1 and opt.steps_skipped == 0
    before = snapshot(opt)
    g2 = stub_grad(2).copy()
    g2[-1] = bad
    flat.flat_grad.copy_(dev(g2))
    opt.step()
    after = snapshot(opt)
    applied = clip is not None and math.isinf(bad)
    if not applied:
        for name, a, b in zip(("p", "m", "v"), before, after):
            same_bits("skipped step changed " + name, a, b)
        assert opt.steps_applied == 1 and opt.steps_skipped == 1
        assert not math.isfinite(opt.last_grad_norm)
        s0, s1 = host(before[3]), host(after[3])
        assert s1[SKIP] == 1.0 and np.array_equal(s1[LR:SKIP], s0[LR:SKIP])
    else:
        assert opt.steps_applied == 2 and opt.steps_skipped == 0 and math.isfinite(opt.last_grad_norm)
        assert all(bool(torch.isfinite(t).all()) for t in after[:3])
        m_last = f32(B1) * float(before[1][-1]) + (1 - f32(B1)) * 1.0          # g' = clamp(+inf) = 1
        assert abs(float(after[1][-1]) - m_last) <= 4 * U * abs(m_last)
        assert not torch.equal(before[0], after[0])
    flat.flat_grad.copy_(dev(stub_grad(3)))
    opt.step()
    t = 3 if applied else 2
    s = host(opt.opt_state)
    assert opt.steps_applied == t and opt.steps_skipped == (0 if applied else 1) and s[SKIP] == 0.0
    assert within_ulp(s[STEP_SIZE], f32(lr) / (1.0 - f32(B1) ** t)) and within_ulp(s[INV_SQRT_BC2], 1.0 / math.sqrt(1.0 - f32(B2) ** t))
    final = snapshot(opt)
    assert all(bool(torch.isfinite(x).all()) for x in final[:3])
    assert float(((final[0] - after[0]).abs() > 0).float().mean()) > 0.99          # Adam's first steps move an element by ~lr


# --------------------------------------------------------------------------- 5. capture, optimizer only
def test_captured_optimizer_replays_bit_exactly(ops):
    """{sumsq x 2, finalize, adam x 2} over a static gradient buffer of 1025 elements in two ranges, max_grad_norm below the
    norm, noam = (0.5, 2), skipping on: captured once and replayed three times with a new gradient copied in before each
    replay (the middle one with an inf) == three eager steps from the same start, bit for bit in p, m, v and the state:
    same kernels, same launch order, no atomics."""
    from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import FusedAdam
    ranges = [(0, 515), (515, N_STUB)]          # the second one off a 16-byte boundary: the scalar-load kernels
    grads = [stub_grad(1), stub_grad(2).copy(), stub_grad(3)]
    grads[1][700] = np.inf

    def make():
        flat = StubFlat(u("opt.p", (N_STUB,)), ranges)
        return FusedAdam(flat, betas=(B1, B2), eps=EPS, max_grad_norm=0.05, skip_nonfinite=True, noam=(0.5, 2))

    eager = make()
    for g in grads:
        eager.flat.flat_grad.copy_(dev(g))
        eager.step()
    assert eager.steps_applied == 2 and eager.steps_skipped == 1 and eager.last_clip_coef < 1.0
    opt = make()
    gd = [dev(g) for g in grads]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        opt.step()
    start = make()
    for name, a, b in zip(("p", "m", "v", "state"), snapshot(start), snapshot(opt)):
        same_bits("capture itself changed " + name, a, b)
    for g in gd:
        opt.flat.flat_grad.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(("p", "m", "v", "state"), snapshot(eager), snapshot(opt)):
        same_bits("replayed " + name, a, b)
    assert opt.steps_applied == 2 and opt.steps_skipped == 1


# --------------------------------------------------------------------------- models
def build_model(n_enc, n_dec):
    """The small deterministic SBL model of tests/test_hip_parity.py (build_model / _load_det), all dropout off."""
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    from sbl_for_multilingual_lip_reading_amd.transformer.transformer import Transformer
    m = Transformer(Encoder(512, n_enc, 8, 64, 64, 512, 2048), Decoder(0, 1, 58, 512, n_dec, 8, 64, 64, 512, 2048), None)
    sd = m.state_dict()
    m.load_state_dict({k: (v if k.endswith("pe") else torch.from_numpy(detfill.fill_value(k, tuple(v.shape), 0, None).copy()))
                       for k, v in sd.items()})
    for mm in m.modules():
        if isinstance(mm, torch.nn.Dropout):
            mm.p = 0.0
    m.visual_frontend.frontend_dropout_p = 0.0
    return m.to(DEV)


# --------------------------------------------------------------------------- 6. the whole step under one graph
@pytest.mark.parametrize("frozen_encoder", [False, True])
def test_whole_training_step_under_one_graph(ops, frozen_encoder):
    """zero_grad + forward + loss + backward + DeviceNoamOptimizer.step() captured once (after an eager warm-up on the capture
    stream, weights and optimizer state restored) and replayed three times, against three eager steps of
    TransformerOptimizer(FusedAdam(default)) from the same weights, by the comparison rule of
    test_fused_adam_training_steps_match_torch_adam (gradients are sums of float atomics: losses to 1e-2, transformer
    matrices to 1e-2 in relative L2).  The coins come from decoder.coins_dev (all teacher-forced) and max_grad_norm is far
    above the norm, so coef == 1.  With the encoder frozen its slice of the flat parameters and of both moments keeps its
    bits."""
    from sbl_for_multilingual_lip_reading_amd import dp
    from sbl_for_multilingual_lip_reading_amd.transformer.loss import cal_performance_device
    from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import DeviceNoamOptimizer, FusedAdam, TransformerOptimizer
    B, T, H, W, ne, nd = 2, 4, 24, 24, 1, 1
    x, l2r, r2l = detfill.synthetic_batch(B, T, H, W, 51)
    xd, ld, rd = torch.from_numpy(x).to(DEV), torch.from_numpy(l2r).to(DEV), torch.from_numpy(r2l).to(DEV)

    def make():
        m = build_model(ne, nd).train()
        m.decoder.coins_dev = torch.zeros(16, dtype=torch.int32, device=DEV)
        if frozen_encoder:
            m.encoder.requires_grad_(False)
        return m, dp.FlatModel(m)

    def train_step(m, opt, loss_out):
        opt.zero_grad()
        pl, gl, pr, gr = m(xd, ld, rd)
        loss = 0.5 * (cal_performance_device(pl, gl, 0.1)[0] + cal_performance_device(pr, gr, 0.1)[0])
        loss.backward()
        ops.join_side_streams()
        opt.step()
        loss_out.copy_(loss.detach())

    m1, flat1 = make()
    opt1 = TransformerOptimizer(FusedAdam(flat1, betas=(B1, B2), eps=EPS), warmup_steps=2, k=0.5)
    loss1, losses1 = torch.zeros((), device=DEV), []
    for _ in range(3):
        train_step(m1, opt1, loss1)
        losses1.append(loss1.item())

    m2, flat2 = make()
    opt2 = DeviceNoamOptimizer(FusedAdam(flat2, betas=(B1, B2), eps=EPS, max_grad_norm=1e6, noam=(0.5, 2)))
    loss2, losses2 = torch.zeros((), device=DEV), []
    start_p = flat2.flat_param.clone()
    start_buf = {k: v.clone() for k, v in m2.named_buffers()}
    start_state = opt2.optimizer.opt_state.clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        train_step(m2, opt2, loss2)
        with torch.no_grad():
            flat2.flat_param.copy_(start_p)
            for k, v in m2.named_buffers():
                v.copy_(start_buf[k])
            opt2.optimizer.exp_avg.zero_()
            opt2.optimizer.exp_avg_sq.zero_()
            opt2.optimizer.opt_state.copy_(start_state)
            ops.refresh_packed_weights()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        train_step(m2, opt2, loss2)
    same_bits("capture changed the weights", flat2.flat_param, start_p)
    for _ in range(3):
        graph.replay()
        losses2.append(loss2.item())
    assert opt2.step_num == 3 and opt2.optimizer.steps_skipped == 0 and opt2.optimizer.last_clip_coef == 1.0
    assert abs(opt1.lr - opt2.lr) <= 2 * np.spacing(opt1.lr)
    print("losses eager %s graph %s" % (losses1, losses2))
    assert max(abs(a - b) for a, b in zip(losses1, losses2)) < 1e-2 and losses2[2] != losses2[0]
    p1 = dict(m1.named_parameters())
    for n, p in m2.named_parameters():
        if (n.startswith("decoder") or n.startswith("encoder")) and p.dim() >= 2:
            num = float((p.detach() - p1[n].detach()).norm())
            assert num < 1e-2 * float(p1[n].detach().norm()) + 1e-6, (n, num)
    if frozen_encoder:
        a, b = flat2.ranges["encoder."]
        same_bits("frozen parameters", flat2.flat_param[a:b], start_p[a:b])
        assert float(opt2.optimizer.exp_avg[a:b].abs().max()) == 0.0 and float(opt2.optimizer.exp_avg_sq[a:b].abs().max()) == 0.0
        same_bits("frozen parameters, eager", flat1.flat_param[a:b], start_p[a:b])
    moved = (flat2.flat_param - start_p).abs()
    a, b = flat2.ranges["decoder."]
    assert float(moved[a:b].max()) > 1e-4


# --------------------------------------------------------------------------- 7. checkpoint
def test_device_mode_checkpoint_round_trip(ops, tmp_path):
    """Two device-mode steps, save_checkpoint, rebuild model + FlatModel + optimizer, load_checkpoint: the state buffer and
    both moments are bit-equal, and one more step from identical planted gradients gives a bit-equal flat_param."""
    from sbl_for_multilingual_lip_reading_amd import checkpoint, dp
    from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import DeviceNoamOptimizer, FusedAdam

    def make():
        m = build_model(1, 1).train()
        flat = dp.FlatModel(m)
        return m, flat, DeviceNoamOptimizer(FusedAdam(flat, betas=(B1, B2), eps=EPS, max_grad_norm=1.0, skip_nonfinite=True, noam=(0.5, 2)))

    m1, flat1, opt1 = make()
    gen = torch.Generator(device=DEV).manual_seed(5)
    grads = [torch.randn(flat1.numel, device=DEV, generator=gen) * 0.01 for _ in range(3)]
    for g in grads[:2]:
        flat1.flat_grad.copy_(g)
        opt1.step()
    assert opt1.step_num == 2 and opt1.optimizer.last_clip_coef < 1.0
    checkpoint.save_checkpoint(tmp_path / "ck.pt", m1, opt1, epoch=1)
    m2, flat2, opt2 = make()
    assert not torch.equal(flat1.flat_param, flat2.flat_param)
    meta = checkpoint.load_checkpoint(tmp_path / "ck.pt", m2, opt2)
    assert meta["epoch"] == 1 and meta["step_num"] == 2 and opt2.step_num == 2
    same_bits("state buffer", opt1.optimizer.opt_state, opt2.optimizer.opt_state)
    same_bits("exp_avg", opt1.optimizer.exp_avg, opt2.optimizer.exp_avg)
    same_bits("exp_avg_sq", opt1.optimizer.exp_avg_sq, opt2.optimizer.exp_avg_sq)
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    for flat, opt in ((flat1, opt1), (flat2, opt2)):
        flat.flat_grad.copy_(grads[2])
        opt.step()
    same_bits("flat_param after the resumed step", flat1.flat_param, flat2.flat_param)
    assert opt2.step_num == 3 and opt1.lr == opt2.lr
