"""Weight averaging in the device optimizer step on the GPU: sbl_adam_ema_step_dev against its parent sbl_adam_step_dev
(p, m, v bit for bit) and a float64 restatement of the average at the edges of the launch geometry, the skip rule,
sbl_swap_f32, FusedAdam(ema_decay=) over a stub flat with a frozen middle, capture and replay, the whole model through
averaged() and the checkpoint, and two replicas fed one summed gradient.  Nothing is compared against the new kernel itself.

The oracle of d_t and w is tests/test_ema_cpu.py (checked there at fixed points); dev, host, u, check, same_bits, new_state,
StubFlat and build_model are those of tests/test_opt_step_gpu.py.

Bound of the average (u = 2^-24): e_new = fl(e + w * fl(p - e)) has one rounding for the difference, one each for product
and sum (the kernel fuses those two: one fewer), and w itself is a rounded float, which the reference takes as given.  That
is at most u |e_new| + 3 u w |p - e|; |e_new| <= max(|e|, |p|) and w |p - e| <= |e| + |p|, so 4 u (|e| + |p|) holds to first
order and the fifth u covers the second-order terms: |e_got - e_ref| <= 5 u (|e_old| + |p_new|)."""
import math

import numpy as np
import pytest
import torch

from sbl_for_multilingual_lip_reading_amd import detfill
from test_ema_cpu import ema_weight
from test_opt_step_cpu import CLIP_COEF, INV_SQRT_BC2, SKIP, STEP_SIZE, f32
from test_opt_step_gpu import B1, B2, DEV, EPS, EW_CAP, U, StubFlat, build_model, check, dev, f64, host, new_state, same_bits, u

pytestmark = pytest.mark.gpu

GUARD = 8                                   # floats: 32 bytes, so a view at GUARD keeps the base's 16-byte alignment
SIZES = [1, 3, 257, 4 * 256 + 1, EW_CAP + 333]
DECAY = 0.9999


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
def framed(a, off):
    """A device copy of `a` inside a NaN frame, `off` floats past a 16-byte boundary: (base, view)."""
    n = a.shape[0]
    base = torch.full((GUARD + off + n + GUARD,), float("nan"), device=DEV, dtype=torch.float32)
    view = base[GUARD + off:GUARD + off + n]
    view.copy_(dev(a))
    assert view.data_ptr() % 16 == (4 * off) % 16
    return base, view


def frame_intact(what, base, off, n):
    assert bool(torch.isnan(base[:GUARD + off]).all()) and bool(torch.isnan(base[GUARD + off + n:]).all()), what + ": guard overwritten"


def adam_inputs(n):
    p0 = u("ema.p", (n,))
    g0 = u("ema.g", (n,)) * np.float32(0.01)
    m0 = u("ema.m", (n,)) * np.float32(0.01)
    v0 = (u("ema.v", (n,)) * np.float32(0.01)) ** 2
    e0 = u("ema.e", (n,))
    return p0, g0, m0, v0, e0


def state_at(t, lr=1e-3, coef=0.75, skip=0.0):
    """The state buffer as sbl_opt_finalize leaves it after the t-th applied step (a clip coefficient below 1)."""
    s = new_state(t, f32(lr))
    s[CLIP_COEF] = coef
    s[STEP_SIZE] = f32(lr) / (1.0 - f32(B1) ** t)
    s[INV_SQRT_BC2] = 1.0 / math.sqrt(1.0 - f32(B2) ** t)
    s[SKIP] = skip
    return dev(s, np.float64)


def ema_bound(e_old, p_new):
    return 5 * U * (np.abs(f64(e_old)) + np.abs(f64(p_new)))


# --------------------------------------------------------------------------- 1. kernel against its parent and float64
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_ema_kernel_against_parent_and_float64(ops, n, off):
    """Sizes: one thread of the tail alone (1, 3), a partial block (257), two blocks plus the n % 4 tail (1025) and the
    grid-stride wrap past the 2048-block cap (8192 * 256 + 333); off = 1 moves all five buffers one float off a 16-byte
    boundary (the scalar route).  At t = 1, 7 (warm-up: d_t = 2/11, 8/17) and 10^6 (capped at the decay), warm-up on and
    off, with a gradient scale and an element clamp inside the data range: p, m, v carry the bits of sbl_adam_step_dev on
    copies of the same inputs, e is within 5 u (|e_old| + |p_new|) of e_old + w (p_new - e_old) in float64 from the kernel's
    own p_new, the gradient and the state are read only, and the NaN frames stay whole.
    measured: worst err/bound 0.26 (t = 1 in warm-up, w = 9/11), 0.19 - 0.20 elsewhere."""
    p0, g0, m0, v0, e0 = adam_inputs(n)
    gscale, clip = 0.5, 2.0 ** -9
    for t in (1, 7, 10 ** 6):
        for warm in (True, False):
            tag = "ema[n=%d off=%d t=%d warm=%d] " % (n, off, t, warm)
            st = state_at(t)
            st_before = st.clone()
            ref = [framed(a, off) for a in (p0, g0, m0, v0)]
            ops.adam_step_dev(ref[0][1], ref[1][1], ref[2][1], ref[3][1], st, B1, B2, EPS, gscale, clip)
            got = [framed(a, off) for a in (p0, g0, m0, v0, e0)]
            ops.adam_ema_step_dev(got[0][1], got[1][1], got[2][1], got[3][1], got[4][1], st, B1, B2, EPS, gscale, clip, DECAY, warm)
            for name, (rb, _), (gb, _) in zip("pgmv", ref, got):
                same_bits(tag + name + " against sbl_adam_step_dev (frame included)", gb, rb)
            for name, (gb, _) in zip("pgmve", got):
                frame_intact(tag + name, gb, off, n)
            same_bits(tag + "gradient", got[1][1], dev(g0))
            same_bits(tag + "state", st, st_before)
            assert not torch.equal(got[0][1], dev(p0)), tag + "the update moved nothing"
            w64 = float(ema_weight(t, DECAY, warm))
            if t == 1:
                assert w64 == (float(np.float32(9.0 / 11.0)) if warm else float(np.float32(1.0 - DECAY)))
            p_new = f64(host(got[0][1]))
            e_ref = f64(e0) + w64 * (p_new - f64(e0))
            check(tag + "e", got[4][1], e_ref, ema_bound(e0, p_new))


# --------------------------------------------------------------------------- 2. skip
@pytest.mark.parametrize("off", [0, 1])
def test_skip_flag_leaves_all_five_buffers_alone(ops, off):
    """state[SBL_OPT_SKIP] = 1: p, g, m, v, e and their frames keep their bits (1025 elements: loop and tail lanes)."""
    n = 4 * 256 + 1
    bufs = [framed(a, off) for a in adam_inputs(n)]
    before = [b.clone() for b, _ in bufs]
    st = state_at(7, skip=1.0)
    ops.adam_ema_step_dev(*[v for _, v in bufs], st, B1, B2, EPS, 1.0, 0.0, DECAY, True)
    for name, (b, _), b0 in zip("pgmve", bufs, before):
        same_bits("skipped step changed " + name, b, b0)
    same_bits("state", st, state_at(7, skip=1.0))
    st[SKIP] = 0.0                                        # the same call without the flag does write
    ops.adam_ema_step_dev(*[v for _, v in bufs], st, B1, B2, EPS, 1.0, 0.0, DECAY, True)
    assert not torch.equal(bufs[4][1], before[4][GUARD + off:GUARD + off + n]) and not torch.equal(bufs[0][1], before[0][GUARD + off:GUARD + off + n])


# --------------------------------------------------------------------------- 3. swap
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_swap_is_exact_and_twice_is_the_identity(ops, n, off):
    a0, b0 = u("swap.a", (n,)).copy(), u("swap.b", (n,)).copy()
    if n >= 3:                                            # bit patterns an arithmetic exchange would not carry over
        a0[0], a0[n - 1], b0[1] = np.float32("nan"), np.float32(-0.0), np.float32("inf")
    (ab, a), (bb, b) = framed(a0, off), framed(b0, off)
    ops.swap_(a, b)
    same_bits("a after one swap", a, dev(b0))
    same_bits("b after one swap", b, dev(a0))
    ops.swap_(a, b)
    same_bits("a after two swaps", a, dev(a0))
    same_bits("b after two swaps", b, dev(b0))
    frame_intact("a", ab, off, n)
    frame_intact("b", bb, off, n)
    if n >= 257:                                          # one side aligned, the other not: the scalar route
        (_, c), (_, d) = framed(a0, 0), framed(b0, 1)
        ops.swap_(c, d)
        same_bits("mixed alignment a", c, dev(b0))
        same_bits("mixed alignment b", d, dev(a0))


def test_swap_rejects_overlapping_ranges(ops):
    from sbl_for_multilingual_lip_reading_amd import _lib
    x = dev(u("swap.a", (64,)))
    x0 = x.clone()
    for a, b in ((x[0:32], x[0:32]), (x[0:32], x[31:63]), (x[16:48], x[0:32]), (x[1:33], x[0:32])):
        with pytest.raises(_lib.SblHipError, match="overlap"):
            ops.swap_(a, b)
    same_bits("rejected calls wrote", x, x0)
    ops.swap_(x[0:32], x[32:64])                          # adjacent ranges are fine
    same_bits("adjacent halves", x, torch.cat([x0[32:], x0[:32]]))


# --------------------------------------------------------------------------- 4. optimizer on a stub flat
N_STUB = 4 * 256 + 1
STUB_RANGES = [(0, 400), (601, N_STUB)]          # frozen middle; the second range starts off a 16-byte boundary


def stub_grad(i):
    return u("ema.step%d" % i, (N_STUB,)) * np.float32(0.01)


def test_fused_adam_average_follows_the_float64_recurrence(ops):
    """Five steps over two trainable ranges with a frozen middle, the third with an inf in the gradient under
    skip_nonfinite; decay 0.3, so t = 1, 2 run in warm-up (2/11, 3/12) and t = 3, 4 at the cap (4/13 > 0.3).  Every applied
    step is held to the bound of the kernel test from the recorded fp32 parameters and the recorded previous average, and
    the final average to the float64 recurrence E_t = E_{t-1} + w_t (p_t - E_{t-1}) from E_0 = p_0 within the sum of the
    per-step bounds (each step scales the error carried in by 1 - w_t <= 1).  The skipped step leaves the average's bits
    alone, the frozen range keeps ema == p == p_0 throughout, and steps_applied is 4.
    measured: worst err/bound 0.10 per step, 0.03 for the recurrence over the four steps."""
    from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import FusedAdam
    decay = 0.3
    p0 = u("ema.p", (N_STUB,))
    flat = StubFlat(p0, STUB_RANGES)
    opt = FusedAdam(flat, lr=1e-3, betas=(B1, B2), eps=EPS, max_grad_norm=0.05, skip_nonfinite=True, ema_decay=decay)
    same_bits("ema starts as the parameters", opt.ema, flat.flat_param)
    mask = np.zeros(N_STUB, dtype=bool)
    for a, b in STUB_RANGES:
        mask[a:b] = True
    E, acc, t = f64(p0).copy(), np.zeros(N_STUB), 0
    for i in range(1, 6):
        g = stub_grad(i).copy()
        if i == 3:
            g[N_STUB - 1] = np.inf
        e_prev, p_prev = host(opt.ema).copy(), host(flat.flat_param).copy()
        flat.flat_grad.copy_(dev(g))
        opt.step()
        e_now, p_now = host(opt.ema), host(flat.flat_param)
        assert np.array_equal(e_now[~mask].view(np.int32), p0[~mask].view(np.int32)), "frozen range of the average moved"
        assert np.array_equal(p_now[~mask].view(np.int32), p0[~mask].view(np.int32)), "frozen parameters moved"
        if i == 3:
            assert np.array_equal(e_now.view(np.int32), e_prev.view(np.int32)), "skipped step changed the average"
            assert np.array_equal(p_now.view(np.int32), p_prev.view(np.int32))
            assert opt.steps_skipped == 1
            continue
        t += 1
        w64 = float(ema_weight(t, decay))
        assert (w64 == float(np.float32(1.0 - decay))) == (t >= 3)
        step_bound = ema_bound(e_prev, p_now)
        check("stub step %d (t=%d), one step" % (i, t), e_now[mask], (f64(e_prev) + w64 * (f64(p_now) - f64(e_prev)))[mask], step_bound[mask])
        E = E + w64 * (f64(p_now) - E)
        acc += step_bound
        assert float((p_now != p_prev)[mask].mean()) > 0.99
    assert opt.steps_applied == 4 and t == 4
    check("stub, float64 recurrence over 4 steps", host(opt.ema)[mask], E[mask], acc[mask])
    assert float(np.abs(host(opt.ema) - host(flat.flat_param))[mask].max()) > 1e-4


# --------------------------------------------------------------------------- 5. graph
def snapshot(opt):
    return [t.clone() for t in (opt.flat.flat_param, opt.exp_avg, opt.exp_avg_sq, opt.ema, opt.opt_state)]


def test_captured_step_and_swap_replay_bit_exactly(ops):
    """zero_grad + a gradient fill from a static buffer + step() captured once and replayed three times (a new gradient in the
    static buffer before each replay, the middle one with an inf) == three eager steps: p, m, v, ema and the state bit for
    bit.  swap_ema() captured: one replay leaves the old average in the parameters and the old parameters in `ema` (over the
    trainable ranges), a second one restores every bit."""
    from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import FusedAdam
    grads = [stub_grad(1), stub_grad(2).copy(), stub_grad(3)]
    grads[1][700] = np.inf

    def make():
        flat = StubFlat(u("ema.p", (N_STUB,)), STUB_RANGES)
        return FusedAdam(flat, betas=(B1, B2), eps=EPS, max_grad_norm=0.05, skip_nonfinite=True, noam=(0.5, 2), ema_decay=0.5)

    eager = make()
    for g in grads:
        eager.zero_grad()
        eager.flat.flat_grad.add_(dev(g))
        eager.step()
    assert eager.steps_applied == 2 and eager.steps_skipped == 1
    opt = make()
    gbuf = torch.zeros(N_STUB, device=DEV)
    gd = [dev(g) for g in grads]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        opt.zero_grad()
        opt.flat.flat_grad.add_(gbuf)
        opt.step()
    for name, a, b in zip(("p", "m", "v", "ema", "state"), snapshot(make()), snapshot(opt)):
        same_bits("capture itself changed " + name, a, b)
    for g in gd:
        gbuf.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(("p", "m", "v", "ema", "state"), snapshot(eager), snapshot(opt)):
        same_bits("replayed " + name, a, b)
    assert not torch.equal(opt.ema, opt.flat.flat_param)

    before = snapshot(opt)
    swap = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(swap, stream=stream):
        opt.swap_ema()
    for name, a, b in zip(("p", "m", "v", "ema", "state"), before, snapshot(opt)):
        same_bits("capturing the swap changed " + name, a, b)
    swap.replay()
    torch.cuda.synchronize()
    for a, b in STUB_RANGES:
        same_bits("parameters hold the average", opt.flat.flat_param[a:b], before[3][a:b])
        same_bits("ema holds the live weights", opt.ema[a:b], before[0][a:b])
    same_bits("frozen parameters", opt.flat.flat_param[400:601], before[0][400:601])
    swap.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(("p", "m", "v", "ema", "state"), before, snapshot(opt)):
        same_bits("two swaps, " + name, a, b)


# --------------------------------------------------------------------------- 6. whole model
# Gradients of a real backward are sums of float atomics, so two runs of one training step do not agree bit for bit; the
# steps below plant seeded gradients in the flat buffer instead (as test_device_mode_checkpoint_round_trip does), which
# makes every run of make_run() the same bits and lets the comparisons be exact.  The forwards are real.
MB, MT, MH, MW = 2, 4, 24, 24


def make_run():
    from sbl_for_multilingual_lip_reading_amd import dp
    from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import DeviceNoamOptimizer, FusedAdam
    m = build_model(1, 1).train()
    m.decoder.coins_dev = torch.zeros(16, dtype=torch.int32, device=DEV)
    flat = dp.FlatModel(m)
    opt = DeviceNoamOptimizer(FusedAdam(flat, betas=(B1, B2), eps=EPS, max_grad_norm=1.0, noam=(0.02, 2), ema_decay=0.5))
    return m, flat, opt


def planted(flat, k):
    gen = torch.Generator(device=DEV).manual_seed(100 + k)
    return torch.randn(flat.numel, device=DEV, generator=gen) * 0.01


def plant_steps(flat, opt, ks):
    for k in ks:
        flat.flat_grad.copy_(planted(flat, k))
        opt.step()


def eval_forward(m):
    x, l2r, r2l = detfill.synthetic_batch(MB, MT, MH, MW, 51)
    was = m.training
    m.eval()
    with torch.no_grad():
        pl, _, pr, _ = m(torch.from_numpy(x).to(DEV), torch.from_numpy(l2r).to(DEV), torch.from_numpy(r2l).to(DEV))
    m.train(was)
    assert bool(torch.isfinite(pl).all()) and bool(torch.isfinite(pr).all())
    return pl.clone(), pr.clone()


def test_averaged_forward_equals_a_model_loaded_from_the_averaged_state_dict(ops):
    """(a) After three steps (the decay of 0.5 moves the average visibly) and an eval forward with the LIVE weights, which
    fills the packed-weight cache, the eval forward inside averaged() equals bit for bit that of a second model built fresh
    and loaded by load_state_dict from the state_dict() taken inside the context; it differs from the live forward.  A stale
    packed image after the raw-kernel exchange would leave the trunk convolutions on the live weights."""
    from sbl_for_multilingual_lip_reading_amd import dp
    m, flat, opt = make_run()
    plant_steps(flat, opt, (1, 2, 3))
    live_p, snapshot_ema = flat.flat_param.clone(), opt.optimizer.ema.clone()
    live_out = eval_forward(m)
    assert float((snapshot_ema - live_p).abs().max()) > 1e-4
    with opt.averaged():
        same_bits("parameters inside the context", flat.flat_param, snapshot_ema)
        same_bits("the optimizer's state_dict inside the context", opt.optimizer.state_dict()["ema"], snapshot_ema)
        avg_out = eval_forward(m)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        with pytest.raises(RuntimeError, match="inside averaged"):
            opt.step()
    same_bits("live weights after the context", flat.flat_param, live_p)
    same_bits("the average after the context", opt.optimizer.ema, snapshot_ema)
    m2 = build_model(1, 1)
    m2.decoder.coins_dev = torch.zeros(16, dtype=torch.int32, device=DEV)
    dp.FlatModel(m2)
    m2.load_state_dict(sd)
    ref_out = eval_forward(m2)
    for name, a, b, c in zip(("l2r", "r2l"), avg_out, ref_out, live_out):
        same_bits("averaged forward, " + name, a, b)
        assert not torch.equal(a, c), "the averaged forward equals the live one"


def test_context_restores_weights_and_packed_images(ops):
    """(b) A run that enters averaged() after three steps (and runs a forward inside, and leaves once through an exception)
    and a run that never does: after the context the eval forward - packed images included - and, after one more step,
    p, m, v and ema are the same bits in both."""
    ma, fa, oa = make_run()
    mb, fb, ob = make_run()
    plant_steps(fa, oa, (1, 2, 3))
    plant_steps(fb, ob, (1, 2, 3))
    eval_forward(ma)                                      # fills the pack cache with the live weights
    with oa.averaged():
        eval_forward(ma)
    with pytest.raises(KeyError):
        with oa.averaged():
            raise KeyError("body")
    same_bits("parameters after the context", fa.flat_param, fb.flat_param)
    same_bits("average after the context", oa.optimizer.ema, ob.optimizer.ema)
    for name, a, b in zip(("l2r", "r2l"), eval_forward(ma), eval_forward(mb)):
        same_bits("forward after the context, " + name, a, b)
    plant_steps(fa, oa, (4,))
    plant_steps(fb, ob, (4,))
    for name, a, b in zip(("p", "m", "v", "ema", "state"), snapshot(oa.optimizer), snapshot(ob.optimizer)):
        same_bits("step after the context, " + name, a, b)
    assert oa.step_num == 4


def test_averaged_checkpoint_and_resume(ops, tmp_path):
    """(c) save_checkpoint(averaged=True) + load_checkpoint into a fresh model and optimizer: the model holds the averaged
    weights and optimizer.ema the stored average (both the saver's `ema`, bit for bit), the saver's live weights are
    untouched; with the live weights restored from the companion checkpoint written with averaged=False, one more step gives
    the uninterrupted run's p and ema bit for bit."""
    from sbl_for_multilingual_lip_reading_amd import checkpoint
    m1, f1, o1 = make_run()
    plant_steps(f1, o1, (1, 2, 3))
    live, avg = f1.flat_param.clone(), o1.optimizer.ema.clone()
    checkpoint.save_checkpoint(tmp_path / "avg.pt", m1, o1, averaged=True, epoch=3)
    checkpoint.save_checkpoint(tmp_path / "live.pt", m1, o1, epoch=3)
    same_bits("saving moved the live weights", f1.flat_param, live)
    same_bits("saving moved the average", o1.optimizer.ema, avg)
    m2, f2, o2 = make_run()
    meta = checkpoint.load_checkpoint(tmp_path / "avg.pt", m2, o2)
    assert meta["epoch"] == 3 and o2.step_num == 3
    same_bits("the model holds the averaged weights", f2.flat_param, avg)
    same_bits("optimizer.ema holds the stored average", o2.optimizer.ema, avg)
    for (k, a), (_, b) in zip(m1.named_buffers(), m2.named_buffers()):
        assert torch.equal(a, b), k                           # buffers: the live BatchNorm statistics, not averaged
    checkpoint.load_checkpoint(tmp_path / "live.pt", m2)
    same_bits("live weights from the companion checkpoint", f2.flat_param, live)
    same_bits("loading the model alone left the average", o2.optimizer.ema, avg)
    plant_steps(f1, o1, (4,))
    plant_steps(f2, o2, (4,))
    for name, a, b in zip(("p", "m", "v", "ema", "state"), snapshot(o1.optimizer), snapshot(o2.optimizer)):
        same_bits("resumed step, " + name, a, b)
    # a checkpoint without an average starts it from the loaded weights
    ck = torch.load(tmp_path / "live.pt", weights_only=True)
    del ck["optimizer_state"]["ema"], ck["optimizer_state"]["ema_decay"]
    torch.save(ck, tmp_path / "old.pt")
    m3, f3, o3 = make_run()
    checkpoint.load_checkpoint(tmp_path / "old.pt", m3, o3)
    same_bits("no stored average: ema == the loaded weights", o3.optimizer.ema, live)


# --------------------------------------------------------------------------- 7. data-parallel consistency
def test_replicas_fed_one_summed_gradient_hold_one_average(ops):
    """Two optimizers as two replicas would run them: each gets the SUM of two micro-gradients and grad_scale = 0.5.  After
    three steps their ema (and p, m, v, state) agree bit for bit, and the average has moved."""
    from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import FusedAdam
    reps = [FusedAdam(StubFlat(u("ema.p", (N_STUB,)), STUB_RANGES), betas=(B1, B2), eps=EPS, grad_scale=0.5, max_grad_norm=0.05,
                      skip_nonfinite=True, noam=(0.5, 2), ema_decay=0.9) for _ in range(2)]
    for i in (1, 2, 3):
        summed = stub_grad(i) + stub_grad(10 + i)
        for r in reps:
            r.zero_grad()
            r.flat.flat_grad.add_(dev(summed))
            r.step()
    for name, a, b in zip(("p", "m", "v", "ema", "state"), snapshot(reps[0]), snapshot(reps[1])):
        same_bits("replicas, " + name, a, b)
    assert reps[0].steps_applied == 3
    assert float((reps[0].ema - dev(u("ema.p", (N_STUB,)))).abs().max()) > 1e-4
