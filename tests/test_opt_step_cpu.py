"""Host side of the device optimizer step (sbl_grad_sumsq, sbl_opt_finalize, sbl_adam_step_dev; FusedAdam's device mode):
argument validation before any launch, the unchanged default surface of FusedAdam, and `finalize_ref`, a restatement of
sbl_opt_finalize's rule in Python doubles that is checked here against TransformerOptimizer and
torch.nn.utils.clip_grad_norm_ and that tests/test_opt_step_gpu.py imports as its oracle."""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

STEP, SKIPPED, GRAD_NORM, CLIP_COEF, LR, STEP_SIZE, INV_SQRT_BC2, SKIP = range(8)


def f32(x):
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def finalize_ref(state, sumsq, max_norm=0.0, skip_nonfinite=False, noam=None, betas=(0.9, 0.98)):
    """sbl_opt_finalize in Python doubles: `state` (8 floats, include/sbl_hip.h SBL_OPT_*) and the total sum of squares in,
    the new state out.  The betas reach the kernel as floats."""
    s = [float(v) for v in state]
    b1, b2 = f32(betas[0]), f32(betas[1])
    sumsq = float(sumsq)
    norm = math.sqrt(sumsq) if sumsq == sumsq and sumsq >= 0 else float("nan")
    finite = math.isfinite(sumsq)
    if max_norm > 0:
        c = max_norm / (norm + 1e-6)
        coef = c if c < 1.0 else 1.0            # fmin: a NaN quotient gives 1
    else:
        coef = 1.0
    s[GRAD_NORM], s[CLIP_COEF] = norm, coef
    if finite or not skip_nonfinite:
        t = int(s[STEP]) + 1
        if noam is not None:
            k, warmup = noam
            s[LR] = k * 512 ** -0.5 * min(t ** -0.5, t * warmup ** -1.5)
        s[STEP] = float(t)
        s[STEP_SIZE] = s[LR] / (1.0 - b1 ** t)
        s[INV_SQRT_BC2] = 1.0 / math.sqrt(1.0 - b2 ** t)
        s[SKIP] = 0.0
    else:
        s[SKIPPED] += 1.0
        s[SKIP] = 1.0
    return s


def _host_addr(buf, misalign=0):
    return ((ctypes.addressof(buf) + 15) & ~15) + misalign


def test_entry_points_reject_bad_arguments_on_the_host():
    """Validation happens before any launch; the addresses are host dummies and nothing dereferences them."""
    from sbl_for_multilingual_lip_reading_amd import _lib
    buf = ctypes.create_string_buffer(256)
    a = _host_addr(buf)
    with pytest.raises(_lib.SblHipError, match="sbl_grad_sumsq: null pointer"):
        _lib.call("sbl_grad_sumsq", None, 4, 1.0, 0.0, a, 8, 0, None)
    with pytest.raises(_lib.SblHipError, match="sbl_grad_sumsq: null pointer"):
        _lib.call("sbl_grad_sumsq", a, 4, 1.0, 0.0, None, 8, 0, None)
    with pytest.raises(_lib.SblHipError, match="sbl_grad_sumsq: n=0 must be positive"):
        _lib.call("sbl_grad_sumsq", a, 0, 1.0, 0.0, a, 8, 0, None)
    with pytest.raises(_lib.SblHipError, match="sbl_grad_sumsq: unaligned"):
        _lib.call("sbl_grad_sumsq", a, 4, 1.0, 0.0, a + 4, 8, 0, None)
    with pytest.raises(_lib.SblHipError, match="sbl_grad_sumsq: unaligned"):
        _lib.call("sbl_grad_sumsq", a + 2, 4, 1.0, 0.0, a, 8, 0, None)
    # 1025 elements = 257 float4 -> 2 blocks; a workspace of 8 doubles holds them at offset 6, not at 7, and 3000 float4-
    # blocks are capped at 2048 partials
    with pytest.raises(_lib.SblHipError, match="too small for 2 partials at offset 7"):
        _lib.call("sbl_grad_sumsq", a, 1025, 1.0, 0.0, a, 8, 7, None)
    with pytest.raises(_lib.SblHipError, match="too small for 2048 partials at offset 0"):
        _lib.call("sbl_grad_sumsq", a, 3000 * 1024, 1.0, 0.0, a, 2047, 0, None)
    with pytest.raises(_lib.SblHipError, match="too small"):
        _lib.call("sbl_grad_sumsq", a, 4, 1.0, 0.0, a, 8, -1, None)

    with pytest.raises(_lib.SblHipError, match="sbl_opt_finalize: null pointer"):
        _lib.call("sbl_opt_finalize", None, a, 1, 0.0, 0, 0.0, 0.0, 0.9, 0.98, None)
    with pytest.raises(_lib.SblHipError, match="sbl_opt_finalize: nparts=0 must be positive"):
        _lib.call("sbl_opt_finalize", a, a, 0, 0.0, 0, 0.0, 0.0, 0.9, 0.98, None)
    with pytest.raises(_lib.SblHipError, match="sbl_opt_finalize: unaligned"):
        _lib.call("sbl_opt_finalize", a + 4, a, 1, 0.0, 0, 0.0, 0.0, 0.9, 0.98, None)
    with pytest.raises(_lib.SblHipError, match="Noam schedule needs"):
        _lib.call("sbl_opt_finalize", a, a, 1, 0.0, 0, 0.2, 0.0, 0.9, 0.98, None)
    with pytest.raises(_lib.SblHipError, match="betas outside"):
        _lib.call("sbl_opt_finalize", a, a, 1, 0.0, 0, 0.0, 0.0, 1.0, 0.98, None)

    with pytest.raises(_lib.SblHipError, match="sbl_adam_step_dev: null pointer"):
        _lib.call("sbl_adam_step_dev", a, a, a, a, 4, None, 0.9, 0.98, 1e-9, 1.0, 0.0, None)
    with pytest.raises(_lib.SblHipError, match="sbl_adam_step_dev: null pointer"):
        _lib.call("sbl_adam_step_dev", a, None, a, a, 4, a, 0.9, 0.98, 1e-9, 1.0, 0.0, None)
    with pytest.raises(_lib.SblHipError, match="sbl_adam_step_dev: n=-3 must be positive"):
        _lib.call("sbl_adam_step_dev", a, a, a, a, -3, a, 0.9, 0.98, 1e-9, 1.0, 0.0, None)
    with pytest.raises(_lib.SblHipError, match="sbl_adam_step_dev: unaligned state buffer"):
        _lib.call("sbl_adam_step_dev", a, a, a, a, 4, a + 4, 0.9, 0.98, 1e-9, 1.0, 0.0, None)
    with pytest.raises(_lib.SblHipError, match="sbl_adam_step_dev: unaligned buffer"):
        _lib.call("sbl_adam_step_dev", a, a, a + 2, a, 4, a, 0.9, 0.98, 1e-9, 1.0, 0.0, None)


def test_opt_blocks_mirrors_the_header():
    from sbl_for_multilingual_lip_reading_amd import ops
    hdr = open(__file__.rsplit("/tests/", 1)[0] + "/include/sbl_hip.h").read()
    assert "#define SBL_OPT_MAX_BLOCKS %d\n" % ops.OPT_MAX_BLOCKS in hdr and "#define SBL_OPT_STATE_SLOTS %d\n" % ops.OPT_STATE_SLOTS in hdr
    for name in ("STEP", "SKIPPED", "GRAD_NORM", "CLIP_COEF", "LR", "STEP_SIZE", "INV_SQRT_BC2", "SKIP"):
        assert "#define SBL_OPT_%s %d\n" % (name, getattr(ops, "OPT_" + name)) in hdr
        assert getattr(ops, "OPT_" + name) == globals()[name]
    assert [ops.opt_blocks(n) for n in (1, 4, 1024, 1025, 2048 * 1024, 2048 * 1024 + 1, 1 << 30)] == [1, 1, 1, 2, 2048, 2048, 2048]


class _FakeFlat:
    """The slice of dp.FlatModel that FusedAdam touches, on CPU tensors."""

    def __init__(self, n=12):
        self.model = torch.nn.Linear(3, 2)
        self.flat_param = torch.zeros(n)
        self.flat_grad = torch.zeros(n)
        self.numel = n
        self.slots = [(p, 0, 4) for p in self.model.parameters()]

    def zero_grad(self):
        self.flat_grad.zero_()

    def trainable_ranges(self):
        return [(0, self.numel)]


def test_fused_adam_default_surface_is_unchanged():
    from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import FusedAdam
    opt = FusedAdam(_FakeFlat(), lr=3e-4)
    assert not opt.device_mode and not hasattr(opt, "opt_state")
    sd = opt.state_dict()
    assert set(sd) == {"step", "exp_avg", "exp_avg_sq", "lr"}
    assert sd["step"] == 0 and sd["lr"] == 3e-4
    opt.load_state_dict({"step": 7, "exp_avg": torch.ones(12), "exp_avg_sq": torch.ones(12), "lr": 1e-2})
    assert opt.step_count == 7 and opt.param_groups[0]["lr"] == 1e-2 and float(opt.exp_avg.sum()) == 12.0
    for kw in ({"max_grad_norm": 1.0}, {"clip_value": 0.5}, {"skip_nonfinite": True}, {"noam": (0.2, 4000)}):
        dev = FusedAdam(_FakeFlat(), **kw)
        assert dev.device_mode and set(dev.state_dict()) == {"step", "exp_avg", "exp_avg_sq", "lr", "opt_state"}
        assert dev.opt_state.dtype == torch.float64 and dev.opt_state.numel() == 8
    with pytest.raises(ValueError):
        FusedAdam(_FakeFlat(), max_grad_norm=-1.0)


def test_device_noam_optimizer_host_surface_follows_transformer_optimizer(tmp_path):
    """step_num's setter and _update_lr() write the state from the host (no kernel): the rate and the bias factors they leave
    are the ones TransformerOptimizer / sbl_adam_step compute, and the state round-trips through checkpoint.py."""
    from sbl_for_multilingual_lip_reading_amd import checkpoint
    from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import DeviceNoamOptimizer, FusedAdam, TransformerOptimizer
    with pytest.raises(ValueError):
        DeviceNoamOptimizer(FusedAdam(_FakeFlat(), max_grad_norm=1.0))
    for k, warmup in ((0.2, 4000), (0.5, 2)):
        ref = TransformerOptimizer(FusedAdam(_FakeFlat()), warmup_steps=warmup, k=k)
        opt = DeviceNoamOptimizer(FusedAdam(_FakeFlat(), noam=(k, warmup)))
        assert opt.step_num == 0 and opt.lr == ref.lr and (opt.k, opt.warmup_steps) == (k, warmup)
        for _ in range(5):
            ref._update_lr()
            opt._update_lr()
            assert opt.step_num == ref.step_num and opt.lr == ref.lr
        opt.step_num = ref.step_num = warmup + 1
        ref.step_num -= 1
        ref._update_lr()
        assert opt.lr == ref.lr
        s = opt.optimizer.opt_state.tolist()
        t = warmup + 1
        assert s[STEP] == t and s[STEP_SIZE] == ref.lr / (1.0 - f32(0.9) ** t) and s[INV_SQRT_BC2] == 1.0 / math.sqrt(1.0 - f32(0.98) ** t)
    model = opt.optimizer.flat.model
    checkpoint.save_checkpoint(tmp_path / "ck.pt", model, opt)
    opt2 = DeviceNoamOptimizer(FusedAdam(_FakeFlat(), noam=(0.5, 2)))
    checkpoint.load_checkpoint(tmp_path / "ck.pt", opt2.optimizer.flat.model, opt2)
    assert opt2.step_num == 3 and torch.equal(opt2.optimizer.opt_state, opt.optimizer.opt_state)
    # a default-mode checkpoint loaded into device mode: the step count carries over, the rest follows from it
    plain = TransformerOptimizer(FusedAdam(_FakeFlat()), warmup_steps=2, k=0.5)
    for _ in range(3):
        plain._update_lr()
    plain.optimizer.step_count = 3
    checkpoint.save_checkpoint(tmp_path / "plain.pt", model, plain)
    opt3 = DeviceNoamOptimizer(FusedAdam(_FakeFlat(), noam=(0.5, 2)))
    checkpoint.load_checkpoint(tmp_path / "plain.pt", opt3.optimizer.flat.model, opt3)
    assert opt3.step_num == 3 and opt3.lr == plain.lr


def test_finalize_ref_against_torch():
    """The restatement itself: Noam rate == TransformerOptimizer's, coefficient and norm == clip_grad_norm_'s (on float64
    tensors, where torch's own arithmetic is the same double arithmetic), bias factors == sbl_adam_step's host formula, and
    the skip rule."""
    from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import FusedAdam, TransformerOptimizer
    for k, warmup in ((0.2, 4000), (0.5, 2)):
        ref = TransformerOptimizer(FusedAdam(_FakeFlat()), warmup_steps=warmup, k=k)
        s = [0.0] * 8
        for t in range(1, 8):
            ref._update_lr()
            s = finalize_ref(s, 1.0, noam=(k, warmup))
            assert s[STEP] == t and s[LR] == ref.lr and s[SKIP] == 0.0
            assert s[STEP_SIZE] == ref.lr / (1.0 - f32(0.9) ** t) and s[INV_SQRT_BC2] == 1.0 / math.sqrt(1.0 - f32(0.98) ** t)
    g = np.random.RandomState(3).randn(1000)
    for max_norm in (1.0, 1e3):
        p = torch.nn.Parameter(torch.zeros(1000, dtype=torch.float64))
        p.grad = torch.from_numpy(g.copy())
        total = torch.nn.utils.clip_grad_norm_([p], max_norm)
        s = finalize_ref([0.0] * 4 + [1e-3] + [0.0] * 3, float((g * g).sum()), max_norm=max_norm)
        assert abs(s[GRAD_NORM] - float(total)) <= 64 * np.spacing(float(total))      # torch sums in another order
        assert np.allclose(p.grad.numpy(), g * s[CLIP_COEF], rtol=1e-13, atol=0)
        assert (s[CLIP_COEF] == 1.0) == (max_norm == 1e3) and s[LR] == 1e-3 and s[STEP] == 1.0
    # skip rule: inf / NaN sums skip only when asked to; t, lr and the factors are untouched by a skip
    s1 = finalize_ref([0.0] * 4 + [1e-3] + [0.0] * 3, 4.0, max_norm=1.0, skip_nonfinite=True)
    assert s1[CLIP_COEF] == 1.0 / (2.0 + 1e-6)
    for bad in (float("inf"), float("nan")):
        s2 = finalize_ref(s1, bad, max_norm=1.0, skip_nonfinite=True)
        assert s2[SKIP] == 1.0 and s2[SKIPPED] == 1.0 and s2[STEP] == 1.0 and s2[LR:SKIP] == s1[LR:SKIP]
        assert not math.isfinite(s2[GRAD_NORM])
        s3 = finalize_ref(s2, 1.0, max_norm=1.0, skip_nonfinite=True)
        assert s3[SKIP] == 0.0 and s3[SKIPPED] == 1.0 and s3[STEP] == 2.0
        s4 = finalize_ref(s1, bad, max_norm=1.0, skip_nonfinite=False)
        assert s4[SKIP] == 0.0 and s4[STEP] == 2.0 and s4[SKIPPED] == 0.0
