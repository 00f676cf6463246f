"""Host side of weight averaging in the device optimizer step (sbl_adam_ema_step_dev, sbl_swap_f32; FusedAdam(ema_decay=)):
`ema_decay_at` / `ema_weight`, a numpy restatement of the kernel's d_t and w that tests/test_ema_gpu.py imports as its
oracle, checked here at fixed points; argument validation of the two entry points before any launch; and the optimizer's
averaging surface (construction, state_dict, load_state_dict) over a CPU stub of dp.FlatModel."""
import ctypes

import numpy as np
import pytest
import torch


def ema_decay_at(t, decay, warmup=True):
    """d_t of sbl_adam_ema_step_dev in the kernel's double arithmetic: t is the applied-step count after the increment."""
    t, d = np.float64(t), np.float64(decay)
    return min(d, (np.float64(1.0) + t) / (np.float64(10.0) + t)) if warmup else d


def ema_weight(t, decay, warmup=True):
    """w = (float)(1 - d_t): the weight of the new parameters in e += w * (p_new - e)."""
    return np.float32(np.float64(1.0) - ema_decay_at(t, decay, warmup))


def test_decay_schedule_fixed_points():
    assert ema_decay_at(1, 0.9999) == np.float64(2.0) / np.float64(11.0)
    assert ema_weight(1, 0.9999) == np.float32(1.0 - 2.0 / 11.0)
    # (1 + t) / (10 + t) reaches 0.9999 at t = 89990 (89991 / 90000) and not before
    assert ema_decay_at(89989, 0.9999) < 0.9999 and ema_decay_at(89989, 0.9999) == np.float64(89990.0) / np.float64(89999.0)
    assert ema_decay_at(89990, 0.9999) == 0.9999 and ema_decay_at(89991, 0.9999) == 0.9999 and ema_decay_at(10 ** 9, 0.9999) == 0.9999
    ts = np.arange(1, 89990)
    assert np.all((1.0 + ts) / (10.0 + ts) < 0.9999)
    # the schedule never decreases and starts well below the cap
    d = [ema_decay_at(t, 0.9999) for t in range(1, 200)]
    assert all(a < b for a, b in zip(d, d[1:]))
    for t in (1, 7, 10 ** 6):
        assert ema_decay_at(t, 0.9999, warmup=False) == 0.9999 and ema_decay_at(t, 0.5, warmup=False) == 0.5
        assert ema_weight(t, 0.5, warmup=False) == np.float32(0.5)
    assert ema_decay_at(1, 0.1) == 0.1                                           # 2/11 > 0.1: a small decay caps at once
    assert ema_decay_at(7, 0.5) == np.float64(8.0) / np.float64(17.0) and ema_decay_at(8, 0.5) == 0.5      # 9/18
    assert ema_weight(10 ** 6, 0.9999) == np.float32(1.0 - 0.9999)


def _host_addr(buf, misalign=0):
    return ((ctypes.addressof(buf) + 15) & ~15) + misalign


def test_new_entry_points_reject_bad_arguments_on_the_host():
    """Validation happens before any launch; the addresses are host dummies and nothing dereferences them."""
    from sbl_for_multilingual_lip_reading_amd import _lib
    buf = ctypes.create_string_buffer(512)
    a = _host_addr(buf)
    ok = (0.9, 0.98, 1e-9, 1.0, 0.0)

    def ema(p=a, g=a, m=a, v=a, e=a, n=4, st=a, decay=0.999, warm=1):
        _lib.call("sbl_adam_ema_step_dev", p, g, m, v, e, n, st, *ok, decay, warm, None)

    for kw in ({"p": None}, {"g": None}, {"m": None}, {"v": None}, {"e": None}, {"st": None}):
        with pytest.raises(_lib.SblHipError, match="sbl_adam_ema_step_dev: null pointer"):
            ema(**kw)
    for n in (0, -3):
        with pytest.raises(_lib.SblHipError, match="sbl_adam_ema_step_dev: n=%d must be positive" % n):
            ema(n=n)
    with pytest.raises(_lib.SblHipError, match="sbl_adam_ema_step_dev: unaligned state buffer"):
        ema(st=a + 4)
    for kw in ({"p": a + 2}, {"g": a + 1}, {"m": a + 2}, {"v": a + 3}, {"e": a + 2}):
        with pytest.raises(_lib.SblHipError, match="sbl_adam_ema_step_dev: unaligned buffer"):
            ema(**kw)
    for decay in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(_lib.SblHipError, match="outside \\(0, 1\\)"):
            ema(decay=decay)

    with pytest.raises(_lib.SblHipError, match="sbl_swap_f32: null pointer"):
        _lib.call("sbl_swap_f32", None, a, 4, None)
    with pytest.raises(_lib.SblHipError, match="sbl_swap_f32: null pointer"):
        _lib.call("sbl_swap_f32", a, None, 4, None)
    with pytest.raises(_lib.SblHipError, match="sbl_swap_f32: n=0 must be positive"):
        _lib.call("sbl_swap_f32", a, a + 64, 0, None)
    with pytest.raises(_lib.SblHipError, match="sbl_swap_f32: unaligned buffer"):
        _lib.call("sbl_swap_f32", a, a + 66, 4, None)
    # [a, a + 16 floats) against itself, shifted by one element either way, and shifted by 15 of 16 elements
    for b in (a, a + 4, a + 60):
        with pytest.raises(_lib.SblHipError, match="sbl_swap_f32: the two ranges of 16 elements overlap"):
            _lib.call("sbl_swap_f32", a, b, 16, None)
        with pytest.raises(_lib.SblHipError, match="sbl_swap_f32: the two ranges of 16 elements overlap"):
            _lib.call("sbl_swap_f32", b, a, 16, None)


def test_ops_refuse_cpu_tensors():
    from sbl_for_multilingual_lip_reading_amd import _lib, ops
    z = torch.zeros(8)
    with pytest.raises(_lib.SblHipError, match="no CPU path"):
        ops.swap_(z, torch.zeros(8))
    with pytest.raises(_lib.SblHipError, match="no CPU path"):
        ops.adam_ema_step_dev(z, z, z, z, z, torch.zeros(8, dtype=torch.float64), 0.9, 0.98, 1e-9)


class _FakeFlat:
    """The slice of dp.FlatModel that FusedAdam touches, on CPU tensors (tests/test_opt_step_gpu.py's StubFlat)."""

    def __init__(self, n=12, ranges=None):
        self.model = torch.nn.Linear(3, 2)
        self.flat_param = torch.arange(n, dtype=torch.float32) * 0.25 - 1.0
        self.flat_grad = torch.zeros(n)
        self.numel = n
        self._ranges = list(ranges) if ranges is not None else [(0, n)]
        self.slots = [None] * len(self._ranges)

    def zero_grad(self):
        self.flat_grad.zero_()

    def trainable_ranges(self):
        return list(self._ranges)


def test_fused_adam_averaging_surface():
    from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import DeviceNoamOptimizer, FusedAdam
    for bad in (0, 1, -0.1, 0.0, 1.0):
        with pytest.raises(ValueError, match="ema_decay"):
            FusedAdam(_FakeFlat(), ema_decay=bad)
    plain = FusedAdam(_FakeFlat(), noam=(0.2, 4000))
    assert plain.ema is None and plain.ema_decay is None and "ema" not in plain.state_dict()
    for call in (plain.swap_ema, plain.averaged, plain.reset_ema):
        with pytest.raises(RuntimeError, match="ema_decay"):
            call()

    flat = _FakeFlat()
    opt = FusedAdam(flat, ema_decay=0.999)
    assert opt.device_mode and opt.ema_warmup is True and opt.ema_decay == 0.999          # a decay alone turns device mode on
    assert torch.equal(opt.ema, flat.flat_param) and opt.ema.data_ptr() != flat.flat_param.data_ptr()
    sd = opt.state_dict()
    assert set(sd) == {"step", "exp_avg", "exp_avg_sq", "lr", "opt_state", "ema", "ema_decay"}
    assert sd["ema"] is opt.ema and sd["ema_decay"] == 0.999
    assert FusedAdam(_FakeFlat(), ema_decay=0.5, ema_warmup=False).ema_warmup is False

    # round trip: a different average, moments and step count come back
    opt.ema.mul_(3.0)
    opt.exp_avg.fill_(0.5)
    opt.set_steps_applied(7)
    saved = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
    flat2 = _FakeFlat()
    opt2 = FusedAdam(flat2, ema_decay=0.999)
    opt2.load_state_dict(saved)
    assert torch.equal(opt2.ema, saved["ema"]) and not torch.equal(opt2.ema, flat2.flat_param)
    assert opt2.steps_applied == 7 and torch.equal(opt2.exp_avg, saved["exp_avg"]) and torch.equal(opt2.opt_state, opt.opt_state)

    # a state dict without an average: ema == the flat parameters as they are at load time
    no_ema = {k: v for k, v in saved.items() if k not in ("ema", "ema_decay")}
    flat3 = _FakeFlat()
    opt3 = FusedAdam(flat3, ema_decay=0.999)
    opt3.ema.zero_()
    flat3.flat_param.add_(2.0)
    opt3.load_state_dict(no_ema)
    assert torch.equal(opt3.ema, flat3.flat_param) and opt3.steps_applied == 7

    # a stored average is ignored by an optimizer that keeps none
    opt4 = FusedAdam(_FakeFlat(), noam=(0.2, 4000))
    opt4.load_state_dict(saved)
    assert opt4.ema is None and "ema" not in opt4.state_dict() and opt4.steps_applied == 7

    # reset_ema, the step() guard inside the context, and DeviceNoamOptimizer's forwards
    flat.flat_param.add_(1.0)
    opt.reset_ema()
    assert torch.equal(opt.ema, flat.flat_param)
    opt._averaging = True          # what averaged().__enter__ sets after the exchange (which needs the GPU)
    for call in (opt.step, opt.reset_ema, lambda: opt.load_state_dict(saved)):
        with pytest.raises(RuntimeError, match="inside averaged"):
            call()
    assert opt.state_dict()["ema"] is flat.flat_param          # inside the context the two buffers have changed places
    opt._averaging = False
    wrapped = DeviceNoamOptimizer(FusedAdam(_FakeFlat(), noam=(0.2, 4000), ema_decay=0.9999))
    wrapped.optimizer.flat.flat_param.add_(1.0)
    wrapped.reset_ema()
    assert torch.equal(wrapped.optimizer.ema, wrapped.optimizer.flat.flat_param)
    assert wrapped.averaged().opt is wrapped.optimizer and callable(wrapped.swap_ema)


def test_checkpoint_carries_the_average(tmp_path):
    from sbl_for_multilingual_lip_reading_amd import checkpoint
    from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import DeviceNoamOptimizer, FusedAdam
    opt = DeviceNoamOptimizer(FusedAdam(_FakeFlat(), noam=(0.5, 2), ema_decay=0.99))
    opt.optimizer.ema.mul_(-2.0)
    opt.step_num = 3
    model = opt.optimizer.flat.model
    checkpoint.save_checkpoint(tmp_path / "ck.pt", model, opt, epoch=2)
    ck = torch.load(tmp_path / "ck.pt", weights_only=True)
    assert ck["optimizer_state"]["ema_decay"] == 0.99 and torch.equal(ck["optimizer_state"]["ema"], opt.optimizer.ema)
    opt2 = DeviceNoamOptimizer(FusedAdam(_FakeFlat(), noam=(0.5, 2), ema_decay=0.99))
    checkpoint.load_checkpoint(tmp_path / "ck.pt", opt2.optimizer.flat.model, opt2)
    assert opt2.step_num == 3 and torch.equal(opt2.optimizer.ema, opt.optimizer.ema)
    # averaged=True needs an optimizer that averages
    with pytest.raises(ValueError, match="ema_decay"):
        checkpoint.save_checkpoint(tmp_path / "no.pt", model, DeviceNoamOptimizer(FusedAdam(_FakeFlat(), noam=(0.5, 2))), averaged=True)
    with pytest.raises(ValueError, match="ema_decay"):
        checkpoint.save_checkpoint(tmp_path / "no.pt", model, None, averaged=True)
