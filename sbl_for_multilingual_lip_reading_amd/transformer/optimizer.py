"""TransformerOptimizer (the reference's transformer/optimizer.py surface), FusedAdam and DeviceNoamOptimizer."""
import math

_SCHEDULE_D_MODEL = 512      # the schedule's model width is fixed, whatever the model's


class TransformerOptimizer(object):
    """Drives a torch-style optimizer with the Noam schedule: step n (counted from 1) runs at
    lr = k / sqrt(512) * min(1 / sqrt(n), n / warmup_steps^1.5), i.e. a linear warm-up that turns into 1/sqrt(n)
    decay at n = warmup_steps.  The rate is written into every param group just before the wrapped step."""

    def __init__(self, optimizer, warmup_steps=4000, k=0.2):
        self.optimizer = optimizer
        self.k = k
        self.warmup_steps = warmup_steps
        self.init_lr = _SCHEDULE_D_MODEL ** -0.5
        self.lr, self.step_num = self.init_lr, 0

    def zero_grad(self):
        return self.optimizer.zero_grad()

    def step(self):
        self._update_lr()
        return self.optimizer.step()

    def _update_lr(self):
        n = self.step_num = self.step_num + 1
        self.lr = self.k * self.init_lr * min(n ** -0.5, n * self.warmup_steps ** -1.5)
        for group in self.optimizer.param_groups:
            group["lr"] = self.lr


class FusedAdam(object):
    """torch.optim.Adam(betas=(0.9, 0.98), eps=1e-9) as SBL/train.py:75 configures it, as ONE kernel launch over the
    flat parameter / gradient buffers of a dp.FlatModel (81 M parameters: 2.3 GB of traffic per step instead of 475
    per-tensor launches).  Duck-types the slice of the torch optimizer API that TransformerOptimizer and the
    reference's train loop use: param_groups[...]['lr'], zero_grad(), step(), state_dict()/load_state_dict().
    grad_scale folds the 1/world_size of data-parallel averaging into the update when the exchange sums.

    DEVICE MODE (any of max_grad_norm, clip_value, skip_nonfinite, noam set; all off by default).  The numbers the update
    needs live in a double[8] device buffer (include/sbl_hip.h, SBL_OPT_*): step() launches sbl_grad_sumsq per trainable
    range, one sbl_opt_finalize and sbl_adam_step_dev per range, with no allocation, no read-back and - with `noam` - no
    host-to-device copy, so it can be captured by torch.cuda.graph together with flat.zero_grad(), forward and backward.
      max_grad_norm   global L2-norm clip, torch.nn.utils.clip_grad_norm_'s rule, over the trainable ranges
      clip_value      element clamp to +-clip_value before the norm (the reference's clip_gradient, SBL/utils.py:10-19);
                      like torch.clamp it turns +-inf into +-clip_value and keeps NaN
      skip_nonfinite  a gradient with an inf / NaN element (after the clamp) leaves parameters, moments, step count and
                      rate untouched and counts as skipped
      noam            (k, warmup_steps): the Noam rate is computed on the device from the applied-step count.  Without
                      it the rate is param_groups[0]['lr'], uploaded when it changed since the last step (a host-to-
                      device copy: that variant is for eager use)
    In data-parallel mode nothing else is needed: step() runs after GradientExchange.finish() on the summed gradient and
    grad_scale applies before the norm.  The kernels sum in an order fixed by the range lengths alone (no atomics), so
    replicas holding the same gradient derive bit-identical coefficients and stay in step.

    WEIGHT AVERAGING (ema_decay in (0, 1); turns device mode on).  `ema` is a second flat buffer, a clone of the parameters
    at construction, and the update launch (sbl_adam_ema_step_dev in place of sbl_adam_step_dev) also does
    ema += (1 - d_t) * (p_new - ema), d_t = min(ema_decay, (1 + t) / (10 + t)) with ema_warmup (t: applied steps), else
    ema_decay: one more read and write in the pass that already streams p, g, m, v.  A skipped step and a frozen range
    leave it alone, so frozen parameters keep ema == p.  `with opt.averaged(): model.validate(...)` evaluates the averaged
    weights; swap_ema() is the exchange it is made of; reset_ema() restarts the average from weights loaded by hand.  The
    average travels in state_dict() as `ema` / `ema_decay`."""

    def __init__(self, flat, lr=1e-3, betas=(0.9, 0.98), eps=1e-9, grad_scale=1.0, max_grad_norm=None, clip_value=None,
                 skip_nonfinite=False, noam=None, ema_decay=None, ema_warmup=True):
        import torch
        from ._env import ops
        if ema_decay is not None and not 0.0 < float(ema_decay) < 1.0:
            raise ValueError("ema_decay must lie in (0, 1), got %r" % (ema_decay,))
        self._ops = ops
        self.flat = flat
        self.param_groups = [{"params": list(flat.model.parameters()), "lr": lr, "betas": betas, "eps": eps}]
        self.exp_avg = torch.zeros_like(flat.flat_param)
        self.exp_avg_sq = torch.zeros_like(flat.flat_param)
        self.step_count = 0
        self.grad_scale = grad_scale
        self.max_grad_norm = float(max_grad_norm) if max_grad_norm else 0.0
        self.clip_value = float(clip_value) if clip_value else 0.0
        self.skip_nonfinite = bool(skip_nonfinite)
        self.noam = (float(noam[0]), float(noam[1])) if noam is not None else None
        self.ema_decay = float(ema_decay) if ema_decay is not None else None
        self.ema_warmup = bool(ema_warmup)
        self.ema = flat.flat_param.clone() if self.ema_decay is not None else None
        self._averaging = False          # inside averaged(): the flat parameters hold the average, `ema` the live weights
        self.device_mode = bool(self.max_grad_norm or self.clip_value or self.skip_nonfinite or self.noam is not None
                                or self.ema_decay is not None)
        if self.device_mode:
            if self.max_grad_norm < 0 or self.clip_value < 0 or (self.noam and min(self.noam) <= 0):
                raise ValueError("max_grad_norm, clip_value, and noam's k and warmup_steps must be positive")
            dev = flat.flat_param.device
            self.opt_state = torch.zeros(ops.OPT_STATE_SLOTS, device=dev, dtype=torch.float64)
            # enough for any set of trainable ranges: sum over ranges of min(cap, ceil(n_r / 1024)) <= numel / 1024 + ranges
            self._partials = torch.zeros(flat.numel // 1024 + len(flat.slots) + 1, device=dev, dtype=torch.float64)
            self._staging = torch.zeros(ops.OPT_STATE_SLOTS, dtype=torch.float64)
            self._lr_uploaded = None
            self._write_state(0)

    # ---- device mode: host <-> state buffer (each of these synchronises or copies; none is called by step() under `noam`)
    def _host_slots(self, t, lr=None):
        """The slots sbl_opt_finalize derives from the applied-step count t, in the same double arithmetic."""
        b1, b2 = (float(_f32(b)) for b in self.param_groups[0]["betas"])
        if self.noam is not None and t >= 1:
            k, warmup = self.noam
            lr = k * _SCHEDULE_D_MODEL ** -0.5 * min(t ** -0.5, t * warmup ** -1.5)
        elif lr is None:
            lr = float(self.opt_state[self._ops.OPT_LR].item())
        if t < 1:
            return lr, 0.0, 0.0
        return lr, lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t)

    def _write_state(self, t, lr=None):
        o = self._ops
        if lr is None and self.noam is None:
            lr = float(_f32(self.param_groups[0]["lr"]))
            self._lr_uploaded = self.param_groups[0]["lr"]
        lr, step_size, inv_sqrt_bc2 = self._host_slots(int(t), lr)
        s = self.opt_state.cpu()
        s[o.OPT_STEP], s[o.OPT_LR], s[o.OPT_STEP_SIZE], s[o.OPT_INV_SQRT_BC2] = float(int(t)), lr, step_size, inv_sqrt_bc2
        self.opt_state.copy_(s)

    def _read_state(self, slot):
        if not self.device_mode:
            raise RuntimeError("FusedAdam: the device state exists only in device mode (max_grad_norm, clip_value, "
                               "skip_nonfinite or noam set)")
        return float(self.opt_state[slot].item())

    @property
    def last_grad_norm(self):
        """L2 norm of the last step's clamped, scaled gradient (reads the device: for logging every N steps)."""
        return self._read_state(self._ops.OPT_GRAD_NORM)

    @property
    def last_clip_coef(self):
        return self._read_state(self._ops.OPT_CLIP_COEF)

    @property
    def steps_applied(self):
        return int(self._read_state(self._ops.OPT_STEP))

    @property
    def steps_skipped(self):
        return int(self._read_state(self._ops.OPT_SKIPPED))

    @property
    def device_lr(self):
        return self._read_state(self._ops.OPT_LR)

    def set_steps_applied(self, t):
        """Set the applied-step count (resume); rate and bias corrections follow from it."""
        self._write_state(t)

    def zero_grad(self, set_to_none=False):
        self.flat.zero_grad()

    def step(self):
        """One launch per maximal run of trainable parameters (one launch in all when nothing is frozen): like
        Adam(filter(lambda p: p.requires_grad, model.parameters())) in SBL/train.py:75, frozen parameters and their
        moments are left untouched."""
        g = self.param_groups[0]
        if self._averaging:
            raise RuntimeError("FusedAdam.step() inside averaged(): the parameters hold the averaged weights")
        if self.device_mode:
            return self._step_device(g)
        self.step_count += 1
        for a, b in self.flat.trainable_ranges():
            self._ops.adam_step(self.flat.flat_param[a:b], self.flat.flat_grad[a:b], self.exp_avg[a:b], self.exp_avg_sq[a:b],
                                g["lr"], g["betas"][0], g["betas"][1], g["eps"], self.step_count, self.grad_scale)
        # the kernel wrote the weights behind torch's back: re-pack the cached convolution weight images in place
        self._ops.refresh_packed_weights()

    def _step_device(self, g):
        o, f = self._ops, self.flat
        if self.noam is None and g["lr"] != self._lr_uploaded:
            # the rate as sbl_adam_step would receive it (a float); the only host-to-device copy of a step, eager use only
            self._staging[0] = float(_f32(g["lr"]))
            self.opt_state[o.OPT_LR:o.OPT_LR + 1].copy_(self._staging[:1])
            self._lr_uploaded = g["lr"]
        ranges = f.trainable_ranges()
        nparts = 0
        for a, b in ranges:
            nparts += o.grad_sumsq(f.flat_grad[a:b], self._partials, nparts, self.grad_scale, self.clip_value)
        if not ranges:
            return
        o.opt_finalize(self.opt_state, self._partials, nparts, self.max_grad_norm, self.skip_nonfinite, self.noam,
                       g["betas"][0], g["betas"][1])
        for a, b in ranges:
            if self.ema is not None:
                o.adam_ema_step_dev(f.flat_param[a:b], f.flat_grad[a:b], self.exp_avg[a:b], self.exp_avg_sq[a:b], self.ema[a:b],
                                    self.opt_state, g["betas"][0], g["betas"][1], g["eps"], self.grad_scale, self.clip_value,
                                    self.ema_decay, self.ema_warmup)
            else:
                o.adam_step_dev(f.flat_param[a:b], f.flat_grad[a:b], self.exp_avg[a:b], self.exp_avg_sq[a:b], self.opt_state,
                                g["betas"][0], g["betas"][1], g["eps"], self.grad_scale, self.clip_value)
        o.refresh_packed_weights()

    # ---- weight averaging
    def _need_ema(self):
        if self.ema is None:
            raise RuntimeError("FusedAdam: no weight average is kept (build the optimizer with ema_decay)")

    def reset_ema(self):
        """Restart the average from the current weights (after weights were loaded by hand)."""
        self._need_ema()
        if self._averaging:
            raise RuntimeError("FusedAdam.reset_ema() inside averaged()")
        self.ema.copy_(self.flat.flat_param)

    def swap_ema(self):
        """Exchange live and averaged weights in place over the trainable ranges (frozen ranges hold ema == p), exactly,
        then re-pack the cached convolution weight images: one sbl_swap_f32 per range, no allocation and no read-back, so
        it can be captured.  Twice is the identity."""
        self._need_ema()
        for a, b in self.flat.trainable_ranges():
            self._ops.swap_(self.flat.flat_param[a:b], self.ema[a:b])
        self._ops.refresh_packed_weights()

    def averaged(self):
        """Context manager: inside it the model's parameters are the averaged ones, so Transformer.validate, recognize*,
        checkpoint.save_checkpoint and the model's state_dict() see them; the live weights come back on exit, also when the
        body raises.  BatchNorm running statistics are buffers, not parameters: they are NOT averaged, the live ones are
        used.  step() inside the context raises.  Entry and exit are one swap_ema() each (capturable)."""
        self._need_ema()
        return _Averaged(self)

    def state_dict(self):
        if self.device_mode:
            sd = {"step": self.steps_applied, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq,
                  "lr": self.param_groups[0]["lr"], "opt_state": self.opt_state}
            if self.ema is not None:
                # inside averaged() the two buffers have changed places (frozen ranges are equal in both)
                sd["ema"] = self.flat.flat_param if self._averaging else self.ema
                sd["ema_decay"] = self.ema_decay
            return sd
        return {"step": self.step_count, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq,
                "lr": self.param_groups[0]["lr"]}

    def load_state_dict(self, sd):
        if self._averaging:
            raise RuntimeError("FusedAdam.load_state_dict() inside averaged()")
        self.step_count = int(sd["step"])
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.param_groups[0]["lr"] = sd["lr"]
        if self.device_mode:
            if sd.get("opt_state") is not None:
                self.opt_state.copy_(sd["opt_state"])
                self._lr_uploaded = None          # the next eager step uploads param_groups' rate again
            else:                                 # a default-mode checkpoint: only the step count is known
                self._write_state(self.step_count)
        if self.ema is not None:                  # a stored average is ignored when this optimizer keeps none
            if sd.get("ema") is not None:
                self.ema.copy_(sd["ema"])
            else:                                 # no average in the checkpoint: start it from the weights as loaded
                self.ema.copy_(self.flat.flat_param)      # (checkpoint.load_checkpoint loads the model first)


class _Averaged(object):
    """FusedAdam.averaged(): swap_ema() on entry and on exit."""

    def __init__(self, opt):
        self.opt = opt

    def __enter__(self):
        if self.opt._averaging:
            raise RuntimeError("FusedAdam.averaged() does not nest")
        self.opt.swap_ema()
        self.opt._averaging = True
        return self.opt

    def __exit__(self, *exc):
        self.opt._averaging = False
        self.opt.swap_ema()
        return False


def _f32(x):
    """x rounded to float32: what a float argument of the C ABI receives."""
    import struct
    return struct.unpack("f", struct.pack("f", float(x)))[0]


class DeviceNoamOptimizer(object):
    """TransformerOptimizer's surface (zero_grad, step, lr, step_num, _update_lr, .optimizer) over a device-mode
    FusedAdam(noam=(k, warmup_steps)): the step count and the rate live in the optimizer's device state, step() touches
    the host for nothing, and a whole training step can be captured as one graph.  `lr` and `step_num` read the device
    (they synchronise: for logging and checkpoints); assigning `step_num` (checkpoint.load_checkpoint does) and
    _update_lr() write it.  Skipped steps (skip_nonfinite) do not advance step_num."""

    def __init__(self, optimizer):
        if not getattr(optimizer, "device_mode", False) or optimizer.noam is None:
            raise ValueError("DeviceNoamOptimizer needs a FusedAdam built with noam=(k, warmup_steps)")
        self.optimizer = optimizer
        self.k, self.warmup_steps = optimizer.noam
        self.init_lr = _SCHEDULE_D_MODEL ** -0.5

    def zero_grad(self):
        return self.optimizer.zero_grad()

    def step(self):
        return self.optimizer.step()

    def swap_ema(self):
        return self.optimizer.swap_ema()

    def averaged(self):
        return self.optimizer.averaged()

    def reset_ema(self):
        return self.optimizer.reset_ema()

    @property
    def lr(self):
        return self.optimizer.device_lr if self.step_num else self.init_lr

    @property
    def step_num(self):
        return self.optimizer.steps_applied

    @step_num.setter
    def step_num(self, n):
        self.optimizer.set_steps_applied(int(n))

    def _update_lr(self):
        """Advance the counter by one and refresh the rate without an update: the reference calls this once after loading
        a checkpoint (SBL/train.py:109), and TransformerOptimizer has the same quirk."""
        self.step_num = self.step_num + 1
