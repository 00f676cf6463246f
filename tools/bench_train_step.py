#!/usr/bin/env python3
"""Times the optimizer update and the whole training step of the SBL model (6+6 layers, B = 32 clips of 29 x 88 x 88,
bf16x6 by default) and prints one JSON line:

  (a) adam_us            sbl_adam_step alone over the flat buffers (the host-scalar update of default FusedAdam)
  (b) device_update_us   sbl_grad_sumsq + sbl_opt_finalize + sbl_adam_step_dev alone (the device-mode update)
      each with the bytes the algorithm moves (7 resp. 8 fp32 accesses per element) and that over --peak-tbs TB/s
  (c) eager_default_ms   zero_grad, forward, loss, backward, TransformerOptimizer(FusedAdam(default)).step(), issued eagerly
  (d) eager_device_ms    the same step with DeviceNoamOptimizer(FusedAdam(max_grad_norm, skip_nonfinite, noam))
  (e) graph_device_ms    step (d) captured once as one hipGraph and replayed
  (f) update_plain_us    (b) again, in the group of the two below
  (g) update_ema_us      the update with the weight average in the same launch (sbl_adam_ema_step_dev in place of sbl_adam_step_dev)
  (h) update_lerp_us     (b) followed by torch.Tensor.lerp_ of the average over the same ranges (the unfused alternative)
      8, 10 and 11 fp32 accesses per element
  (i) swap_ema_us        FusedAdam.swap_ema(): sbl_swap_f32 over the trainable ranges + the weight re-pack

Every figure is the median over --rounds windows of --steps calls (device events around each window, after --warmup calls);
the variants of a group alternate inside each round, and *_spread is (max - min) / median over the rounds.

    python tools/bench_train_step.py --steps 10 --warmup 3 --rounds 5
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def alternate(fns, steps, warmup, rounds):
    """{name: (median ms per call, spread)}; the variants take turns inside every round."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(window(fn, steps))
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in ms.items()}


def build_model(dev, layers):
    """The model of bench.py: reference defaults (SBL/utils.py:90-114), deterministic weights, dropout on, train mode."""
    from sbl_for_multilingual_lip_reading_amd import detfill
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    from sbl_for_multilingual_lip_reading_amd.transformer.transformer import Transformer
    enc = Encoder(512, layers, 8, 64, 64, 512, 2048, dropout=0.1, pe_maxlen=5000)
    dec = Decoder(0, 1, 58, 512, layers, 8, 64, 64, 512, 2048, dropout=0.1, tgt_emb_prj_weight_sharing=True, pe_maxlen=5000)
    m = Transformer(enc, dec, None)
    sd = m.state_dict()
    m.load_state_dict({k: (v if k.endswith(".pe") else torch.from_numpy(detfill.fill_value(k, tuple(v.shape)).copy()))
                       for k, v in sd.items()})
    return m.to(dev).train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=29)
    ap.add_argument("--size", type=int, default=88)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--update-reps", type=int, default=50, help="calls per window of the update-only timings (a), (b)")
    ap.add_argument("--ema-decay", type=float, default=0.9999, help="decay of the weight average in (f), (h) and the exchange")
    ap.add_argument("--precision", default="bf16x6")
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM peak the byte rates are quoted against")
    args = ap.parse_args()

    from sbl_for_multilingual_lip_reading_amd import detfill, dp, ops
    from sbl_for_multilingual_lip_reading_amd.transformer.loss import cal_performance_device
    from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import DeviceNoamOptimizer, FusedAdam, TransformerOptimizer
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_step: needs the GPU (there is no CPU path)")
    ops.set_matmul_precision(args.precision)
    dev = "cuda:0"
    B = args.batch
    model = build_model(dev, args.layers)
    flat = dp.FlatModel(model)
    x_np, l2r_np, r2l_np = detfill.synthetic_batch(B, args.frames, args.size, args.size, 7)
    x, l2r, r2l = torch.from_numpy(x_np).to(dev), torch.from_numpy(l2r_np).to(dev), torch.from_numpy(r2l_np).to(dev)
    model.decoder.coins_host = [i % 2 == 1 for i in range(16)]      # 8 own-argmax coins: the expectation of decoder.py:176
    drop = ops.dropout_state(dev)
    opt_default = TransformerOptimizer(FusedAdam(flat))
    opt_device = DeviceNoamOptimizer(FusedAdam(flat, max_grad_norm=5.0, skip_nonfinite=True, noam=(0.2, 4000)))
    loss_out = torch.zeros((), device=dev)
    n = flat.numel
    out = {"tool": "bench_train_step", "batch": B, "frames": args.frames, "size": args.size, "layers": args.layers,
           "precision": args.precision, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "flat_elements": n, "trainable_ranges": len(flat.trainable_ranges())}

    def train_step(opt):
        drop.begin_step()
        opt.zero_grad()
        pl, gl, pr, gr = model(x, l2r, r2l)
        loss = 0.5 * (cal_performance_device(pl, gl, 0.1)[0] + cal_performance_device(pr, gr, 0.1)[0])
        loss.backward()
        ops.join_side_streams()
        opt.step()
        loss_out.copy_(loss.detach())

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        # ---- (c), (d): eager steps (also the warm-up of the capture stream); they leave a real gradient in flat.flat_grad
        r = alternate({"eager_default": lambda: train_step(opt_default), "eager_device": lambda: train_step(opt_device)},
                      args.steps, args.warmup, args.rounds)
        # ---- (e): the same device-mode step as one graph
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            train_step(opt_device)
        r.update(alternate({"eager_device_again": lambda: train_step(opt_device), "graph_device": graph.replay},
                           args.steps, args.warmup, args.rounds))
        for k, (ms, spread) in r.items():
            out[k + "_ms"], out[k + "_spread"] = round(ms, 3), round(spread, 4)
        out["loss"] = round(float(loss_out), 4)
        out["steps_applied"], out["steps_skipped"] = opt_device.optimizer.steps_applied, opt_device.optimizer.steps_skipped
        out["last_grad_norm"], out["last_clip_coef"] = opt_device.optimizer.last_grad_norm, opt_device.optimizer.last_clip_coef

        # ---- (a), (b): the update alone, on the gradient the last step left, without the weight re-pack both steps share
        fa, fd = opt_default.optimizer, opt_device.optimizer
        ranges = flat.trainable_ranges()
        count = [0]

        def adam_host():
            count[0] += 1
            for a, b in ranges:
                ops.adam_step(flat.flat_param[a:b], flat.flat_grad[a:b], fa.exp_avg[a:b], fa.exp_avg_sq[a:b], 1e-4, 0.9, 0.98, 1e-9,
                              count[0], 1.0)

        def update_device():
            nparts = 0
            for a, b in ranges:
                nparts += ops.grad_sumsq(flat.flat_grad[a:b], fd._partials, nparts, 1.0, 0.0)
            ops.opt_finalize(fd.opt_state, fd._partials, nparts, fd.max_grad_norm, True, fd.noam, 0.9, 0.98)
            for a, b in ranges:
                ops.adam_step_dev(flat.flat_param[a:b], flat.flat_grad[a:b], fd.exp_avg[a:b], fd.exp_avg_sq[a:b], fd.opt_state,
                                  0.9, 0.98, 1e-9, 1.0, 0.0)

        def sumsq_only():
            nparts = 0
            for a, b in ranges:
                nparts += ops.grad_sumsq(flat.flat_grad[a:b], fd._partials, nparts, 1.0, 0.0)
            ops.opt_finalize(fd.opt_state, fd._partials, nparts, fd.max_grad_norm, True, fd.noam, 0.9, 0.98)

        u = alternate({"adam": adam_host, "device_update": update_device, "sumsq_finalize": sumsq_only}, args.update_reps, 5,
                      args.rounds)

        # ---- (f), (g), (h): the update with and without the weight average, and the average as a pass of its own
        fe = FusedAdam(flat, max_grad_norm=5.0, skip_nonfinite=True, noam=(0.2, 4000), ema_decay=args.ema_decay)
        lerp_w = 1.0 - args.ema_decay

        def update_ema():
            nparts = 0
            for a, b in ranges:
                nparts += ops.grad_sumsq(flat.flat_grad[a:b], fe._partials, nparts, 1.0, 0.0)
            ops.opt_finalize(fe.opt_state, fe._partials, nparts, fe.max_grad_norm, True, fe.noam, 0.9, 0.98)
            for a, b in ranges:
                ops.adam_ema_step_dev(flat.flat_param[a:b], flat.flat_grad[a:b], fe.exp_avg[a:b], fe.exp_avg_sq[a:b], fe.ema[a:b],
                                      fe.opt_state, 0.9, 0.98, 1e-9, 1.0, 0.0, fe.ema_decay, fe.ema_warmup)

        def update_then_lerp():
            update_device()
            for a, b in ranges:
                fe.ema[a:b].lerp_(flat.flat_param[a:b], lerp_w)

        def swap_and_repack():
            fe.swap_ema()

        e = alternate({"update_plain": update_device, "update_ema": update_ema, "update_lerp": update_then_lerp},
                      args.update_reps, 5, args.rounds)
        # an even number of exchanges per window and in the warm-up: the weights end where they started
        e.update(alternate({"swap_ema": swap_and_repack}, args.update_reps // 2 * 2, 4, args.rounds))
    for k, acc in (("adam", 7), ("device_update", 8), ("sumsq_finalize", 1)):
        ms, spread = u[k]
        nbytes = acc * 4 * n
        out[k + "_us"], out[k + "_spread"], out[k + "_bytes"] = round(ms * 1e3, 1), round(spread, 4), nbytes
        out[k + "_frac_of_peak"] = round(nbytes / (ms * 1e-3) / (args.peak_tbs * 1e12), 4)
    # 8 accesses per element without the average, 10 with it in the update launch, 8 + 3 with torch's lerp_ after the update;
    # the exchange moves 4 (the weight re-pack it ends with is not counted in its bytes)
    for k, acc in (("update_plain", 8), ("update_ema", 10), ("update_lerp", 11), ("swap_ema", 4)):
        ms, spread = e[k]
        nbytes = acc * 4 * n
        out[k + "_us"], out[k + "_spread"], out[k + "_bytes"] = round(ms * 1e3, 1), round(spread, 4), nbytes
        out[k + "_frac_of_peak"] = round(nbytes / (ms * 1e-3) / (args.peak_tbs * 1e12), 4)
    out["ema_decay"] = args.ema_decay
    out["ema_over_plain_time"], out["ema_over_plain_bytes"] = round(e["update_ema"][0] / e["update_plain"][0], 4), round(10 / 8, 4)
    out["ema_over_lerp_time"], out["ema_over_lerp_bytes"] = round(e["update_ema"][0] / e["update_lerp"][0], 4), round(10 / 11, 4)
    out["device_over_adam_time"] = round(u["device_update"][0] / u["adam"][0], 4)
    out["device_over_adam_bytes"] = round(8 / 7, 4)
    out["graph_over_eager_device"] = round(r["graph_device"][0] / r["eager_device_again"][0], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
