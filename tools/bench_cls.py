"""Stage-1 classification pre-training step (ClassifierTransformer, 3 encoder layers, T = 31 frames of 88x88) with
cal_cls_loss, backward and the FusedAdam step over dp.FlatModel, per clips-per-GPU and precision mode; and the
classification head alone (forward + loss + backward of the sbl_cls_* kernels) against the same head built from existing
ops (avgpool + linear + smoothed_ce, the two losses added by torch).
Usage: python tools/bench_cls.py [--steps K] [--warmup W] [--batches 32,100] [--modes f32,bf16x6] [--json PATH]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from sbl_for_multilingual_lip_reading_amd import detfill, dp, ops
from sbl_for_multilingual_lip_reading_amd.transformer.classifier import ClassifierTransformer, cal_cls_loss
from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import FusedAdam, TransformerOptimizer

DEV = "cuda:0"
T, H, W = 31, 88, 88


def timed(fn, n, warmup):
    """Mean ms per call over n calls after warmup, device events around the window."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def step_time(N, steps, warmup):
    torch.manual_seed(0)
    m = ClassifierTransformer(Encoder(512, 3, 8, 64, 64, 512, 2048), None).to(DEV).train()
    flat = dp.FlatModel(m)
    opt = TransformerOptimizer(FusedAdam(flat))
    x = torch.from_numpy(detfill.synthetic_batch(N, T, H, W, 3)[0]).to(DEV)
    g = torch.Generator().manual_seed(1)
    t1, t2 = torch.randint(0, 1500, (N,), generator=g).to(DEV), torch.randint(0, 2, (N,), generator=g).to(DEV)
    last = {}

    def step():
        opt.zero_grad()
        v, lang = m(x)
        loss, stats = cal_cls_loss(v, lang, t1, t2)
        loss.backward()
        opt.step()
        last["loss"] = loss

    ms = timed(step, steps, warmup)
    return ms, float(last["loss"])


def head_times(N, n=50, warmup=5):
    g = torch.Generator().manual_seed(2)
    enc = torch.randn(N, T, 512, generator=g).to(DEV).requires_grad_(True)
    w1 = (torch.randn(1500, 512, generator=g) * 0.05).to(DEV).requires_grad_(True)
    b1 = torch.zeros(1500, device=DEV, requires_grad=True)
    w2 = (torch.randn(2, 512, generator=g) * 0.05).to(DEV).requires_grad_(True)
    b2 = torch.zeros(2, device=DEV, requires_grad=True)
    t1, t2 = torch.randint(0, 1500, (N,), generator=g).to(DEV), torch.randint(0, 2, (N,), generator=g).to(DEV)

    def fused():
        l1, l2 = ops.ClsHeadFn.apply(enc, w1, b1, w2, b2, T - 1)
        loss, _ = ops.ClsLossFn.apply(l1, l2, t1, t2, 0.1, -100)
        loss.backward()

    def existing():
        pooled = ops.AvgPoolFn.apply(enc.view(N, T, 1, 512))
        l1 = ops.linear(pooled, w1, b1)
        l2 = ops.linear(enc[:, T - 1], w2, b2)
        loss = ops.SmoothedCEFn.apply(l1, t1, 0.0, -100)[0] + 0.1 * ops.SmoothedCEFn.apply(l2, t2, 0.0, -100)[0]
        loss.backward()

    return timed(fused, n, warmup) * 1e3, timed(existing, n, warmup) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="32,100")
    ap.add_argument("--modes", default="f32,bf16x6")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for mode in a.modes.split(","):
        ops.set_matmul_precision(mode)
        for N in (int(v) for v in a.batches.split(",")):
            ms, loss = step_time(N, a.steps, a.warmup)
            head_us, old_us = head_times(N)
            r = {"mode": mode, "clips_per_gpu": N, "step_ms": round(ms, 3), "clips_per_s": round(N / ms * 1e3, 1),
                 "head_fwd_loss_bwd_us": round(head_us, 1), "head_existing_ops_us": round(old_us, 1), "loss": round(loss, 4)}
            rows.append(r)
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()
    ops.set_matmul_precision("f32")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
