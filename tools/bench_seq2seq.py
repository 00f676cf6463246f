#!/usr/bin/env python3
"""Times the single-direction seq2seq model (transformer/seq2seq.py) at the reference's LRW shapes, B = 32, T = 29, 88x88:
one training step (forward, loss, backward, FusedAdam over the flat buffers) and the greedy decode three ways - KV-cached
under one hipGraph, KV-cached eager, prefix-recompute eager.  Prints one JSON line (milliseconds, median of --steps runs
after --warmup runs, timed with device events on one stream).

    python tools/bench_seq2seq.py --steps 20 --warmup 5
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=29)
    ap.add_argument("--size", type=int, default=88)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--vocab", type=int, default=42)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="bf16x6")
    args = ap.parse_args()

    from sbl_for_multilingual_lip_reading_amd import dp, ops
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    from sbl_for_multilingual_lip_reading_amd.transformer.loss import cal_performance_device
    from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import FusedAdam
    from sbl_for_multilingual_lip_reading_amd.transformer.seq2seq import Seq2SeqDecoder, Seq2SeqTransformer
    ops.set_matmul_precision(args.precision)
    torch.manual_seed(0)
    dev = "cuda:0"
    B, T, S, V = args.batch, args.frames, args.size, args.vocab
    model = Seq2SeqTransformer(Encoder(512, args.layers, 8, 64, 64, 512, 2048),
                               Seq2SeqDecoder(0, 1, V, 512, args.layers, 8, 64, 64, 512, 2048)).to(dev)
    x = torch.randn(B, T, S, S, device=dev)
    tgt = torch.randint(2, V, (B, 13), device=dev)
    tgt[torch.arange(13, device=dev).unsqueeze(0) >= torch.randint(1, 14, (B, 1), device=dev)] = -1
    out = {"tool": "bench_seq2seq", "batch": B, "frames": T, "size": S, "layers": args.layers, "vocab": V,
           "precision": args.precision, "steps": args.steps, "warmup": args.warmup}

    model.eval()
    with torch.no_grad():
        ys_eager = model.recognize(x)
        out["recognize_cached_eager_ms"], _ = timed(lambda: model.recognize(x), args.steps, args.warmup)
        out["recognize_recompute_eager_ms"], _ = timed(lambda: model.recognize(x, cached=False), args.steps, args.warmup)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            model.recognize(x)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ys_graph = model.recognize(x)
        out["recognize_cached_graph_ms"], _ = timed(graph.replay, args.steps, args.warmup)
    # the frontend's always-on dropout draws a new mask per call, so tokens are compared only when it is off
    out["frontend_dropout_p"] = float(model.lipreading.frontend_dropout_p)
    del graph, ys_graph, ys_eager

    model.train()
    flat = dp.FlatModel(model)
    opt = FusedAdam(flat, lr=1e-4)

    def step():
        flat.zero_grad()
        pred, gold = model(x, tgt)
        cal_performance_device(pred, gold, 0.1)[0].backward()
        opt.step()

    out["train_step_ms"], out["train_step_min_ms"] = timed(step, args.steps, args.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
