#!/usr/bin/env python3
"""Times the decoder of the single-direction seq2seq model (transformer/seq2seq.py) at the LRW1000 shapes, B = 32 clips,
T = 29 encoder frames = decode steps, 6 decoder layers, 48 classes, on a fixed encoder output: the KV-cached greedy decode
under one hipGraph, and the batched beam search (Seq2SeqDecoder.beam_search) with W = 1, 5 and 8, eager and under one
hipGraph.  Prints one JSON line: milliseconds per call (median of --steps runs after --warmup runs, device events on one
stream), milliseconds per decode step, the ratio to the greedy decode, and whether a W = 8 step is no slower than eight
W = 1 steps.

    python tools/bench_beam.py --steps 20 --warmup 5
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_seq2seq import timed  # noqa: E402


def graphed(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        keep = fn()
    return graph, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=29)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--vocab", type=int, default=48)
    ap.add_argument("--beams", type=int, nargs="*", default=[1, 5, 8])
    ap.add_argument("--nbest", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="bf16x6")
    args = ap.parse_args()

    from sbl_for_multilingual_lip_reading_amd import ops
    from sbl_for_multilingual_lip_reading_amd.transformer.seq2seq import Seq2SeqDecoder
    ops.set_matmul_precision(args.precision)
    torch.manual_seed(0)
    dev = "cuda:0"
    B, T, V = args.batch, args.frames, args.vocab
    dec = Seq2SeqDecoder(0, 1, V, 512, args.layers, 8, 64, 64, 512, 2048).to(dev).eval()
    enc = torch.randn(B, T, 512, device=dev)
    prior = torch.log_softmax(torch.randn(V, V, device=dev) * 3, dim=1)
    out = {"tool": "bench_beam", "batch": B, "frames": T, "layers": args.layers, "vocab": V, "nbest": args.nbest,
           "precision": args.precision, "steps": args.steps, "warmup": args.warmup}
    with torch.no_grad():
        graph, keep = graphed(lambda: dec.recognize_beam(enc))
        greedy, _ = timed(graph.replay, args.steps, args.warmup)
        out["greedy_cached_graph_ms"] = greedy
        del graph, keep
        for W in args.beams:
            run = lambda: dec.beam_search(enc, W, args.nbest, 0, prior)      # noqa: E731
            eager, _ = timed(run, args.steps, args.warmup)
            graph, keep = graphed(run)
            rep, _ = timed(graph.replay, args.steps, args.warmup)
            out["beam%d_eager_ms" % W], out["beam%d_graph_ms" % W] = eager, rep
            out["beam%d_graph_ms_per_step" % W] = rep / T
            out["beam%d_graph_over_greedy" % W] = rep / greedy
            del graph, keep
    if 1 in args.beams and 8 in args.beams:
        out["beam8_step_not_slower_than_8_beam1_steps"] = bool(out["beam8_graph_ms"] <= 8 * out["beam1_graph_ms"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
