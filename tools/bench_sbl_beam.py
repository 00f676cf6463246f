#!/usr/bin/env python3
"""Times the bidirectional SBL decoder (transformer/decoder.py) alone at the model's shapes, B = 32 clips, T = 29 encoder
frames, 6 + 6 decoder layers, 16 decode steps, on a fixed encoder output: the greedy decode (Decoder.recognize_beam) under
one hipGraph, and the beam search over pairs (Decoder.beam_search) with W = 1, 3 and 5, eager and under one hipGraph, all in
the same run.  Prints one JSON line: milliseconds per call (median of --steps runs after --warmup runs, device events on one
stream), milliseconds per decode step and the ratio to the greedy decode of this run.

    python tools/bench_sbl_beam.py --steps 20 --warmup 5
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_beam import graphed  # noqa: E402
from bench_seq2seq import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=29)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--beams", type=int, nargs="*", default=[1, 3, 5])
    ap.add_argument("--nbest", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="bf16x6")
    args = ap.parse_args()

    from sbl_for_multilingual_lip_reading_amd import config, ops
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    ops.set_matmul_precision(args.precision)
    torch.manual_seed(0)
    dev = "cuda:0"
    B, T, steps = args.batch, args.frames, config.MAX_DECODE_LEN
    dec = Decoder(0, 1, 58, 512, args.layers, 8, 64, 64, 512, 2048).to(dev).eval()
    enc = torch.randn(B, T, 512, device=dev)
    out = {"tool": "bench_sbl_beam", "batch": B, "frames": T, "layers": args.layers, "nbest": args.nbest,
           "precision": args.precision, "steps": args.steps, "warmup": args.warmup}
    with torch.no_grad():
        graph, keep = graphed(lambda: dec.recognize_beam(enc))
        greedy, _ = timed(graph.replay, args.steps, args.warmup)
        out["greedy_graph_ms"] = greedy
        del graph, keep
        for W in args.beams:
            run = lambda: dec.beam_search(enc, W, min(args.nbest, W))      # noqa: E731
            eager, _ = timed(run, args.steps, args.warmup)
            graph, keep = graphed(run)
            rep, _ = timed(graph.replay, args.steps, args.warmup)
            out["beam%d_eager_ms" % W], out["beam%d_graph_ms" % W] = eager, rep
            out["beam%d_graph_ms_per_step" % W] = rep / steps
            out["beam%d_graph_over_greedy" % W] = rep / greedy
            del graph, keep
    print(json.dumps(out))


if __name__ == "__main__":
    main()
