#!/usr/bin/env python3
"""Times the decoder of the single-direction seq2seq model (transformer/seq2seq.py) at the LRW1000 shapes, B = 32 clips,
T = 29 encoder frames = decode steps, 6 decoder layers, 48 classes, on a fixed encoder output: the KV-cached greedy decode
under one hipGraph, and the batched beam search (Seq2SeqDecoder.beam_search) with W = 1, 5 and 8, eager and under one
hipGraph.  Prints one JSON line: milliseconds per call (median of --steps runs after --warmup runs, device events on one
stream), milliseconds per decode step, the ratio to the greedy decode, and whether a W = 8 step is no slower than eight
W = 1 steps.  With --lexicon-words N (default 1000 seeded random words of 2..13 tokens) it then times the lexicon-constrained
search (Seq2SeqDecoder.beam_search_lex with a Lexicon: longest word + 1 steps) next to the unconstrained one at the same W,
both eager and under one hipGraph, in --rounds alternating rounds: per W the medians over the rounds' medians with their
spread (max - min), per search and per decode step ("lex_*" keys).

    python tools/bench_beam.py --steps 20 --warmup 5
"""
import argparse
import json
import os
import random
import statistics
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
    ap.add_argument("--lexicon-words", type=int, default=1000, help="0: skip the lexicon-constrained runs")
    ap.add_argument("--rounds", type=int, default=5)
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
    if args.lexicon_words:
        from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
        rnd = random.Random(0)
        lex = Lexicon([[rnd.randrange(2, V) for _ in range(rnd.randint(2, 13))] for _ in range(args.lexicon_words)],
                      device=dev, vocab=V)
        lex.trie()          # built on the host once, before any capture
        steps_lex = lex.max_len + 1
        out.update(lex_words=args.lexicon_words, lex_steps=steps_lex, lex_trie_nodes=int(lex.trie()[0].numel()), lex_rounds=args.rounds)
        med, spread = statistics.median, lambda v: max(v) - min(v)      # noqa: E731
        with torch.no_grad():
            for W in args.beams:
                runs = {"beam": (lambda: dec.beam_search(enc, W, args.nbest, 0, prior), T),
                        "lex": (lambda: dec.beam_search_lex(enc, W, args.nbest, 0, prior, lex), steps_lex)}
                graphs = {k: graphed(fn) for k, (fn, _) in runs.items()}
                ms = {(k, mode): [] for k in runs for mode in ("eager", "graph")}
                for _ in range(args.rounds):          # alternating: beam, lex, beam, lex, ...
                    for k, (fn, _) in runs.items():
                        ms[k, "eager"].append(timed(fn, args.steps, args.warmup)[0])
                        ms[k, "graph"].append(timed(graphs[k][0].replay, args.steps, args.warmup)[0])
                for (k, mode), v in ms.items():
                    n = runs[k][1]
                    tag = "lex_%s%d_%s" % (k, W, mode)
                    out[tag + "_ms"], out[tag + "_ms_spread"] = round(med(v), 4), round(spread(v), 4)
                    out[tag + "_ms_per_step"], out[tag + "_ms_per_step_spread"] = round(med(v) / n, 5), round(spread(v) / n, 5)
                out["lex_lex%d_graph_over_beam" % W] = round(med(ms["lex", "graph"]) / med(ms["beam", "graph"]), 4)
                del graphs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
