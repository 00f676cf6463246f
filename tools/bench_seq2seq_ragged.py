#!/usr/bin/env python3
"""Times the single-direction baseline's decodes on a batch of ragged clips at the model's shapes: B = 32
clips of 29 x 88 x 88, 6 + 6 layers, vocab 48, eval mode, every call under one hipGraph.  Seq2SeqTransformer.recognize and
recognize_words (W = 5, a synthetic lexicon of 1000 words) in three forms, in --rounds alternating rounds:
  (a) without lengths                         - today's path, launch for launch;
  (b) with a CUDA lengths tensor of all 29    - the key-count step attention doing the same work;
  (c) with lengths drawn uniformly from 8..29 - a ragged batch;
and what a caller had to do for an exact answer without the lengths: one recognize call per distinct length on the clips of
that length cut to it.  Prints one JSON line: milliseconds per call (median over the rounds of the median of --steps replays
after --warmup, device events on one stream) with the spread (max - min) over the rounds.

    python tools/bench_seq2seq_ragged.py --steps 20 --warmup 5 --rounds 3
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
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
    ap.add_argument("--vocab", type=int, default=48)
    ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default="bf16x6")
    args = ap.parse_args()

    from sbl_for_multilingual_lip_reading_amd import ops
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    from sbl_for_multilingual_lip_reading_amd.transformer.seq2seq import Seq2SeqDecoder, Seq2SeqTransformer
    ops.set_matmul_precision(args.precision)
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    B, T, W, V = args.batch, args.frames, args.beam, args.vocab
    m = Seq2SeqTransformer(Encoder(512, args.layers, 8, 64, 64, 512, 2048),
                           Seq2SeqDecoder(0, 1, V, 512, args.layers, 8, 64, 64, 512, 2048, tgt_emb_prj_weight_sharing=False)).to(dev).eval()
    rng = np.random.RandomState(0)
    lengths = rng.randint(8, T + 1, size=B)
    x = torch.randn(B, T, 88, 88)
    for n, l in enumerate(lengths):
        x[n, l:] = 0.0                                           # the loader's padding: all-zero frames
    x = x.to(dev)
    lex = Lexicon([rng.randint(2, V, size=rng.randint(3, 15)).tolist() for _ in range(args.words)], device=dev, vocab=V, sos_id=0, eos_id=1)
    lex.trie()
    forms = {"a_none": None, "b_full": torch.full((B,), T, dtype=torch.int32, device=dev),
             "c_ragged": torch.tensor(lengths, dtype=torch.int32, device=dev)}
    out = {"tool": "bench_seq2seq_ragged", "batch": B, "frames": T, "layers": args.layers, "vocab": V, "words": args.words, "beam": W,
           "precision": args.precision, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "lengths": lengths.tolist()}
    runs = {}
    for tag, lens in forms.items():
        runs["recognize_" + tag] = lambda lens=lens: m.recognize(x, input_lengths=lens)
        runs["words_" + tag] = lambda lens=lens: m.recognize_words_len(x, lens, lex, beam_size=W, nbest=W)
    with torch.no_grad():
        graphs = {k: graphed(fn) for k, fn in runs.items()}
        per_len = {}
        for l in sorted(set(lengths.tolist())):
            xs = x[torch.from_numpy(np.flatnonzero(lengths == l)).to(dev), :l].contiguous()
            per_len[l] = graphed(lambda xs=xs: m.recognize(xs))

        def per_length():
            for g, _ in per_len.values():
                g.replay()
        ms = {k: [] for k in list(runs) + ["recognize_per_length"]}
        for _ in range(args.rounds):                             # alternating: every row once per round
            for k in runs:
                ms[k].append(timed(graphs[k][0].replay, args.steps, args.warmup)[0])
            ms["recognize_per_length"].append(timed(per_length, args.steps, args.warmup)[0])
    for k, v in ms.items():
        out[k + "_ms"], out[k + "_ms_spread"] = round(statistics.median(v), 4), round(max(v) - min(v), 4)
    out["distinct_lengths"] = len(per_len)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
