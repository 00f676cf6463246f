#!/usr/bin/env python3
"""Times the decode of a batch of ragged clips at the model's shapes: B = 32 clips of 29 x 88 x 88, 6 + 6
layers, eval mode, every call under one hipGraph.  Transformer.recognize and Transformer.validate_words_lex (W = 5, a
synthetic lexicon of 1000 words) in three forms, in --rounds alternating rounds:
  (a) without lengths                              - the path of a batch whose clips all fill their frames;
  (b) with a CUDA lengths tensor of all 29         - the key-count kernels doing the same work;
  (c) with lengths drawn uniformly from 8..29      - a ragged batch.
Then the encoder alone under the lengths of (c): the explicit-mask route (the workgroup kernel; what gradients-enabled calls
take) against the key-count route; and what a caller had to do for an exact answer without the lengths: one recognize call per
distinct length on the clips of that length cut to it (the sum of the per-length graphs).  Last (alone with --only-kernel):
the decoder's cross-attention launch by itself, grouped entry against key-count entry (kernel_rows).
Prints one JSON line: milliseconds per call (median over the rounds of the median of --steps replays after --warmup, device
events on one stream) with the spread (max - min) over the rounds, and (b) - (a) next to the spread of (a).

    python tools/bench_ragged.py --steps 20 --warmup 5 --rounds 3
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
import bench  # noqa: E402
from bench_beam import graphed  # noqa: E402
from bench_seq2seq import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=29)
    ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default="bf16x6")
    ap.add_argument("--only-kernel", action="store_true", help="only the cross-attention launch rows (kernel_rows)")
    args = ap.parse_args()

    from sbl_for_multilingual_lip_reading_amd import config, detfill, ops
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    from sbl_for_multilingual_lip_reading_amd.transformer.metrics import WordAccuracyMeter
    ops.set_matmul_precision(args.precision)
    dev = torch.device("cuda", 0)
    B, T, W = args.batch, args.frames, args.beam
    m = bench.build_model(dev, False)
    m.load_state_dict({k: (v if k.endswith(".pe") else torch.from_numpy(detfill.fill_value(k, tuple(v.shape), 0, "varied").copy()))
                       for k, v in m.state_dict().items()})
    m.eval()
    rng = np.random.RandomState(0)
    lengths = rng.randint(8, T + 1, size=B)
    x = detfill.synthetic_batch(B, T, 88, 88, 7)[0]
    for n, l in enumerate(lengths):
        x[n, l:] = 0.0                                           # the loader's padding: all-zero frames
    x = torch.from_numpy(x).to(dev)
    lex = Lexicon([rng.randint(2, config.vocab_size, size=rng.randint(3, 15)).tolist() for _ in range(args.words)], device=dev)
    gold = torch.from_numpy(rng.randint(0, len(lex), size=B)).to(dev)
    meter = WordAccuracyMeter(device=dev)
    forms = {"a_none": None, "b_full": torch.full((B,), T, dtype=torch.int32, device=dev),
             "c_ragged": torch.tensor(lengths, dtype=torch.int32, device=dev)}
    if args.only_kernel:
        out = {"tool": "bench_ragged", "batch": B, "frames": T, "beam": W, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds}
        kernel_rows(args, dev, B, T, W, out)
        print(json.dumps(out))
        return
    out = {"tool": "bench_ragged", "batch": B, "frames": T, "words": args.words, "beam": W, "precision": args.precision,
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "lengths": lengths.tolist()}
    runs = {}
    for tag, lens in forms.items():
        runs["recognize_" + tag] = lambda lens=lens: m.recognize(x, lens)
        runs["words_lex_" + tag] = lambda lens=lens: m.validate_words_lex(x, gold, lex, meter, beam_size=W, nbest=W, input_lengths=lens)
    with torch.no_grad():
        feats = m.visual_frontend(x.unsqueeze(1))
        lens_c = forms["c_ragged"]
        runs["encoder_keycount"] = lambda: m.encoder(feats, lens_c)

        def encoder_mask():                                      # the route of a gradients-enabled call: explicit (B, T, T) mask
            with torch.enable_grad():
                return m.encoder(feats, lens_c)
        for p in m.parameters():
            p.requires_grad_(False)
        runs["encoder_mask"] = encoder_mask
        graphs = {k: graphed(fn) for k, fn in runs.items()}
        # one call per distinct length on the clips of that length, cut to it
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
    for k in ("recognize", "words_lex"):
        out[k + "_b_minus_a_ms"] = round(out[k + "_b_full_ms"] - out[k + "_a_none_ms"], 4)
        out[k + "_b_within_spread_of_a"] = bool(out[k + "_b_minus_a_ms"] <= out[k + "_a_none_ms_spread"])
    kernel_rows(args, dev, B, T, W, out)
    print(json.dumps(out))


def kernel_rows(args, dev, B, T, W, out):
    """The decoder's cross-attention launch alone at the shapes of the width-W search (B * W sequences of 8 heads, one segment
    of 1 / 8 / 15 queries, T keys shared by a clip's W slots): sbl_attention_seg_grouped_fwd against sbl_attention_seg_len_fwd
    with counts of all T and with counts 8..T, 100 launches per graph, alternating rounds -> microseconds per launch."""
    import ctypes

    from sbl_for_multilingual_lip_reading_amd import ops
    S, H, HD = B * W, 8, 512
    kv = torch.randn(B * T, 2 * HD, device=dev)
    full = torch.full((B,), T, dtype=torch.int32, device=dev)
    ragged = torch.from_numpy(np.random.RandomState(0).randint(8, T + 1, size=B).astype(np.int32)).to(dev)
    for L in (1, 8, 15):
        q, o = torch.randn(S * L, HD, device=dev), torch.empty(S * L, HD, device=dev)
        seg = (ctypes.c_int * 1)(L)
        head = (q.data_ptr(), HD, kv.data_ptr(), 2 * HD, kv[:, HD:].data_ptr(), 2 * HD, o.data_ptr(), HD, S, H, seg, 1, T, W)

        def launch(lens):
            for _ in range(100):
                if lens is None:
                    ops.call("sbl_attention_seg_grouped_fwd", *head, 0.125, 0.0, None, 0, ops._s())
                else:
                    ops.call("sbl_attention_seg_len_fwd", *head, lens.data_ptr(), 0.125, 0.0, None, 0, ops._s())
        graphs = {"grouped": graphed(lambda: launch(None)), "len_full": graphed(lambda: launch(full)), "len_ragged": graphed(lambda: launch(ragged))}
        us = {k: [] for k in graphs}
        for _ in range(args.rounds):
            for k, (g, _) in graphs.items():
                us[k].append(timed(g.replay, args.steps, args.warmup)[0] * 10.0)
        for k, v in us.items():
            out["attn_L%d_%s_us" % (L, k)], out["attn_L%d_%s_us_spread" % (L, k)] = round(statistics.median(v), 3), round(max(v) - min(v), 3)


if __name__ == "__main__":
    main()
