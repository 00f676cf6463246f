#!/usr/bin/env python3
"""Times the closed-vocabulary word decode (Transformer.recognize_words) on one validation batch at the model's shapes:
B = 32 clips of 29 x 88 x 88, 6 + 6 layers, eval mode, a synthetic lexicon of 1000 words.  In one run: Transformer.validate
(the greedy decode with the WER / PER meter) under one hipGraph as the yardstick; recognize_words with greedy hypotheses and
a shortlist of 4 and of 8, and with the 5 best pairs of a width-5 beam search and a shortlist of 8, each eager and under one
hipGraph; the rescoring stage alone (Decoder.score_pairs on a shortlist of 8: 8 x 136 rows per clip and direction) under one
hipGraph; and the shortlist launch alone (100 launches in one graph).  Prints one JSON line: milliseconds per call (median of
--steps runs after --warmup runs, device events on one stream), the ratio to validate, and the share of the (greedy, K = 8)
call that the rescoring stage takes.  Last (alone with --only-lex): the one-pass decode, Transformer.validate_words_lex at
W = 1 / 5 / 8, next to the two-pass validate_words rows in alternating rounds (lex_rows).

    python tools/bench_words.py --steps 20 --warmup 5
    python tools/bench_words.py --only-lex --rounds 3
"""
import argparse
import json
import os
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="bf16x6")
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds of the one-pass / two-pass rows")
    ap.add_argument("--only-lex", action="store_true", help="only the one-pass / two-pass rows (lex_rows)")
    args = ap.parse_args()

    from sbl_for_multilingual_lip_reading_amd import config, detfill, ops
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    from sbl_for_multilingual_lip_reading_amd.transformer.metrics import ErrorRateMeter
    ops.set_matmul_precision(args.precision)
    dev = torch.device("cuda", 0)
    B, T, Wn = args.batch, args.frames, args.words
    m = bench.build_model(dev, False)
    # the "varied" gains: greedy tokens that differ across steps and samples (detfill.GAIN_SETS)
    m.load_state_dict({k: (v if k.endswith(".pe") else torch.from_numpy(detfill.fill_value(k, tuple(v.shape), 0, "varied").copy()))
                       for k, v in m.state_dict().items()})
    m.eval()
    x, l2r, r2l = (torch.from_numpy(a).to(dev) for a in detfill.synthetic_batch(B, T, 88, 88, 7))
    rng = np.random.RandomState(0)
    lex = Lexicon([rng.randint(2, config.vocab_size, size=rng.randint(3, 15)).tolist() for _ in range(Wn)], device=dev)
    meter = ErrorRateMeter(device=dev)
    out = {"tool": "bench_words", "batch": B, "frames": T, "words": Wn, "precision": args.precision, "steps": args.steps,
           "warmup": args.warmup}
    if args.only_lex:
        lex_rows(args, m, x, lex, out)
        print(json.dumps(out))
        return
    with torch.no_grad():
        graph, keep = graphed(lambda: m.validate(x, l2r, r2l, meter))
        base, _ = timed(graph.replay, args.steps, args.warmup)
        out["validate_greedy_graph_ms"] = base
        del graph, keep
        for tag, kw in (("greedy_k4", dict(shortlist=4)), ("greedy_k8", dict(shortlist=8)),
                        ("beam5_nbest5_k8", dict(beam_size=5, nbest=5, shortlist=8))):
            run = lambda: m.recognize_words(x, lex, **kw)      # noqa: E731
            eager, _ = timed(run, args.steps, args.warmup)
            graph, keep = graphed(run)
            rep, _ = timed(graph.replay, args.steps, args.warmup)
            out[tag + "_eager_ms"], out[tag + "_graph_ms"], out[tag + "_graph_over_validate"] = eager, rep, rep / base
            del graph, keep
        # the rescoring stage alone, on the candidates of the (greedy, K = 8) call
        enc, _ = m._encode(x)
        ys = m.decoder.recognize_beam(enc)
        sl = ops.lexicon_shortlist(ys[0], ys[1], lex.packed, 8, 0, 1, config.IGNORE_ID)
        graph, keep = graphed(lambda: m.decoder.score_pairs(enc, sl.cand_ys_l2r, sl.cand_ys_r2l, sl.n_pos, group=8))
        out["rescore_k8_graph_ms"], _ = timed(graph.replay, args.steps, args.warmup)
        out["rescore_k8_rows_per_clip_and_direction"] = 8 * 136
        out["rescore_k8_share_of_greedy_k8"] = out["rescore_k8_graph_ms"] / out["greedy_k8_graph_ms"]
        del graph, keep
        # the shortlist launch alone: 100 back-to-back launches in one graph
        for tag, hyp in (("h1", ys), ("h5", tuple(y.unsqueeze(1).repeat(1, 5, 1) for y in ys))):
            for K in (4, 8):
                graph, keep = graphed(lambda: [ops.lexicon_shortlist(hyp[0], hyp[1], lex.packed, K, 0, 1, config.IGNORE_ID) for _ in range(100)])
                ms, _ = timed(graph.replay, args.steps, args.warmup)
                out["shortlist_%s_k%d_us" % (tag, K)] = ms * 1e3 / 100
                del graph, keep
    lex_rows(args, m, x, lex, out)
    print(json.dumps(out))


def lex_rows(args, m, x, lex, out):
    """The one-pass decode (Transformer.validate_words_lex, the lexicon-constrained pair beam search) at W = 1 / 5 / 8 next to
    the two-pass validate_words rows (greedy, K = 8; beam 5 with its 5 best, K = 8), each with the WordAccuracyMeter, eager
    and under one hipGraph, in --rounds alternating rounds: the medians over the rounds' medians with their spread
    (max - min) as "words_*" keys, and the ratio of every graph row to the (greedy, K = 8) graph row of the same run."""
    import statistics

    from sbl_for_multilingual_lip_reading_amd.transformer.metrics import WordAccuracyMeter
    dev = x.device
    gold = torch.from_numpy(np.random.RandomState(1).randint(0, len(lex), size=x.size(0))).to(dev)
    meter = WordAccuracyMeter(device=dev)
    runs = {"twopass_greedy_k8": lambda: m.validate_words(x, gold, lex, meter, shortlist=8),
            "twopass_beam5_k8": lambda: m.validate_words(x, gold, lex, meter, beam_size=5, nbest=5, shortlist=8)}
    for W in (1, 5, 8):
        runs["lex_w%d" % W] = lambda W=W: m.validate_words_lex(x, gold, lex, meter, beam_size=W, nbest=W)
    out.update(words_rounds=args.rounds, words_lex_steps=lex.max_len + 1, words_twopass_steps="16 + one rescoring stage",
               words_pair_trie_nodes=int(lex.pair_trie()[2].numel()), words_pair_trie_root_children=int(lex.pair_trie()[0][1]))
    med, spread = statistics.median, lambda v: max(v) - min(v)      # noqa: E731
    with torch.no_grad():
        graphs = {k: graphed(fn) for k, fn in runs.items()}
        ms = {(k, mode): [] for k in runs for mode in ("eager", "graph")}
        for _ in range(args.rounds):          # alternating: every row once per round
            for k, fn in runs.items():
                ms[k, "eager"].append(timed(fn, args.steps, args.warmup)[0])
                ms[k, "graph"].append(timed(graphs[k][0].replay, args.steps, args.warmup)[0])
        for (k, mode), v in ms.items():
            out["words_%s_%s_ms" % (k, mode)], out["words_%s_%s_ms_spread" % (k, mode)] = round(med(v), 4), round(spread(v), 4)
        for k in runs:
            out["words_%s_graph_over_twopass_greedy_k8" % k] = round(med(ms[k, "graph"]) / med(ms["twopass_greedy_k8", "graph"]), 4)
        del graphs


if __name__ == "__main__":
    main()
