"""One validation batch (B = 32, eval mode, 6 + 6 layers, 29 x 88 x 88 clips) three ways:
  (a) Transformer.recognize alone, one hipGraph replay;
  (b) Transformer.validate = recognize + sbl_seq_score into a device meter, one hipGraph replay, no host sync inside;
  (c) the recognize replay of (a) followed by a host loop that restates SBL/train.py:251-276 in this file: per row and
      direction a .cpu().numpy() of the tokens and of the target, lists of names, and a pure-Python edit distance per
      sample (the reference computes its distances once per epoch over the same lists; here they are computed per batch so
      that the figure is per batch, and every sample enters once: the duplicating `extend` of :262-263 is left out.  The
      reference calls the C extension `editdistance`, which this loop does not have: the copies and list building are the
      reference's, the distance itself is slower here than there).
(b) - (a) is what scoring costs on the device, (c) - (a) what the host loop as written here costs.  The three are timed
alternately, REPS rounds after WARM warm-up rounds, host clock around replay .. synchronize; medians are printed with the
min-max range.  The scorer's own time is taken from device events around a graph of 100 back-to-back launches (so it includes
the gap between two kernels of a graph).

Measured on one MI355X (bf16x6 arithmetic, the default of bench.py), median (min - max) ms per batch:
(a) 21.52 (21.40 - 21.90), (b) 21.62 (21.08 - 21.77), (c) 25.03 (24.81 - 25.54); (b) - (a) = +0.10 ms, below the 2-3 %
box-to-box spread and so no difference; (c) - (a) = +3.51 ms; sbl_seq_score 9.8 us per launch (64 pairs, name table)."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from sbl_for_multilingual_lip_reading_amd import detfill, ops
from sbl_for_multilingual_lip_reading_amd.transformer.metrics import ErrorRateMeter

B, WARM, REPS = 32, 5, 40
SOS, EOS, IGN = 0, 1, -1
# a made-up spelling per id (the reference's phoneme list is not part of this repository)
NAMES = ["<s>", "</s>"] + [chr(97 + k) for k in range(26)] + [chr(97 + (7 * k) % 26) + chr(97 + (3 * k + 1) % 26) for k in range(30)]


def edit_distance(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def host_loop(pred_l2r, pred_r2l, gold_l2r, gold_r2l, totals):
    """train.py:251-276, then per_compute / wer_compute on this batch's lists; totals[d] = [sum dist/c, word errors, n]"""
    for d, (pred, gold) in enumerate(((pred_l2r, gold_l2r), (pred_r2l, gold_r2l))):
        pred_txt, gold_txt, pred_ph, gold_ph = [], [], [], []
        for n in range(pred.size(0)):
            golds = [NAMES[one] for one in gold[n].cpu().numpy() if one not in (SOS, EOS, IGN)]
            c = len(golds)
            preds = [NAMES[one] for one in pred[n].cpu().numpy()[:c + 1] if one not in (SOS, EOS, IGN)]
            pred_txt.append("".join(preds))
            gold_txt.append("".join(golds))
            pred_ph.append(preds)
            gold_ph.append(golds)
        for p, g, pt, gt in zip(pred_ph, gold_ph, pred_txt, gold_txt):
            totals[d][0] += edit_distance(p, g) / len(g)
            totals[d][1] += edit_distance(pt.split(" "), gt.split(" ")) / len(gt.split(" "))
            totals[d][2] += 1


def capture(fn, stream):
    stream.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(stream):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g, stream=stream):
        out = fn()
    return g, out


def main():
    dev = torch.device("cuda", 0)
    ops.set_matmul_precision("bf16x6")
    m = bench.build_model(dev, False)
    # the "varied" gains: greedy tokens that differ across steps and samples (detfill.GAIN_SETS)
    m.load_state_dict({k: (v if k.endswith(".pe") else torch.from_numpy(detfill.fill_value(k, tuple(v.shape), 0, "varied").copy()))
                       for k, v in m.state_dict().items()})
    m.eval()
    x, l2r, r2l = (torch.from_numpy(a).to(dev) for a in detfill.synthetic_batch(B, 29, 88, 88, 7))
    meter = ErrorRateMeter(NAMES, device=dev)
    s = torch.cuda.Stream()
    g_rec, ys = capture(lambda: m.recognize(x), s)
    g_val, _ = capture(lambda: m.validate(x, l2r, r2l, meter), s)
    meter.reset()
    totals = [[0.0, 0.0, 0], [0.0, 0.0, 0]]

    def run_a():
        g_rec.replay()

    def run_b():
        g_val.replay()

    def run_c():
        g_rec.replay()
        host_loop(ys[0], ys[1], l2r, r2l, totals)

    times = {"a": [], "b": [], "c": []}
    for r in range(WARM + REPS):
        for tag, fn in (("a", run_a), ("b", run_b), ("c", run_c)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= WARM:
                times[tag].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    for tag, what in (("a", "recognize, graph replay"), ("b", "validate, graph replay"), ("c", "recognize replay + host loop")):
        print("(%s) %-30s %8.3f ms per batch of %d  (min %.3f, max %.3f, %d rounds)" % (tag, what, med[tag], B, min(times[tag]), max(times[tag]), REPS))
    print("(b) - (a) = %+.3f ms   (c) - (a) = %+.3f ms" % (med["b"] - med["a"], med["c"] - med["a"]))

    # the scorer alone: 100 launches in one graph, device events around the replay
    probe = ErrorRateMeter(NAMES, device=dev)
    g_k, _ = capture(lambda: [probe.update(ys[0], ys[1], l2r, r2l) for _ in range(100)], s)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for r in range(WARM + REPS):
        e0.record()
        g_k.replay()
        e1.record()
        torch.cuda.synchronize()
        if r >= WARM:
            per.append(e0.elapsed_time(e1) * 1e3 / 100)
    print("sbl_seq_score: %.2f us per launch back to back in a graph (min %.2f, max %.2f), %d pairs per launch" % (statistics.median(per), min(per), max(per), 2 * B))

    # same answers: the device meter over its WARM + REPS batches against the host loop over its own
    res = meter.result()
    print("device meter: l2r per %.6f wer %.6f | r2l per %.6f wer %.6f | n %d" % (res["l2r_per"], res["l2r_wer"], res["r2l_per"], res["r2l_wer"], res["n"]))
    print("host loop   : l2r per %.6f wer %.6f | r2l per %.6f wer %.6f | n %d" % (totals[0][0] / totals[0][2], totals[0][1] / totals[0][2], totals[1][0] / totals[1][2], totals[1][1] / totals[1][2], totals[0][2]))


if __name__ == "__main__":
    main()
