"""Validation metrics kept on the device: WER / PER of greedy decodes (the scoring of valid_lrw / valid_lrw1000,
SBL/train.py:212-362 and SBL/test.py:146-300, with wer_compute / per_compute of train.py:28-42).

Per direction and sample, with `ys` the (17,) row Transformer.recognize returns and `gold` the IGNORE_ID-padded target:
  g = gold without sos / eos / IGNORE_ID, c = len(g);  p = ys[:c+1] without sos / eos / IGNORE_ID (an eos is stripped where
  it stands; the row is not cut at the first eos);  dist = Levenshtein(p, g) over ids;  PER = mean of dist / c;
  word error = 0 if p and g spell the same string, else 1, and WER = its mean.  The reference joins the phoneme NAMES without
  a separator before it compares, so two different id sequences can be the same word ("a" + "n" against "an"): give the
  meter the list of names (one short ASCII string per id) to compare spellings; without it the ids are compared.

Deviations from the reference, on purpose:
  (a) every sample counts once (train.py:262-263 extends the WER lists inside the per-sample loop, so sample j of a batch
      of B enters the reference's WER mean B - j times);
  (b) a sample whose target is empty (c = 0: a division by zero in the reference) is counted in "n_empty" and left out of
      every mean;
  (c) rows at or beyond an optional `valid_rows` count are ignored (the short last batch of a replayed graph).

Tokens never leave the device: an update is one launch of sbl_seq_score that adds to an integer accumulator, and only
result() synchronises.  All state is integer, so a result is independent of the order of the atomics, identical between
eager launches and graph replays, and sums exactly across ranks."""
import torch

from ._env import config, ops


class ErrorRateMeter:
    """Accumulates the scoring counters of both directions over an epoch.

    names: None, or a list of `vocab` ASCII strings of at most 7 bytes (the spelling of every token id).
    device: where the accumulator lives (and where update()'s tensors must be)."""

    def __init__(self, names=None, device=None, sos_id=config.sos_id, eos_id=config.eos_id, ignore_id=config.IGNORE_ID):
        self.device = torch.device(config.device if device is None else device)
        self.sos_id, self.eos_id, self.ignore_id = int(sos_id), int(eos_id), int(ignore_id)
        self.names = None if names is None else ops.pack_names(names).to(self.device)
        self.acc = torch.zeros(2, ops.SCORE_COUNTERS, dtype=torch.int64, device=self.device)
        self.single = False          # set by update_single: result() then also reports the un-prefixed single-direction keys

    def update(self, ys_l2r, ys_r2l, gold_l2r, gold_r2l, valid_rows=None):
        """Score one batch and add it: one launch on the current stream, no sync, no allocation (capturable).
        valid_rows: None or a device int32[1]; rows at or beyond it are ignored."""
        ops.seq_score(ys_l2r, ys_r2l, gold_l2r, gold_r2l, self.acc, self.sos_id, self.eos_id, self.ignore_id,
                      names=self.names, valid_rows=valid_rows)

    def update_single(self, ys, gold, valid_rows=None):
        """Score one batch of a single-direction model (seq2seq.Seq2SeqTransformer; LRW/train.py:245-260: predictions cut at
        len(gold) + 1 and stripped of sos / eos / IGNORE_ID) and add it to the first counter row: one launch of
        sbl_seq_score1, no sync, no allocation.  The second row stays zero."""
        self.single = True
        ops.seq_score1(ys, gold, self.acc[0], self.sos_id, self.eos_id, self.ignore_id, names=self.names, valid_rows=valid_rows)

    def all_reduce(self, group=None):
        """Sum the counters over the ranks of a torch.distributed group (RCCL on the GPU, gloo on CPU tensors): every
        rank then reads the result of the union of all ranks' samples."""
        torch.distributed.all_reduce(self.acc, op=torch.distributed.ReduceOp.SUM, group=group)

    def reset(self):
        self.acc.zero_()

    def result(self):
        """The one synchronisation: read the counters and form the means in fp64.
        {"l2r_wer", "l2r_per", "r2l_wer", "r2l_per"}: means over the scored samples (nan when there are none);
        "n", "n_empty": scored / empty-target samples of the l2r direction ("r2l_n", "r2l_n_empty": of the other one);
        "l2r_per_corpus", "r2l_per_corpus": sum of distances over sum of target lengths."""
        a = self.acc.cpu().tolist()
        nan = float("nan")
        out = {}
        for d, tag in enumerate(("l2r", "r2l")):
            n = a[d][ops.SCORE_N_SCORED]
            by_len = a[d][ops.SCORE_DIST_BY_LEN:ops.SCORE_DIST_BY_LEN + 16]
            out[tag + "_wer"] = a[d][ops.SCORE_N_WORD_ERR] / n if n else nan
            out[tag + "_per"] = sum(by_len[c] / c for c in range(1, 16)) / n if n else nan
            out[tag + "_per_corpus"] = a[d][ops.SCORE_SUM_DIST] / a[d][ops.SCORE_SUM_LEN] if n else nan
            out["n" if d == 0 else "r2l_n"] = n
            out["n_empty" if d == 0 else "r2l_n_empty"] = a[d][ops.SCORE_N_EMPTY]
        if self.single:      # a single-direction model: "wer", "per", "per_corpus" (with "n", "n_empty") are its result
            out.update(wer=out["l2r_wer"], per=out["l2r_per"], per_corpus=out["l2r_per_corpus"])
        return out


class WordAccuracyMeter:
    """Word accuracy of closed-vocabulary decodes (Transformer.validate_words) over an epoch: int64 device counters
    n (clips), n_correct (word == gold_word) and n_in_shortlist (gold_word is among the shortlisted candidates, the ceiling of
    what rescoring can reach; for Seq2SeqTransformer.validate_words, whose candidates are the distinct words of the constrained
    beam search's n-best, it reads "gold word among the n-best").  Integer torch ops on the device; update() does not synchronise and, after the first call of
    a batch shape, allocates nothing (the work buffers of every batch shape seen are kept), so it can be captured with the
    decode.  All state is integer: it sums exactly across calls, replays and ranks."""

    def __init__(self, device=None):
        self.device = torch.device(config.device if device is None else device)
        self.acc = torch.zeros(3, dtype=torch.int64, device=self.device)      # n, n_correct, n_in_shortlist
        self._bufs = {}      # (N, K) -> work buffers, never dropped: a captured graph keeps writing into the ones it saw

    def _buffers(self, N, K):
        if (N, K) not in self._bufs:
            b = lambda *s: torch.empty(*s, dtype=torch.bool, device=self.device)      # noqa: E731
            rows = torch.arange(N, dtype=torch.int32, device=self.device)
            self._bufs[N, K] = (rows, b(N), b(N), b(N, K), b(N), torch.zeros(3, dtype=torch.int64, device=self.device))
        return self._bufs[N, K]

    def update(self, result, gold_word, valid_rows=None):
        """Add one batch: result = the WordResult of recognize_words, gold_word int64 (N,) word indices on the device.
        valid_rows: None or a device int32[1]; rows at or beyond it are ignored."""
        N, K = result.cand.shape
        if gold_word.shape != (N,) or gold_word.dtype != torch.int64:
            raise ValueError("WordAccuracyMeter.update: gold_word must be int64 (%d,), got %s %s" % (N, gold_word.dtype, tuple(gold_word.shape)))
        if valid_rows is not None and (valid_rows.dtype != torch.int32 or valid_rows.numel() != 1):
            raise ValueError("WordAccuracyMeter.update: valid_rows must be an int32[1] tensor")
        rows, live, hit, among, inside, add = self._buffers(N, K)
        if valid_rows is None:
            live.fill_(True)
        else:
            torch.lt(rows, valid_rows.view(1), out=live)
        torch.eq(result.word, gold_word, out=hit)
        hit.logical_and_(live)
        torch.eq(result.cand, gold_word.unsqueeze(1), out=among)
        torch.any(among, 1, out=inside)
        inside.logical_and_(live)
        for k, t in enumerate((live, hit, inside)):
            torch.sum(t, 0, dtype=torch.int64, out=add[k])
        self.acc.add_(add)

    def all_reduce(self, group=None):
        """Sum the counters over the ranks of a torch.distributed group, as ErrorRateMeter.all_reduce does."""
        torch.distributed.all_reduce(self.acc, op=torch.distributed.ReduceOp.SUM, group=group)

    def reset(self):
        self.acc.zero_()

    def result(self):
        """The one synchronisation: {"n", "n_correct", "n_in_shortlist", "accuracy", "shortlist_recall"} (nan without clips)."""
        n, ok, among = self.acc.cpu().tolist()
        nan = float("nan")
        return dict(n=n, n_correct=ok, n_in_shortlist=among, accuracy=ok / n if n else nan, shortlist_recall=among / n if n else nan)


def wer_per(ys_l2r, ys_r2l, gold_l2r, gold_r2l, names=None):
    """One-shot scoring of a batch: (l2r_wer, l2r_per, r2l_wer, r2l_per), the order valid_lrw returns (train.py:286)."""
    meter = ErrorRateMeter(names, device=ys_l2r.device)
    meter.update(ys_l2r, ys_r2l, gold_l2r, gold_r2l)
    r = meter.result()
    return r["l2r_wer"], r["l2r_per"], r["r2l_wer"], r["r2l_per"]
