"""Shared by tests/test_metrics_cpu.py and tests/test_metrics_gpu.py: the scoring definition restated in plain Python
(SBL/train.py:252-254 and :40-42: Python lists, textbook Levenshtein) and a seeded generator of (prediction, target) pairs
that builds the awkward classes explicitly."""
import numpy as np

SOS, EOS, IGN = 0, 1, -1
VOCAB, LY, TO = 58, 17, 15
SPECIAL = (SOS, EOS, IGN)

# A made-up spelling per id (not the reference's phoneme list): ids 2..27 spell one letter, ids 28..57 two letters, so
# that two one-letter ids and one two-letter id can spell the same string.
NAMES = ["<s>", "</s>"] + [chr(97 + k) for k in range(26)] + [chr(97 + (7 * k) % 26) + chr(97 + (3 * k + 1) % 26) for k in range(30)]
TWO = 28                                                    # id whose name has two letters ...
ONE_A, ONE_B = 2 + ord(NAMES[TWO][0]) - 97, 2 + ord(NAMES[TWO][1]) - 97      # ... and the ids of those letters


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def restate(ys, gold, names=None):
    """(dist, c, word_err) of one sample of one direction."""
    golds = [int(t) for t in gold if t not in SPECIAL]
    c = len(golds)
    preds = [int(t) for t in ys[:c + 1] if t not in SPECIAL]
    if names is None:
        werr = int(preds != golds)
    else:
        werr = int("".join(names[t] for t in preds) != "".join(names[t] for t in golds))
    return levenshtein(preds, golds), c, werr


def expect(samples):
    """What a meter must report for one direction, from the restated (dist, c, word_err) of its samples: integers, and
    fp64 means formed from those integers (sum over the gold lengths of dist_by_len / len, over the scored count)."""
    scored = [s for s in samples if s[1] > 0]
    n = len(scored)
    by_len = [0] * 16
    for d, c, _ in scored:
        by_len[c] += d
    nan = float("nan")
    return {"n": n, "n_empty": len(samples) - n,
            "wer": sum(s[2] for s in scored) / n if n else nan,
            "per": sum(by_len[c] / c for c in range(1, 16)) / n if n else nan,
            "per_corpus": sum(s[0] for s in scored) / sum(s[1] for s in scored) if n else nan}


def counters(samples):
    """The 37 counters of one direction (include/sbl_hip.h, SBL_SCORE_*)."""
    scored = [s for s in samples if s[1] > 0]
    by_len, cnt = [0] * 16, [0] * 16
    for d, c, _ in scored:
        by_len[c] += d
        cnt[c] += 1
    return [len(scored), len(samples) - len(scored), sum(s[2] for s in scored), sum(s[0] for s in scored),
            sum(s[1] for s in scored)] + by_len + cnt


def _row(tokens, width, fill):
    r = np.full(width, fill, dtype=np.int64)
    r[:len(tokens)] = tokens
    return r


def generate(n_random=2048, seed=20):
    """(ys (M, 17), gold (M, 15)) int64: the explicit classes first (so that every prefix of >= 32 rows holds them all),
    then n_random seeded pairs: gold of 0..15 ids with stray IGNORE_ID / sos / eos inside, prediction = the gold under
    random edits (or noise) with stray eos / IGNORE_ID, random tail behind the window."""
    rng = np.random.RandomState(seed)
    ys, gold = [], []

    def add(pred, tgt, tail=EOS):
        ys.append(_row([SOS] + list(pred), LY, tail))
        gold.append(_row(tgt, TO, IGN))

    full = [int(t) for t in rng.randint(2, VOCAB, size=15)]
    add([5, 6, 7], [])                                       # c = 0, prediction not empty
    add([], [IGN] * 3)                                       # c = 0, nothing predicted
    add(full, full)                                          # c = 15, exact match over the full width
    add(full[:7] + [9] + full[8:], full)                     # c = 15, one substitution
    add([4, 5, 6], [4, 5, 6])                                # exact match
    add([4, EOS, 6, 7], [4, 5, 6, 7])                        # eos inside the window, a kept token behind it
    add([4, 5, 6, 7, 8, 9, 10], [4, 5, 6], tail=11)          # prediction longer than the window
    add([EOS] * 16, [4, 5, 6, 7])                            # all-eos prediction
    add([TWO], [ONE_A, ONE_B])                               # ids differ, spellings agree
    add([ONE_A, ONE_B], [TWO, 3])                            # the other way round, then one more letter: spellings differ
    add([4, IGN, 5], [4, IGN, 5, SOS, 6])                    # specials in the middle of both
    for _ in range(n_random):
        c = int(rng.randint(0, 16))
        g = [int(t) for t in rng.randint(2, 12 if rng.rand() < 0.5 else VOCAB, size=c)]
        tgt = list(g)
        while len(tgt) < TO and rng.rand() < 0.2:            # stray specials inside the target row
            tgt.insert(int(rng.randint(0, len(tgt) + 1)), int(rng.choice(SPECIAL)))
        kind = rng.rand()
        if kind < 0.15:
            p = list(g)
        elif kind < 0.3:
            p = [int(t) for t in rng.randint(2, VOCAB, size=int(rng.randint(0, 17)))]
        else:
            p = []
            for t in g:
                e = rng.rand()
                if e < 0.1:
                    continue                                 # deletion
                p.append(int(rng.randint(2, VOCAB)) if e < 0.25 else t)
                if e > 0.9:
                    p.append(int(rng.randint(2, VOCAB)))     # insertion
                if e > 0.97:
                    p.append(int(rng.choice((EOS, IGN))))
        p = p[:16]
        tail = [int(t) for t in rng.choice([EOS, EOS, IGN, 3, 40], size=16 - len(p))]
        add(p + tail, tgt)
    return np.stack(ys), np.stack(gold)
