"""Inputs shared by tests/test_lexicon_cpu.py and tests/test_lexicon_gpu.py: the hand-worked cases of the shortlist definition
(include/sbl_hip.h, sbl_lexicon_shortlist) and the seeded lexicons / hypotheses that embed them."""
import numpy as np

SOS, EOS, IGN, V = 0, 1, -1, 58


def row(tokens, tail=None):
    """A 17-wide row: sos, the tokens, then eos fill - or, behind one eos, the `tail` (what a decoder leaves there)."""
    r = [SOS] + list(tokens) + [EOS] * (16 - len(tokens))
    if tail is not None:
        k = len(tokens) + 2
        r[k:] = list(tail)[:17 - k]
    assert len(r) == 17
    return r


LONG = list(range(2, 18))          # 16 tokens, no eos in the row

# (name, words, ys_l2r (H rows), ys_r2l (H rows), K, want cand, want dist, want hyp)
HAND = [
    ("empty hypothesis (eos first): D = c + c", [[5], [5, 6]], [row([])], [row([], tail=[9] * 15)], 2, [0, 1], [2, 4], [0, 0]),
    ("16 tokens without eos against a word of length 15", [LONG[:15], [40]], [row(LONG)], [row(LONG[::-1])], 2, [0, 1], [2, 32], [0, 0]),
    ("two identical lexicon rows: the lower index first", [[7, 8], [9], [7, 8]], [row([7, 8])], [row([8, 7])], 3, [0, 2, 1], [0, 0, 4], [0, 0, 0]),
    ("equal D from two hypotheses: the lower h", [[7, 8], [7, 9], [4]], [row([7, 9]), row([7, 8])], [row([8, 7]), row([9, 7])], 3,
     [0, 1, 2], [1, 1, 4], [0, 0, 0]),
    ("the second hypothesis is nearer", [[7, 8], [3]], [row([]), row([7, 8])], [row([]), row([8, 7])], 2, [0, 1], [0, 2], [1, 0]),
    ("sos and ignore are dropped, the row is cut at the first eos", [[7, 8]], [row([7, IGN, 8, SOS], tail=[7] * 12)], [row([SOS, 8, 7])], 1,
     [0], [0], [0]),
]


def make_lexicon(Wn, seed):
    """Wn seeded words of 1..15 tokens in 2..57; word 0 has 15 tokens and (Wn >= 5) words 1 and 3 are identical rows."""
    rng = np.random.RandomState(seed)
    words = [rng.randint(2, V, size=rng.randint(1, 16)).tolist() for _ in range(Wn)]
    words[0] = rng.randint(2, V, size=15).tolist()
    if Wn >= 5:
        words[3] = list(words[1])
    return words


def make_strided_lexicon(Wn, seed, stride=1024):
    """make_lexicon(Wn) whose words at the indices 1 + k * stride and k * stride, k >= 1, are word 1 and word 0 again, exact or
    with one or two edits: a kernel whose lanes stride over the words by `stride` then has ONE lane that owns several of the
    best words of the clips that decode word 1 / word 0 (make_hyps: clips 0 and 2, clip 1 with H = 3)."""
    rng = np.random.RandomState(seed + 1)
    words = make_lexicon(Wn, seed)
    for base in (1, 0):
        for k, w in enumerate(range(base + stride, Wn, stride)):
            v = list(words[base])
            if k % 3 == 1:
                v[len(v) // 2] = int(rng.randint(2, V))
            elif k % 3 == 2 and len(v) > 2:
                del v[int(rng.randint(0, len(v)))]
                v[0] = int(rng.randint(2, V))
            words[w] = v
    return words


def _noisy(rng, w):
    w = list(w)
    for _ in range(rng.randint(1, 3)):
        k = rng.randint(0, 3)
        i = rng.randint(0, len(w)) if w else 0
        if k == 0 and w:
            w[i] = int(rng.randint(2, V))
        elif k == 1 and len(w) > 1:
            del w[i]
        elif len(w) < 16:
            w.insert(i, int(rng.randint(2, V)))
    return w


def make_hyps(words, H, seed):
    """(ys_l2r, ys_r2l) int64 (3, H, 17).  Clip 0 / h 0 is empty, clip 1 / h 0 has 16 tokens and no eos, clip 2 / h 0 is
    exactly word 1 (D = 0; with Wn >= 5 words 1 and 3 tie).  For H = 3: clip 0 holds word 1 twice, as h 1 and h 2 (equal D from
    two hypotheses), clip 1 an l2r row that is exactly the last word beside a random r2l row and the 15-token word with an ignore
    and a sos entry inside, clip 2 two noisy words."""
    rng = np.random.RandomState(seed)
    Wn = len(words)
    pick = lambda: words[rng.randint(0, Wn)]      # noqa: E731
    rnd = lambda n: rng.randint(2, V, size=n).tolist()      # noqa: E731
    ys = np.zeros((2, 3, H, 17), np.int64)
    first = [(row([], tail=rnd(15)), row([])), (row(rnd(16)), row(rnd(16))), (row(words[1 % Wn]), row(words[1 % Wn][::-1]))]
    for n in range(3):
        ys[0, n, 0], ys[1, n, 0] = first[n]
    if H > 1:
        assert H == 3
        a = list(words[1 % Wn])
        w0 = list(words[0])
        rest = [[(row(a), row(a[::-1])), (row(a), row(a[::-1]))],
                [(row(words[-1]), row(rnd(7))), (row(w0[:7] + [IGN] + w0[7:]), row([SOS] + w0[::-1]))],
                [(row(_noisy(rng, pick())), row(_noisy(rng, pick()))), (row(_noisy(rng, pick())), row(rnd(3)))]]
        for n in range(3):
            for h in (1, 2):
                ys[0, n, h], ys[1, n, h] = rest[n][h - 1]
    return ys[0], ys[1]
