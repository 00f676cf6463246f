"""Plain-torch CPU restatement of the lexicon-constrained beam search of the single-direction decoder (include/sbl_hip.h,
sbl_beam_tail_lex; Seq2SeqDecoder.recognize_words) on the primitives of tests/seq2seq_oracle.py, with the word lists, salts
and cases that tests/test_lex_beam_cpu.py and tests/test_lex_beam_gpu.py share.  Used by the tests only.

lex_beam_clip is beam_oracle.beam_clip line for line with one addition: every hypothesis carries its prefix, and candidate
(hypothesis, v) exists only where `allowed(prefix, v)` holds.  With allowed = None it is beam_clip (test_lex_beam_cpu.py pins
every field), so the restatement the reference's fixtures pin carries over.  The lexicon is a plain dict here (prefix tuple ->
children, prefix tuple -> lowest word index): nothing is shared with Lexicon.trie(), whose tables the tests check against it."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import sbl_oracle as O
import beam_oracle as B
import seq2seq_oracle as S


# --------------------------------------------------------------------------- the lexicon as a dict
def dict_trie(words):
    """(children: prefix tuple -> set of next tokens, owner: prefix tuple -> lowest word index) over every prefix, () included."""
    children, owner = {(): set()}, {}
    for i, w in enumerate(words):
        w = tuple(int(t) for t in w)
        for k in range(len(w)):
            children.setdefault(w[:k], set()).add(w[k])
            children.setdefault(w[:k + 1], set())
        owner.setdefault(w, i)
    return children, owner


def bfs_order(children):
    """Breadth-first numbering with siblings in ascending token id = the prefixes sorted by (length, tokens): within one
    depth the parents are in that order by induction, and so are their children."""
    return sorted(children, key=lambda p: (len(p), p))


def child_by_formula(mask, first, p, v, eos):
    """child(p, v) of include/sbl_hip.h on host integers (mask as the unsigned bit pattern)."""
    m = int(mask[p]) & (2 ** 64 - 1)
    return min(max(int(first[p]) + bin(m & ~(1 << eos) & ((1 << v) - 1)).count("1"), 0), len(mask) - 1)


def make_words(Wn, V, seed, lo=1, hi=6, sos=0, eos=1):
    """Wn seeded words of lo..hi tokens over the ids of [0, V) that are neither sos nor eos.  From Wn = 5 on, word 3 repeats
    word 1 (a duplicate row), word 4 is word 0 with one more token (a word that is a prefix of a word) and word 2 uses the
    top id V - 1."""
    rng = np.random.RandomState(seed)
    ids = np.array([t for t in range(V) if t not in (sos, eos)])
    words = [ids[rng.randint(0, len(ids), size=rng.randint(lo, hi + 1))].tolist() for _ in range(Wn)]
    if Wn >= 5:
        words[3] = list(words[1])
        words[0] = words[0][:max(hi - 1, 1)]
        words[4] = words[0] + [int(ids[rng.randint(0, len(ids))])]
        words[2][-1] = V - 1 if V - 1 not in (sos, eos) else words[2][-1]
    return words


# --------------------------------------------------------------------------- the constrained search
def lex_beam_clip(sd, enc, n_layers, scale, W, nbest, maxlen, log_prior, allowed=None, sos_id=0, eos_id=1):
    """enc (T, 512) of one clip -> beam_clip's dict.  allowed(prefix tuple, v) -> bool, or None for every candidate."""
    emb, prj = sd["decoder.tgt_word_emb.weight"], sd["decoder.tgt_word_prj.weight"]
    V = emb.size(0)
    live = [(0, torch.zeros((), dtype=torch.float32), [sos_id])]          # (slot, score, yseq)
    ended = []
    h_tok = np.full((maxlen, W), eos_id, dtype=np.int32)
    h_par = np.tile(np.arange(W, dtype=np.int32), (maxlen, 1))
    h_score = np.full((maxlen, W), -np.inf, dtype=np.float32)
    h_flag = np.zeros((maxlen, W), dtype=np.int32)
    margin = math.inf
    for i in range(maxlen):
        if not live:
            continue
        ys = torch.tensor([y for _, _, y in live], dtype=torch.long)
        n, L = ys.shape
        x = emb[ys] * scale + O.positional_encoding(L).unsqueeze(0)
        causal = torch.ones(L, L, dtype=torch.bool).triu(1).unsqueeze(0).expand(n, -1, -1)
        x = S._layers(sd, x, enc.unsqueeze(0).expand(n, -1, -1), n_layers, causal, None, None)
        local = F.log_softmax(F.linear(x[:, -1], prj), dim=1)          # over all V classes: not renormalised
        if log_prior is not None:
            local = local + log_prior[ys[:, -1]]
        cand = torch.stack([sc for _, sc, _ in live]).unsqueeze(1) + local          # (n, V) fp32
        flat = [(float(cand[a, v]), live[a][0], v, a) for a in range(n) for v in range(V)
                if float(cand[a, v]) > -math.inf and (allowed is None or allowed(tuple(live[a][2][1:]), v))]
        flat.sort(key=lambda c: (-c[0], c[1], c[2]))
        kept = flat[:W]
        for a, b in zip(flat[:W], flat[1:W + 1]):          # adjacent kept ranks, and rank W against rank W + 1
            margin = min(margin, a[0] - b[0])
        nxt = []
        for r, (_, slot, v, a) in enumerate(kept):
            sc, yseq = cand[a, v], live[a][2] + [v]
            if i == maxlen - 1:
                yseq = yseq + [eos_id]
            end = yseq[-1] == eos_id
            h_tok[i, r], h_par[i, r], h_score[i, r], h_flag[i, r] = v, slot, float(sc), 2 if end else 1
            (ended if end else nxt).append((r, sc, yseq))
        live = nxt
    order = sorted(ended, key=lambda e: -float(e[1]))          # stable
    for a, b in zip(order[:nbest], order[1:nbest + 1]):       # adjacent final ranks, and rank nbest against the next one
        margin = min(margin, float(a[1]) - float(b[1]))
    return dict(nbest=[(float(sc), y) for _, sc, y in order[:nbest]], tok=h_tok, par=h_par, score=h_score, flag=h_flag,
                margin=margin, n_ended=len(ended), early=sum(1 for _, _, y in ended if len(y) < maxlen + 2),
                min_live=int((h_flag == 1).sum(1)[:-1].min()) if maxlen > 1 else W)


def allowed_by(words, eos_id=1):
    children, owner = dict_trie(words)
    return lambda prefix, v: (prefix in owner) if v == eos_id else (v in children.get(prefix, ()))


def spelled(y, sos_id=0, eos_id=1):
    """The tokens of a yseq list: entry 0 skipped, cut before the first eos."""
    out = []
    for t in y[1:]:
        if t == eos_id:
            break
        if t != sos_id:
            out.append(t)
    return tuple(out)


def lex_beam_search(sd, enc, n_layers, scale, words, W, nbest, log_prior=None, sos_id=0, eos_id=1):
    """All clips -> beam_oracle.pack's dict with maxlen = longest word + 1, plus cand (N, nbest) int32 and word (N,) int64."""
    maxlen = max(len(w) for w in words) + 1
    owner = dict_trie(words)[1]
    ok = allowed_by(words, eos_id)
    with torch.no_grad():
        clips = [lex_beam_clip(sd, e, n_layers, scale, W, nbest, maxlen, log_prior, ok, sos_id, eos_id) for e in enc]
    out = B.pack(clips, nbest, maxlen, eos_id)
    out["cand"] = np.full((len(clips), nbest), -1, dtype=np.int32)
    for n, c in enumerate(clips):
        for k, (_, y) in enumerate(c["nbest"]):
            out["cand"][n, k] = owner[spelled(y, sos_id, eos_id)]          # a KeyError here: a hypothesis that is no word
    out["word"] = out["cand"][:, 0].astype(np.int64)
    out["maxlen"] = maxlen
    return out


def brute_force(sd, enc, n_layers, scale, words, log_prior=None, sos_id=0, eos_id=1):
    """Teacher-forced score of every DISTINCT word (its lowest index) for one clip enc (T, 512): the sum of the log-softmax
    at the word's tokens and the eos (+ the prior's bigram terms), added in step order in fp32 like the search's totals.
    Returns [(score, word index)] best first (ties: the lower index)."""
    emb, prj = sd["decoder.tgt_word_emb.weight"], sd["decoder.tgt_word_prj.weight"]
    owner = dict_trie(words)[1]
    out = []
    with torch.no_grad():
        for w, idx in owner.items():
            ys = torch.tensor([[sos_id] + list(w)], dtype=torch.long)
            L = ys.size(1)
            x = emb[ys] * scale + O.positional_encoding(L).unsqueeze(0)
            causal = torch.ones(L, L, dtype=torch.bool).triu(1).unsqueeze(0)
            x = S._layers(sd, x, enc.unsqueeze(0), n_layers, causal, None, None)
            local = F.log_softmax(F.linear(x[0], prj), dim=1)
            if log_prior is not None:
                local = local + log_prior[ys[0]]
            sc = torch.zeros((), dtype=torch.float32)
            for i, v in enumerate(list(w) + [eos_id]):
                sc = sc + local[i, v]
            out.append((float(sc), idx))
    return sorted(out, key=lambda c: (-c[0], c[1]))


# --------------------------------------------------------------------------- the end-to-end cases of the GPU tests
# The lexicon sizes Wn = 1, 5 (W = 5: exhaustive), 257 and 1000 with W = 1, 3, 8, 16 on each of the two fixture shapes, and
# one case per shape with the synthetic bigram prior (beam_oracle.make_freq).  nbest = 5 is computed and nbest = 1 is its
# first column (a stable sort: the 1-best of five is the 1-best), so one oracle run and its margins cover both.
# E2E_PICK names, per case (shape, Wn, W, prior), the salt (weights AND clips are re-drawn, as beam_oracle.with_salt does),
# the seed of the word list and the number of clips.  They were picked on the CPU, as beam_oracle.UNSEEN_SALTS was, so that
# every case meets beam_oracle.margin_floor: with 16 kept ranks per step there are some 70 decision gaps per clip and most
# draws have one below the floor, so the W = 16 cases run two clips; and the randomly filled decoder of beam_varied barely
# tells permutations of the same tokens apart (see make_freq), which a beam of 16 over a dense lexicon always holds, so its
# W = 16 cases carry the prior.  test_lex_beam_cpu.py asserts the floor for every entry: no GPU case is skipped or loosened.
E2E_SHAPES = ("beam_small", "beam_varied")
E2E_NBEST = 5
E2E_WORD_LEN = {1: (15, 15), 5: (1, 12), 257: (1, 4), 1000: (1, 4)}          # the single word has 15 tokens: maxlen = 16
PRIOR_SALT = 7
E2E_PICK = {
    ("beam_small", 1, 1, False): (100, 1, 4), ("beam_varied", 1, 1, False): (100, 1, 4),
    ("beam_small", 5, 5, False): (100, 1, 4), ("beam_varied", 5, 5, False): (100, 1, 4),
    ("beam_small", 257, 1, False): (100, 1, 4), ("beam_varied", 257, 1, False): (100, 1, 4),
    ("beam_small", 257, 3, False): (100, 1, 4), ("beam_varied", 257, 3, False): (100, 1, 4),
    ("beam_small", 257, 8, False): (100, 1, 4), ("beam_varied", 257, 8, False): (100, 3, 4),
    ("beam_small", 257, 16, False): (100, 2, 2), ("beam_varied", 257, 16, True): (102, 4, 2),
    ("beam_small", 1000, 1, False): (100, 1, 4), ("beam_varied", 1000, 1, False): (100, 1, 4),
    ("beam_small", 1000, 3, False): (100, 1, 4), ("beam_varied", 1000, 3, False): (100, 3, 4),
    ("beam_small", 1000, 8, False): (100, 1, 4), ("beam_varied", 1000, 8, False): (100, 5, 4),
    ("beam_small", 1000, 16, False): (100, 2, 2), ("beam_varied", 1000, 16, True): (102, 5, 2),
    ("beam_small", 257, 8, True): (104, 2, 4), ("beam_varied", 257, 8, True): (102, 3, 4),
}
E2E_CASES = sorted(E2E_PICK)


def e2e_pick(shape, Wn, W, prior):
    """(salt, word seed, clips) of a case."""
    return E2E_PICK[shape, Wn, W, prior]


def e2e_vocab(shape):
    return S.case_config(B.load_golden(shape + ".npz"))["vocab"]


def e2e_words(shape, Wn, W, prior):
    lo, hi = E2E_WORD_LEN[Wn]
    return make_words(Wn, e2e_vocab(shape), e2e_pick(shape, Wn, W, prior)[1], lo, hi)


def e2e_prior(shape):
    return torch.log(torch.from_numpy(B.make_freq(e2e_vocab(shape), PRIOR_SALT))).float()


def e2e_fixture(shape, salt):
    """The fixture's shape and gains with the weights and clips of `salt`."""
    return B.with_salt(B.load_golden(shape + ".npz"), salt)


@functools.lru_cache(maxsize=None)
def e2e_encoded(shape, salt):
    """(state dict, encoder output of all clips) of a shape and salt, once per process."""
    g = e2e_fixture(shape, salt)
    sd = S.case_state(g)
    with torch.no_grad():
        enc = S.encode(sd, B.case_clips(g), S.case_config(g)["ne"], training=False)
    return sd, enc


@functools.lru_cache(maxsize=None)
def e2e_oracle(shape, Wn, W, prior):
    salt, _, clips = e2e_pick(shape, Wn, W, prior)
    sd, enc = e2e_encoded(shape, salt)
    c = S.case_config(e2e_fixture(shape, salt))
    return lex_beam_search(sd, enc[:clips], c["nd"], c["scale"], e2e_words(shape, Wn, W, prior), W, E2E_NBEST,
                           e2e_prior(shape) if prior else None)


def first_k(ref, k):
    """The oracle's result for nbest = k <= E2E_NBEST from the one computed with E2E_NBEST."""
    out = dict(ref)
    for key in ("yseq", "lengths", "scores", "cand"):
        out[key] = ref[key][:, :k]
    out["n_hyps"] = np.minimum(ref["n_hyps"], k)
    return out


# --------------------------------------------------------------------------- the tail alone: planted tables and states
U64 = 2 ** 64 - 1
TAIL_N, TAIL_MAXLEN, TAIL_EOS, TAIL_SCALE, TAIL_P = 3, 6, 1, 0.25, 6
TAIL_SHAPES = [(5, 1), (5, 3), (42, 16), (64, 1), (64, 16)]
TAIL_STEPS = (2, TAIL_MAXLEN - 1)


def planted_trie(V, eos, rng):
    """Six nodes that no lexicon needs to produce (the kernel only reads tables): 0 many tokens and eos; 1 only eos; 2 only
    token V - 1; 3 nothing; 4 many tokens, no eos, and (V < 64) every bit at and above V, which no lane may take; 5 a few
    tokens.  first: the children of 0 inside the table, of 2 at 5, of 4 past the end (clamped to P - 1), of 5 negative
    (clamped to 0)."""
    def some(k):
        return sum(1 << int(t) for t in rng.choice([t for t in range(V) if t != eos], size=min(k, V - 1), replace=False))
    mask = [some(V // 2 + 1) | 1 << eos, 1 << eos, 1 << (V - 1), 0, some(V // 2 + 1) | ((U64 >> V) << V if V < 64 else 0), some(3)]
    return mask, [1, 0, 5, 0, 4, -40]


def tail_ref(y, w, lp, score, last, node, mask, first, anc_old, step, maxlen, eos, W):
    """float64 restatement of sbl_beam_tail_lex for N clips (include/sbl_hip.h) -> dict of expected outputs."""
    Sn, V, P = y.shape[0], w.shape[0], len(mask)
    N = Sn // W
    logits = y.astype(np.float64) @ w.astype(np.float64).T
    mx = logits.max(1, keepdims=True)
    local = logits - mx - np.log(np.exp(logits - mx).sum(1, keepdims=True))          # over all V classes
    if lp is not None:
        local = local + lp.astype(np.float64)[last]
    q = np.clip(node, 0, P - 1)
    out = dict(tok=np.full((N, W), eos, np.int32), par=np.tile(np.arange(W, dtype=np.int32), (N, 1)), score=np.full((N, W), -np.inf),
               flag=np.zeros((N, W), np.int32), node=np.zeros((N, W), np.int32), ended=[[] for _ in range(N)],
               anc=np.zeros((Sn, step + 1), np.int32), gap=np.inf, n_cand=[])
    for n in range(N):
        cand = [(score[n * W + r] + local[n * W + r, v], r, v) for r in range(W) for v in range(V)
                if score[n * W + r] > -np.inf and (mask[q[n * W + r]] >> v) & 1]
        cand = sorted([c for c in cand if c[0] > -np.inf], key=lambda c: (-c[0], c[1], c[2]))
        out["n_cand"].append(len(cand))
        for a, b in zip(cand[:W], cand[1:W + 1]):
            if a[0] != b[0]:
                out["gap"] = min(out["gap"], a[0] - b[0])
        for r, (sc, par, v) in enumerate(cand[:W]):
            end = v == eos or step == maxlen - 1
            out["tok"][n, r], out["par"][n, r], out["score"][n, r], out["flag"][n, r] = v, par, sc, 2 if end else 1
            p = int(q[n * W + par])
            out["node"][n, r] = p if v == eos else min(max(first[p] + bin(mask[p] & ~(1 << eos) & ((1 << v) - 1)).count("1"), 0), P - 1)
            if end:
                out["ended"][n].append((sc, step * W + r))
        for r in range(W):
            ps = n * W + out["par"][n, r]
            out["anc"][n * W + r, :step] = anc_old[ps, :step]
            out["anc"][n * W + r, step] = ps
    return out


def tail_case(V, W):
    """The head, the planted table and, per step of TAIL_STEPS, the state before the launch with tail_ref's expectation
    and the names of the planted situations that the expectation shows (asserted here, so the data cannot drift away
    from what it is for).  Planted: a slot whose node allows only eos; a node whose only child is token V - 1 (63 at
    V = 64); a dead slot; a clip with fewer candidates than W; a clip whose every node has an all-zero mask, where nothing
    is kept; two parents that are exact copies and lead (lower parent first, then lower token); nodes out of range on
    input; children that clamp at the end of the table."""
    N, maxlen, eos, P = TAIL_N, TAIL_MAXLEN, TAIL_EOS, TAIL_P
    Sn = N * W
    rng = np.random.RandomState(300 * V + W)
    w = (rng.randn(V, 512) * 0.05).astype(np.float32)
    emb = rng.randn(V, 512).astype(np.float32)
    lp = (rng.randn(V, V) * 2).astype(np.float32)
    lp[rng.rand(V, V) < 0.2] = -np.inf
    lp[:, eos] = 2.0
    lp[:, V - 1] = 1.0
    mask, first = planted_trie(V, eos, rng)
    steps = []
    for step in TAIL_STEPS:
        y = rng.randn(Sn, 512).astype(np.float32)
        score = (-rng.rand(Sn) * 10).astype(np.float32)
        last = rng.randint(2, V, Sn).astype(np.int32)
        node = rng.choice([0, 4, 5], size=Sn).astype(np.int32).reshape(N, W)
        counts = np.array([0, 2, 5], np.int32)
        if W == 1:
            node[:, 0] = [0, 3, P + 5] if step == 2 else [1, 2, -3]
        elif step == 2:
            node[0, :3] = [0, 1, 4]                       # clip 0: a normal slot, one that may only end, a dead one
            score[2] = -np.inf
            node[1] = 3                                   # clip 1: two candidates in all: the single child V - 1, an eos
            node[1, :2] = [2, 1]
            node[2, :2] = 4                               # clip 2: slots 0 and 1 are exact copies and lead
            score[2 * W] = 20.0
            y[2 * W + 1], score[2 * W + 1], last[2 * W + 1] = y[2 * W], score[2 * W], last[2 * W]
            node[2, 2] = P + 5                            # out of range: read as P - 1 ...
            if W > 3:
                node[2, 3] = -3                           # ... and as 0
        else:
            node[0] = 3                                   # clip 0: all-zero masks, nothing is kept
            node[1, :2] = [1, 2]
            node[2, :3] = [-3, 2, P + 5]
        node = node.reshape(-1)
        anc_old = rng.randint(0, Sn, (Sn, maxlen)).astype(np.int32)
        ref = tail_ref(y, w, lp, score, last, node, mask, first, anc_old, step, maxlen, eos, W)
        assert ref["gap"] > 1e-4, "test data: a near tie that float32 may order either way"
        fin = ref["flag"] != 0
        saw = set()
        if W == 1 and step == 2:
            assert ref["flag"][1, 0] == 0 and ref["n_cand"][1] == 0
            saw.update(["all-zero mask", "node out of range"])
        elif W == 1:
            assert ref["tok"][0, 0] == eos and ref["node"][0, 0] == 1 and ref["tok"][1, 0] == V - 1 and ref["node"][1, 0] == 5
            saw.update(["only eos", "only child V - 1", "node out of range"])
        elif step == 2:
            assert ref["n_cand"][1] == 2 and sorted(ref["tok"][1, :2].tolist()) == [eos, V - 1] and (ref["flag"][1, 2:] == 0).all()
            assert np.all(ref["node"][1, 2:] == 0)
            saw.update(["only eos", "only child V - 1", "fewer candidates than W"])
            assert not (ref["par"][0][fin[0]] == 2).any()
            saw.add("dead slot")
            assert ref["score"][2, 0] == ref["score"][2, 1] and ref["par"][2, :2].tolist() == [0, 1] and ref["tok"][2, 0] == ref["tok"][2, 1]
            if W >= 4:                                    # the copies' second-best token: again parent 0 first
                assert ref["score"][2, 2] == ref["score"][2, 3] and ref["par"][2, 2:4].tolist() == [0, 1]
            saw.add("parent tie")
            assert (ref["node"][2][fin[2]] == P - 1).any(), "the children of node 4 clamp to P - 1"
            saw.add("node out of range")
        else:
            assert ref["n_cand"][0] == 0 and (ref["flag"][0] == 0).all()
            saw.add("all-zero mask")
            assert np.all(ref["flag"][fin] == 2)
        steps.append(dict(step=step, y=y, score=score, last=last, node=node, counts=counts, anc_old=anc_old, ref=ref, saw=saw))
    return dict(w=w, emb=emb, lp=lp, mask=mask, first=first, steps=steps)
