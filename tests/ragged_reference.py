"""float64 attention with a key count per entry: the restatement of sbl_attention_seg_len_fwd (include/sbl_hip.h) that the
ragged tests compare with.  It is tests/attention_routes.py with one rule added - sequence b sees key j iff
j < min(max(kv_len[b // kv_group], 0), Lk) - and it introduces no tolerance of its own: problems(), documented_mask_index(),
forward_problem(), compare() and the error bounds are that module's.  numpy only.

The keys at or behind the count are not part of a problem at all: forward_problem gets the visible K/V rows only, as the
kernels never load the others.  So the restatement on a full K/V equals itself on K/V cut to the count bit for bit, whatever
the cut rows hold, and the bound counts the MFMA steps of the visible key tiles only.  The dropout keep mask is drawn at the
indices of the FULL layout (Lk keys), which is what the header promises."""
import numpy as np

import attention_routes as A
from sbl_for_multilingual_lip_reading_amd import detfill


def case(name, B, H, segL, Lk, kvg=1):
    """An attention_routes.Case of the new entry: Lk >= 1 cross-attention (B // kvg K/V entries), Lk == 0 self-attention."""
    assert B % kvg == 0 and (Lk > 0 or (len(segL) == 1 and kvg == 1))
    return A.Case(name, "grouped" if Lk else "seg", B, H, tuple(segL), Lk, None, kvg, (), None, None)


def route(c):
    """The kernel the host picks, from the shapes alone (attention.hip, sbl_attention_seg_len_fwd: the grouped entry's
    dispatch, self-attention by seg_L[0])."""
    return A.route_fwd(c.segL, c.Lk, 0).kernel


def n_entries(c):
    return c.B // c.kvg


def clamp(kv_len, c, pr):
    return int(min(max(int(kv_len[pr["b"] // c.kvg]), 0), pr["Lk"]))


def make_inputs(c):
    """float32 q (rows_q, H*64), k, v (rows_k, H*64), uniform in [-1, 1); self-attention: k / v have q's rows."""
    HD = c.H * 64
    return {n: detfill.uniform("ragged.%s.%s" % (c.name, n), (r, HD)) for n, r in (("q", A.rows_q(c)), ("k", A.rows_k(c)), ("v", A.rows_k(c)))}


def reference(c, inp, kv_len, drop_p=0.0, seed=0, offset=0):
    """(o, bound) in float64, (rows_q, H*64).  A sequence without a visible key: o = 0 with bound 0 (exact)."""
    assert len(kv_len) == n_entries(c)
    q, k, v = (inp[n].astype(np.float64) for n in ("q", "k", "v"))
    ks = float(A.keep_scale(drop_p)) if drop_p else 1.0
    O, EO = np.zeros((A.rows_q(c), c.H * 64)), np.zeros((A.rows_q(c), c.H * 64))
    for pr in A.problems(c):
        n = clamp(kv_len, c, pr)
        if n == 0:
            continue
        cols = slice(pr["h"] * 64, pr["h"] * 64 + 64)
        vis = np.ones((pr["Lq"], n), dtype=bool)
        keep = vis
        if drop_p:
            keep = A.keep_mask(seed, offset, A.documented_mask_index(c, pr), drop_p)[:, :n]
        r = A.forward_problem(q[pr["qrows"], cols], k[pr["krows"][:n], cols], v[pr["krows"][:n], cols], vis, keep, ks)
        O[pr["qrows"], cols], EO[pr["qrows"], cols] = r[5], A.SLACK * (r[6] + A.TINY)
    return O, EO


def trimmed(c, inp, kv_len, entry):
    """The case and inputs of K/V entry `entry` alone with its K/V cut to its count n >= 1: the entry's kv_group sequences
    (self-attention: the one sequence) of every segment, in the (segment, b, l) row order, against n key rows.  Returns
    (case, inputs, rows): rows = where the sub-problem's q rows sit in the full q."""
    n = int(min(max(int(kv_len[entry]), 0), c.Lk or c.segL[0]))
    assert n >= 1
    sub = case("%s.e%d" % (c.name, entry), c.kvg, c.H, c.segL, n, c.kvg)
    rows, row = [], 0
    for L in c.segL:
        for b in range(entry * c.kvg, (entry + 1) * c.kvg):
            rows.extend(range(row + b * L, row + (b + 1) * L))
        row += c.B * L
    rows = np.array(rows)
    krows = entry * c.Lk + np.arange(n) if c.Lk else rows[:n]
    return sub, dict(q=inp["q"][rows], k=inp["k"][krows], v=inp["v"][krows]), rows
