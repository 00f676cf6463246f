"""The dropout sites of a step as the host issued them: a recorder of every launch that takes a stream offset, the table of
the element indices each such entry point draws, and audits of the resulting ledger.  No GPU is needed to import or to
audit; the recorder only wraps the Python launch entry (it adds no launch and no synchronisation).

A dropout decision is sbl_rand_u32(seed, offset, idx) (csrc/sbl_common.h): the hash of seed + C1 * (offset + 1) + C2 * idx in
wrap-around 64-bit arithmetic.  C2 is odd, so that sum is seed + C2 * u with

    u = (offset + 1) * C1 * C2^-1 + idx   (mod 2^64),

the draw's CANONICAL POSITION: under one seed two draws are the same random number exactly when their u is equal.  Folded
stage offsets (decoder_stages._fold) and the whole-buffer offsets of the batched backward become comparable without
un-folding: audit_disjoint() asks that no two forward sites share a position, audit_backward() that every position backward
regenerates was drawn in forward and the other way round.

The index table (INDEX_TABLE) is written from include/sbl_hip.h and the restatements in tests/attention_routes.py
(p_offsets, mask_index_full, mask_index_ends) and tests/decoder_rows_reference.py (stage_rows, ends_table); nothing is taken
from transformer/decoder_stages.py, which is the code under test.
"""
import contextlib
import ctypes

import numpy as np

import attention_routes as AR

C1 = 0x9E3779B97F4A7C15
C2 = 0xD1B54A32D192ED03
M64 = (1 << 64) - 1
KC = (C1 * pow(C2, -1, 1 << 64)) & M64          # C1 * C2^-1
DEFAULT_SEED = 0x5B1C0FFEE                      # ops.DropoutState
RANK_FOLD = 0x9E3779B97F4A7C15
BUMP_MUL, BUMP_ADD = 6364136223846793005, 1442695040888963407      # sbl_seed_bump


def canon(offset, idx=0):
    """Canonical position of element idx of the stream `offset`."""
    return ((int(offset) + 1) * KC + int(idx)) & M64


def fold(offset, base):
    """The stream offset under which element i draws what element base + i of stream `offset` draws (restated from the
    affine form of the hash, not imported): (offset' + 1) * C1 = (offset + 1) * C1 + base * C2."""
    return ((int(offset) + 1 + int(base) * ((C2 * pow(C1, -1, 1 << 64)) & M64)) - 1) & M64


def unfold(folded, base):
    """Inverse of fold() in its first argument."""
    return ((int(folded) + 1 - int(base) * ((C2 * pow(C1, -1, 1 << 64)) & M64)) - 1) & M64


def rank_seed(rank):
    """The default seed of data-parallel rank `rank` (ops.DropoutState.__init__)."""
    return DEFAULT_SEED ^ ((rank * RANK_FOLD) & 0x7FFFFFFFFFFFFFFF)


def bumped(seed):
    """sbl_seed_bump in uint64."""
    return (int(seed) * BUMP_MUL + BUMP_ADD) & M64


# --------------------------------------------------------------------------- index table
def _rows_full(B, segL):
    return B * int(sum(segL))


def _ends_full_rows(B, segL):
    """decoder.ends_rows restated: segment s keeps positions 0 and L-1 of every sequence, (b, k) order."""
    rows, row0 = [], 0
    for L in segL:
        rows += [row0 + b * L + k * (L - 1) for b in range(B) for k in range(min(2, L))]
        row0 += B * L
    return rows


def _merge(ranges):
    out = []
    for a, b in sorted(ranges):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [(a, b) for a, b in out]


def _one(n):
    return [(0, int(n))]


def _idx_rows(ints):                  # (M, D): element m * D + c
    return _one(ints[-2] * ints[-1])


def _idx_seg_rows(ints):              # (B, segL, nseg, D): the stage's rows in (segment, b, l) order
    B, segL, _, D = ints[-4:]
    return _one(_rows_full(B, segL) * D)


def _idx_ends_rows(ints):             # compact rows draw at their FULL row
    B, segL, _, D = ints[-4:]
    return _merge((r * D, (r + 1) * D) for r in _ends_full_rows(B, segL))


def _idx_att(ints):                   # (B, H, Lq, Lk): ((h * B + b) * Lq + i) * Lk + j
    B, H, Lq, Lk = ints[-4:]
    return _one(H * B * Lq * Lk)


def _idx_att_seg(ints):               # (B, H, segL, nseg, Lk_fixed): the segments' (H*B, L, Lk) blocks back to back
    B, H, segL, _, Lk = ints[-5:]
    return _one(AR.p_offsets(segL, B, H, Lk)[1])


def _idx_att_ends(ints):              # compact query kk of sequence (s, b) draws as position kk * (L - 1) of the full layout
    B, H, segL, _, Lk = ints[-5:]
    out = []
    for s, L in enumerate(segL):
        for h in range(H):
            for b in range(B):
                for kk in range(min(2, L)):
                    a = AR.mask_index_ends(segL, B, H, Lk, s, h, b, kk, 0)
                    out.append((a, a + Lk))
    return _merge(out)


def _idx_emb(ints):                   # (ld, B, segL, nseg, D, V): sbl_dropout's indexing over the stage's rows
    _, B, segL, _, D, _ = ints
    return _one(_rows_full(B, segL) * D)


# entry -> (phase, function of the launch's integer arguments -> sorted disjoint [start, stop) index ranges)
INDEX_TABLE = {
    "sbl_dropout": (None, lambda ints: _one(ints[0])),
    "sbl_add_layernorm_fwd": ("fwd", _idx_rows),
    "sbl_add_layernorm_bwd": ("bwd", _idx_rows),
    "sbl_add_layernorm2_fwd": ("fwd", _idx_rows),
    "sbl_add_layernorm2_fusion_fwd": ("fwd", _idx_seg_rows),
    "sbl_add_layernorm2_ends_fwd": ("fwd", _idx_ends_rows),
    "sbl_add_layernorm_ends_bwd": ("bwd", _idx_ends_rows),
    "sbl_attention_fwd": ("fwd", _idx_att),
    "sbl_attention_bwd": ("bwd", _idx_att),
    "sbl_attention_seg_fwd": ("fwd", _idx_att_seg),
    "sbl_attention_seg2_fwd": ("fwd", _idx_att_seg),
    "sbl_attention_seg_bwd": ("bwd", _idx_att_seg),
    "sbl_attention_seg_grouped_fwd": ("fwd", lambda ints: _idx_att_seg(ints[:-1])),
    "sbl_attention_seg_len_fwd": ("fwd", lambda ints: _idx_att_seg(ints[:-1])),
    "sbl_attention_ends2_fwd": ("fwd", _idx_att_ends),
    "sbl_attention_ends_bwd": ("bwd", _idx_att_ends),
    "sbl_embed_pe_drop2_fwd": ("fwd", _idx_emb),
}


class Record:
    """One (launch, offset): entry name, p, the offset, whether the seed pointer was null, the launch's integer arguments
    (a host segment array counts as one, a tuple), which of the launch's offsets this is (0 / 1) and the phase it ran in."""

    def __init__(self, name, p, offset, null_seed, ints, slot=0, phase="fwd"):
        self.name, self.p, self.offset, self.null_seed = name, float(p), int(offset) & M64, bool(null_seed)
        self.ints, self.slot, self.phase = tuple(ints), slot, phase

    def ranges(self):
        return INDEX_TABLE[self.name][1](self.ints)

    def count(self):
        return sum(b - a for a, b in self.ranges())

    def uranges(self):
        """The canonical positions drawn, as [start, stop) ranges of ints in [0, 2^64] (a range that wraps is split)."""
        base = canon(self.offset)
        out = []
        for a, b in self.ranges():
            lo = (base + a) & M64
            hi = lo + (b - a)
            if hi <= M64 + 1:
                out.append((lo, hi))
            else:
                out += [(lo, M64 + 1), (0, hi - (M64 + 1))]
        return out

    def __repr__(self):
        return "Record(%s, p=%g, offset=%d, slot=%d, %s, ints=%s)" % (self.name, self.p, self.offset, self.slot, self.phase, self.ints)


class Ledger(list):
    """The records of one step in host issue order.  `phase` is what the recorder stamps on new records."""
    phase = "fwd"

    @contextlib.contextmanager
    def backward(self):
        prev, self.phase = self.phase, "bwd"
        try:
            yield self
        finally:
            self.phase = prev

    def fwd(self, live=True):
        return [r for r in self if r.phase == "fwd" and (r.p > 0 or not live)]

    def bwd(self, live=True):
        return [r for r in self if r.phase == "bwd" and (r.p > 0 or not live)]


def records_of(name, args, signature, phase):
    """The Records of one launch (none if the entry takes no offset)."""
    from sbl_for_multilingual_lip_reading_amd import _lib
    u = [i for i, t in enumerate(signature) if t is _lib.U64]
    if not u:
        return []
    assert name in INDEX_TABLE, "entry %s takes a stream offset and has no row in INDEX_TABLE" % name
    assert signature[u[0] - 1] is _lib.P and signature[u[0] - 2] is _lib.F, name      # ..., drop_p, seed, offset[, offset]
    ints = []
    for a, t in zip(args, signature):
        if isinstance(a, ctypes.Array):
            ints.append(tuple(int(v) for v in a))
        elif t in (_lib.I, _lib.L) and not isinstance(a, bool):
            ints.append(int(a))
    table_phase = INDEX_TABLE[name][0]
    return [Record(name, args[u[0] - 2], args[i], args[u[0] - 1] is None, ints, slot, table_phase or phase) for slot, i in enumerate(u)]


@contextlib.contextmanager
def recording(ledger=None):
    """Wrap the launch entry (_lib.call and the name ops binds to it) for the duration of the block; yields the Ledger."""
    from sbl_for_multilingual_lip_reading_amd import _lib, ops
    led = Ledger() if ledger is None else ledger
    inner = _lib.call

    def call(name, *args):
        sig = _lib.SIGNATURES.get(name)
        if sig is not None:
            led.extend(records_of(name, args, sig, led.phase))
        return inner(name, *args)

    saved = (_lib.call, ops.call)
    _lib.call = ops.call = call
    try:
        yield led
    finally:
        _lib.call, ops.call = saved


# --------------------------------------------------------------------------- audits
def audit_disjoint(ledger):
    """(a) the canonical ranges of all forward launches with p > 0 are pairwise disjoint -> list of offending record pairs."""
    spans = sorted(((a, b, k) for k, r in enumerate(ledger.fwd()) for a, b in r.uranges()), key=lambda t: (t[0], t[1]))
    recs = ledger.fwd()
    bad, reach, who = [], -1, None
    for a, b, k in spans:
        if a < reach:
            bad.append((recs[who], recs[k]))
        if b > reach:
            reach, who = b, k
    return bad


def audit_backward(ledger):
    """(b) the union of the backward launches' canonical ranges equals that of the forward launches (p > 0 on both sides)
    -> (ranges backward draws that forward never drew, ranges forward drew that backward never regenerates)."""
    f = _merge(u for r in ledger.fwd() for u in r.uranges())
    b = _merge(u for r in ledger.bwd() for u in r.uranges())
    return _minus(b, f), _minus(f, b)


def _minus(xs, ys):
    out, j = [], 0
    for a, b in xs:
        while a < b:
            while j < len(ys) and ys[j][1] <= a:
                j += 1
            if j == len(ys) or ys[j][0] >= b:
                out.append((a, b))
                break
            if ys[j][0] > a:
                out.append((a, ys[j][0]))
            a = ys[j][1]
    return out


def audit_seed(ledger):
    """(c) no launch with p > 0 has a null seed -> offending records."""
    return [r for r in ledger if r.p > 0 and r.null_seed]


def audit(ledger, backward=True):
    """All three audits; raises AssertionError naming the offenders."""
    bad = audit_disjoint(ledger)
    assert not bad, "forward sites share random numbers: %s" % (bad[:4],)
    assert not audit_seed(ledger), "p > 0 with a null seed: %s" % (audit_seed(ledger)[:4],)
    if backward:
        extra, missing = audit_backward(ledger)
        assert not extra, "backward draws with no forward twin (canonical ranges): %s" % (extra[:4],)
        assert not missing, "forward draws backward never regenerates (canonical ranges): %s" % (missing[:4],)


# --------------------------------------------------------------------------- masks
def mask(seed, offset, indices, p):
    """bool keep decisions of the elements `indices` of stream `offset` (attention_routes.keep_mask)."""
    return AR.keep_mask(int(seed) & M64, int(offset) & M64, np.asarray(indices, dtype=np.uint64), p)


def mask_range(seed, offset, start, n, p):
    return mask(seed, offset, np.arange(int(start), int(start) + int(n), dtype=np.uint64), p)


def keep_scale(p):
    """float32(1) / (float32(1) - float32(p)), as sbl_dropout forms it."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))
