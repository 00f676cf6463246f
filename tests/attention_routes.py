"""The host dispatch of csrc/attention.hip restated in Python, the case table of the route-aware attention tests, a float64
reference of forward and backward with an explicit dropout keep mask, per-output error bounds, and a float32 emulation that
exists only to check the bounds and the table on the CPU.  numpy only: no torch, no GPU.

Routes.  route_fwd / route_seg2 / route_grouped / route_bwd / route_ends_fwd / route_ends_bwd follow the entry points of
attention.hip line by line and return the leaf a call lands on:

    Leaf(entry, kernel, tiles, kv, red, waves, fallback)
      entry     "seg" sbl_attention_seg_fwd / _bwd (and the uniform sbl_attention_fwd / _bwd, which forward to them)
                "dual" sbl_attention_seg2_fwd's own launch | "two" its two-launch fallback | "grouped" | "ends"
      kernel    "small" one wavefront per problem | "qtile" 16-row query tiles of one sequence on the same kernel
                | "workgroup" the 256-thread kernel that stages operands in LDS
      tiles     key tiles: 16-key tiles of the one-wavefront kernels (NT), 32-key tiles of the workgroup kernel (TK): 1 | 2
      kv        "self" | "cross" | "grouped"
      red       reduction of dK / dV over the segments (or tiles) that share keys: "none" | "lds" | "atomics"
      waves     wavefronts per workgroup
      fallback  why the call left the kernel its sizes would take, or None
Every threshold is a copy; the comment next to it names the line it mirrors.  CASES carries, next to each shape, the
leaves it is meant to hit, written by hand (never computed by the route functions); tests/test_attention_routes_cpu.py
checks route(case) == case leaf and that the table reaches every reachable leaf of all_leaves().

Dropout.  rand_u32 / drop_thresh restate sbl_rand_u32 / sbl_drop_thresh of csrc/sbl_common.h; mask_index_full / _qtile /
_ends give the index sbl_keep is documented to draw for probability (segment, h, b, i, j).  They are derived from the layout
documentation of include/sbl_hip.h (the probability blocks are (H*B, L, Lk), back to back over the segments; "the dropout
mask index is the element's place in the probability layout"; the ends kernels draw "the decision of the full-layout kernels
for the same element", compact row k standing for full row k*(L-1)), not from the kernels' index expressions.

Bounds.  U = 2^-24.  Every output gets a first-order forward error bound from float64 sums of absolute values of its terms
(derivations next to the constants below), times SLACK = 2 for the second-order terms.  The one term that cannot be derived is
the relative error of __expf (x * log2(e) rounded, then v_exp_f32): measured on an MI355X on 2026-10-19 with a stand-alone
program that compares __expf with float64 exp at 2^23 points of [-104, 0]: worst |err| / ((|x| + 2) * U * exp(x)) =
EXPF_MEASURED = 1.176742 (55.0 U at x = -44.74; 2.9 U at most on [-2, 0]); the bounds allow twice that (EXPF_C).  Every result
below 2^-126 came back as exactly 0 (worst absolute error 1.0 * 2^-126); the bounds carry an absolute TINY = 2^-125 for that,
on p and on every later float32 value that a product of small numbers can push below 2^-126 (pd, ds and the outputs).
"""
import collections
import itertools

import numpy as np

from sbl_for_multilingual_lip_reading_amd import detfill

Leaf = collections.namedtuple("Leaf", "entry kernel tiles kv red waves fallback")
Case = collections.namedtuple("Case", "name entry B H segL Lk mask kvg flags fwd bwd")

MAX_SEG = 16                        # sbl_common.h: SBL_MAX_SEG
SCALE = 0.125
U = 2.0 ** -24
TINY = 2.0 ** -125                  # a probability whose exp fell below 2^-126 may be flushed or denormal-rounded
SLACK = 2.0                         # second-order terms of the first-order bounds below
EXPF_MEASURED = 1.176742            # worst measured |err| / ((|x| + 2) U exp(x)) of __expf on gfx950 (at x = -44.74: 55.0 U)
EXPF_C = 2 * EXPF_MEASURED          # the margin the bounds allow
C_DOT64 = 66                        # 64-term fp32 contraction over the head dim (<= 64 U sum|terms|) + the scale multiply + 1
C_SUM = 12                          # softmax row sum: 6-level shuffle tree (workgroup) or 8 serial adds + 2 levels (small), <= 10 U,
                                    # then one division (workgroup) or reciprocal + multiply (small): <= 2 U


# ------------------------------------------------------------------------------------------------ host dispatch
def small_ok(segL, Lk_fixed, mask_kind):
    """attention.hip at_small_ok"""
    if mask_kind == 2 or Lk_fixed > 32:
        return False
    return all(L <= 16 for L in segL)


def qtile_ok(segL, Lk_fixed, mask_kind):
    """attention.hip at_qtile_ok"""
    return len(segL) == 1 and mask_kind != 2 and 16 < segL[0] <= 32 and Lk_fixed <= 32


def _kv(Lk_fixed):
    return "cross" if Lk_fixed > 0 else "self"


def _tiles16(segL, Lk_fixed):
    """NT of the one-wavefront kernels: `Lk > 16 ? 2 : 1`, the largest over the problems of the launch"""
    return 2 if (Lk_fixed or max(segL)) > 16 else 1


def _tiles32(segL, Lk_fixed):
    """TK = Lkp >> 5 of the workgroup kernels, the largest over the problems of the launch"""
    return ((Lk_fixed or max(segL)) + 31) // 32


def _why_workgroup(segL, Lk_fixed, mask_kind):
    """Which condition of at_small_ok / at_qtile_ok sends the sizes to the workgroup kernel (None: they would pass)."""
    if mask_kind == 2:
        return "tensor-mask"
    if Lk_fixed > 32:
        return "keys>32"
    if max(segL) > 32:
        return "rows>32"
    if len(segL) > 1 and max(segL) > 16:
        return "multiseg>16"
    return None


def route_fwd(segL, Lk_fixed, mask_kind, o_aligned=True, entry="seg", kv=None):
    """sbl_attention_seg_fwd (sbl_attention_fwd forwards to it with seg_L = {Lq}, Lk_fixed = Lk)"""
    kv = kv or _kv(Lk_fixed)
    if small_ok(segL, Lk_fixed, mask_kind):                 # `if (at_small_ok(d, Lk_fixed, mask_kind))`: 4 problems per workgroup
        return Leaf(entry, "small", _tiles16(segL, Lk_fixed), kv, "none", 4, None)
    if qtile_ok(segL, Lk_fixed, mask_kind) and o_aligned:   # `if (at_qtile_ok(d, Lk_fixed, mask_kind) && sbl_aligned16(o))`
        return Leaf(entry, "qtile", _tiles16(segL, Lk_fixed), kv, "none", 4, None)
    why = _why_workgroup(segL, Lk_fixed, mask_kind) or "o-unaligned"
    return Leaf(entry, "workgroup", _tiles32(segL, Lk_fixed), kv, "none", 4, why)      # attention_fwd_kernel, dim3(256)


def route_seg2(segL, Lk_fixed, mask_kind):
    """sbl_attention_seg2_fwd: `if (!at_small_ok(d, Lk_fixed, mask_kind))` two plain launches, else the dual launch"""
    if not small_ok(segL, Lk_fixed, mask_kind):
        return route_fwd(segL, Lk_fixed, mask_kind, True, "two")
    return Leaf("dual", "small", _tiles16(segL, Lk_fixed), _kv(Lk_fixed), "none", 4, None)


def route_grouped(segL, Lk_fixed):
    """sbl_attention_seg_grouped_fwd: `small || at_qtile_ok(d, Lk_fixed, 0)`, else attention_grouped_fwd_kernel"""
    assert Lk_fixed >= 1
    return route_fwd(segL, Lk_fixed, 0, True, "grouped", "grouped")


def route_bwd(segL, Lk_fixed, ldd_mult4=True, grads_aligned=True):
    """sbl_attention_seg_bwd.  ldd_mult4: lddq, lddk, lddv are multiples of 4 floats; grads_aligned: dq, dk, dv 16-byte aligned"""
    kv, nseg = _kv(Lk_fixed), len(segL)
    vec = ldd_mult4 and grads_aligned
    shared = Lk_fixed > 0 and nseg > 1
    if small_ok(segL, Lk_fixed, 0) and vec:                 # `if (at_small_ok(d, Lk_fixed, 0) && lddq % 4 == 0 && ... aligned16(dv))`
        if shared:                                          # `if (Lk_fixed > 0 && nseg > 1)`: attention_small_bwd_kernel<true>
            return Leaf("seg", "small", _tiles16(segL, Lk_fixed), kv, "lds", min(nseg, 8), None)      # `nwv = nseg < 8 ? nseg : 8`
        return Leaf("seg", "small", _tiles16(segL, Lk_fixed), kv, "none", 4, None)
    if qtile_ok(segL, Lk_fixed, 0) and vec:                 # `if (at_qtile_ok(d, Lk_fixed, 0) && lddq % 4 == 0 && ...)`: dim3(128)
        return Leaf("seg", "qtile", _tiles16(segL, Lk_fixed), kv, "lds", 2, None)
    why = _why_workgroup(segL, Lk_fixed, 0) or ("grad-stride" if not ldd_mult4 else "grad-unaligned")
    red = "atomics" if shared else "none"                   # `if (Lk_fixed > 0 && nseg > 1)`: hipMemset2DAsync + kv_atomic
    return Leaf("seg", "workgroup", _tiles32(segL, Lk_fixed), kv, red, 4, why)


def route_ends_fwd(segL, Lk_fixed):
    """sbl_attention_ends2_fwd: always attention_small2_ends_fwd_kernel (at_ends_check: 1 <= Lk_fixed <= 32)"""
    assert 1 <= Lk_fixed <= 32
    return Leaf("ends", "small", _tiles16((2,), Lk_fixed), "cross", "none", 4, None)


def route_ends_bwd(segL, Lk_fixed):
    """sbl_attention_ends_bwd: `if (nseg > 1)` the shared-keys form on min(nseg, 8) wavefronts, else the plain one"""
    assert 1 <= Lk_fixed <= 32
    nseg = len(segL)
    if nseg > 1:
        return Leaf("ends", "small", _tiles16((2,), Lk_fixed), "cross", "lds", min(nseg, 8), None)
    return Leaf("ends", "small", _tiles16((2,), Lk_fixed), "cross", "none", 4, None)


def route_case(c):
    """(forward leaf, backward leaf or None) of a table case"""
    mk = {None: 0, "causal": 1, "tensor": 2}[c.mask]
    if c.entry == "seg":
        return (route_fwd(c.segL, c.Lk, mk, "o_off1" not in c.flags),
                route_bwd(c.segL, c.Lk, "gstride2" not in c.flags, "dq_off1" not in c.flags))
    if c.entry == "seg2":
        return route_seg2(c.segL, c.Lk, mk), None
    if c.entry == "grouped":
        return route_grouped(c.segL, c.Lk), None
    return route_ends_fwd(c.segL, c.Lk), route_ends_bwd(c.segL, c.Lk)


def _domain_segs():
    singles = [(L,) for L in range(1, 65)]
    # 2, 3, 5, 8, 9 and 16 segments: below, at and above the 8-wavefront cap of the shared-keys backward kernels
    multi = [(5, 16), (5, 16, 1), (5, 20, 1), (12, 20), (5, 40), (33, 2, 64), tuple(range(1, 9)), tuple(range(1, 10)),
             tuple(range(1, 17)), (1,) * 16, (16,) * 5, (17,) * 3, (32, 1) * 8]
    return singles + multi


def all_leaves():
    """{"fwd": {leaf: reachable}, "bwd": {leaf: reachable}} over the whole product of leaf field values.  A leaf is reachable
    when some argument list the ABI accepts lands on it: every segment list of _domain_segs() (all single lengths 1..64 and
    multi-segment lists on each side of the 16 / 32 thresholds and of the 8-wavefront cap), every Lk_fixed 0..64, the three
    mask kinds (a tensor mask as the library's callers pass it: one segment, through sbl_attention_fwd, so Lk_fixed > 0), both
    alignments of o and both of the gradient conditions."""
    fwd, bwd = set(), set()
    for segL in _domain_segs():
        for Lk in range(0, 65):
            for mk in (0, 1, 2):
                if mk == 2 and (len(segL) > 1 or Lk == 0):
                    continue
                for oa in (True, False):
                    if not oa and small_ok(segL, Lk, mk):
                        continue                              # the one-wavefront kernel refuses an unaligned o (no leaf)
                    fwd.add(route_fwd(segL, Lk, mk, oa))
                if mk != 2:
                    fwd.add(route_seg2(segL, Lk, mk))
            if Lk >= 1:
                fwd.add(route_grouped(segL, Lk))
                if Lk <= 32:
                    fwd.add(route_ends_fwd(segL, Lk))
                    bwd.add(route_ends_bwd(segL, Lk))
            for m4, al in ((True, True), (False, True), (True, False)):
                bwd.add(route_bwd(segL, Lk, m4, al))
    reasons = (None, "tensor-mask", "keys>32", "rows>32", "multiseg>16", "o-unaligned", "grad-stride", "grad-unaligned")
    out = {"fwd": {}, "bwd": {}}
    for f in itertools.product(("seg", "dual", "two", "grouped", "ends"), ("small", "qtile", "workgroup"), (1, 2),
                               ("self", "cross", "grouped"), ("none", "lds", "atomics"), range(1, 9), reasons):
        leaf = Leaf(*f)
        out["fwd"][leaf] = leaf in fwd
        out["bwd"][leaf] = leaf in bwd
    return out


# ------------------------------------------------------------------------------------------------ case table
def _F(entry, kernel, tiles, kv, why=None):
    return Leaf(entry, kernel, tiles, kv, "none", 4, why)


def _Bk(kernel, tiles, kv, red="none", waves=4, why=None, entry="seg"):
    return Leaf(entry, kernel, tiles, kv, red, waves, why)


def _c(name, entry, segL, Lk, mask, fwd, bwd, B=3, H=2, kvg=1, flags=()):
    return Case(name, entry, B, H, tuple(segL), Lk, mask, kvg, tuple(flags), fwd, bwd)


R1_8, R1_9, R1_16 = tuple(range(1, 9)), tuple(range(1, 10)), tuple(range(1, 17))
CASES = [
    # ---- one wavefront per problem.  Self-attention has Lk = L <= 16: one key tile; cross-attention to 17..32 keys: two.
    _c("small_self_causal", "seg", (5, 16, 1), 0, "causal", _F("seg", "small", 1, "self"), _Bk("small", 1, "self")),
    _c("small_self_plain", "seg", (1, 2), 0, None, _F("seg", "small", 1, "self"), _Bk("small", 1, "self")),
    _c("small_self_idle_waves", "seg", (7,), 0, "causal", _F("seg", "small", 1, "self"), _Bk("small", 1, "self"), B=1, H=1),
    _c("small_self_n16", "seg", R1_16, 0, "causal", _F("seg", "small", 1, "self"), _Bk("small", 1, "self")),
    _c("small_cross13", "seg", (4,), 13, None, _F("seg", "small", 1, "cross"), _Bk("small", 1, "cross")),
    _c("small_cross13_idle_waves", "seg", (16,), 13, None, _F("seg", "small", 1, "cross"), _Bk("small", 1, "cross"), B=1, H=1),
    _c("small_cross32_idle_waves", "seg", (16,), 32, None, _F("seg", "small", 2, "cross"), _Bk("small", 2, "cross"), B=1, H=1),
    _c("small_cross29_n5", "seg", (5, 16, 7, 1, 3), 29, None, _F("seg", "small", 2, "cross"), _Bk("small", 2, "cross", "lds", 5)),
    _c("small_cross29_n3", "seg", (5, 16, 7), 29, None, _F("seg", "small", 2, "cross"), _Bk("small", 2, "cross", "lds", 3)),
    _c("small_cross13_n2", "seg", (4, 2), 13, None, _F("seg", "small", 1, "cross"), _Bk("small", 1, "cross", "lds", 2)),
    _c("small_cross13_n5", "seg", (1, 16, 2, 3, 5), 13, None, _F("seg", "small", 1, "cross"), _Bk("small", 1, "cross", "lds", 5)),
    _c("small_cross13_n16", "seg", R1_16, 13, None, _F("seg", "small", 1, "cross"), _Bk("small", 1, "cross", "lds", 8)),
    _c("small_cross32_n2", "seg", (16, 3), 32, None, _F("seg", "small", 2, "cross"), _Bk("small", 2, "cross", "lds", 2)),
    _c("small_cross29_n8", "seg", R1_8, 29, None, _F("seg", "small", 2, "cross"), _Bk("small", 2, "cross", "lds", 8)),
    _c("small_cross32_n9", "seg", (16, 3, 1, 9, 2, 2, 7, 5, 11), 32, None, _F("seg", "small", 2, "cross"),
       _Bk("small", 2, "cross", "lds", 8)),
    _c("small_cross29_n16", "seg", R1_16, 29, None, _F("seg", "small", 2, "cross"), _Bk("small", 2, "cross", "lds", 8)),
    _c("small_cross13_n3", "seg", (2, 16, 5), 13, None, _F("seg", "small", 1, "cross"), _Bk("small", 1, "cross", "lds", 3)),
    _c("small_cross29_h8", "seg", (9, 4), 29, None, _F("seg", "small", 2, "cross"), _Bk("small", 2, "cross", "lds", 2), H=8),
    # ---- query tiles: one segment of 17..32 rows
    _c("qtile_self17_causal", "seg", (17,), 0, "causal", _F("seg", "qtile", 2, "self"), _Bk("qtile", 2, "self", "lds", 2)),
    _c("qtile_self29", "seg", (29,), 0, None, _F("seg", "qtile", 2, "self"), _Bk("qtile", 2, "self", "lds", 2)),
    _c("qtile_self32_causal", "seg", (32,), 0, "causal", _F("seg", "qtile", 2, "self"), _Bk("qtile", 2, "self", "lds", 2)),
    _c("qtile_cross20x32", "seg", (20,), 32, None, _F("seg", "qtile", 2, "cross"), _Bk("qtile", 2, "cross", "lds", 2)),
    _c("qtile_cross17x5", "seg", (17,), 5, None, _F("seg", "qtile", 1, "cross"), _Bk("qtile", 1, "cross", "lds", 2)),
    _c("qtile_self29_h8", "seg", (29,), 0, "causal", _F("seg", "qtile", 2, "self"), _Bk("qtile", 2, "self", "lds", 2), H=8),
    # ---- the workgroup kernel, one case per reason it is reached.  (Backward knows no mask: p is already zero there, so the
    # tensor-mask shapes go back to the kernels their sizes take.)
    _c("wg_mask7x11", "seg", (7,), 11, "tensor", _F("seg", "workgroup", 1, "cross", "tensor-mask"), _Bk("small", 1, "cross")),
    _c("wg_mask29x29", "seg", (29,), 29, "tensor", _F("seg", "workgroup", 1, "cross", "tensor-mask"),
       _Bk("qtile", 2, "cross", "lds", 2)),
    _c("wg_mask33x64", "seg", (33,), 64, "tensor", _F("seg", "workgroup", 2, "cross", "tensor-mask"),
       _Bk("workgroup", 2, "cross", why="keys>32")),
    _c("wg_keys33", "seg", (5,), 33, None, _F("seg", "workgroup", 2, "cross", "keys>32"), _Bk("workgroup", 2, "cross", why="keys>32")),
    _c("wg_keys64_n2", "seg", (16, 3), 64, None, _F("seg", "workgroup", 2, "cross", "keys>32"),
       _Bk("workgroup", 2, "cross", "atomics", why="keys>32")),
    _c("wg_rows33_self", "seg", (33,), 0, None, _F("seg", "workgroup", 2, "self", "rows>32"), _Bk("workgroup", 2, "self", why="rows>32")),
    _c("wg_rows64_self_causal", "seg", (64,), 0, "causal", _F("seg", "workgroup", 2, "self", "rows>32"),
       _Bk("workgroup", 2, "self", why="rows>32")),
    _c("wg_rows40x13", "seg", (40,), 13, None, _F("seg", "workgroup", 1, "cross", "rows>32"), _Bk("workgroup", 1, "cross", why="rows>32")),
    _c("wg_multiseg_self", "seg", (5, 20, 1), 0, "causal", _F("seg", "workgroup", 1, "self", "multiseg>16"),
       _Bk("workgroup", 1, "self", why="multiseg>16")),
    _c("wg_multiseg_self40", "seg", (3, 40), 0, None, _F("seg", "workgroup", 2, "self", "rows>32"),
       _Bk("workgroup", 2, "self", why="rows>32")),
    _c("wg_multiseg_cross29", "seg", (12, 20), 29, None, _F("seg", "workgroup", 1, "cross", "multiseg>16"),
       _Bk("workgroup", 1, "cross", "atomics", why="multiseg>16")),
    _c("wg_multiseg_cross29_rows40", "seg", (40, 2, 7), 29, None, _F("seg", "workgroup", 1, "cross", "rows>32"),
       _Bk("workgroup", 1, "cross", "atomics", why="rows>32")),
    _c("wg_o_offset_self29", "seg", (29,), 0, "causal", _F("seg", "workgroup", 1, "self", "o-unaligned"),
       _Bk("qtile", 2, "self", "lds", 2), flags=("o_off1",)),
    _c("wg_o_offset_cross20x32", "seg", (20,), 32, None, _F("seg", "workgroup", 1, "cross", "o-unaligned"),
       _Bk("qtile", 2, "cross", "lds", 2), flags=("o_off1",)),
    _c("wg_keys33_h8", "seg", (16,), 33, None, _F("seg", "workgroup", 2, "cross", "keys>32"), _Bk("workgroup", 2, "cross", why="keys>32"), H=8),
    # ---- backward fallbacks of shapes the one-wavefront kernels would take
    _c("bwd_gstride_cross29_n3", "seg", (5, 16, 7), 29, None, _F("seg", "small", 2, "cross"),
       _Bk("workgroup", 1, "cross", "atomics", why="grad-stride"), flags=("gstride2",)),
    _c("bwd_gstride_self29", "seg", (29,), 0, None, _F("seg", "qtile", 2, "self"), _Bk("workgroup", 1, "self", why="grad-stride"),
       flags=("gstride2",)),
    _c("bwd_dq_offset_self", "seg", (9, 4), 0, "causal", _F("seg", "small", 1, "self"), _Bk("workgroup", 1, "self", why="grad-unaligned"),
       flags=("dq_off1",)),
    _c("bwd_dq_offset_cross13", "seg", (4,), 13, None, _F("seg", "small", 1, "cross"), _Bk("workgroup", 1, "cross", why="grad-unaligned"),
       flags=("dq_off1",)),
    _c("bwd_gstride_cross13", "seg", (4,), 13, None, _F("seg", "small", 1, "cross"), _Bk("workgroup", 1, "cross", why="grad-stride"),
       flags=("gstride2",)),
    _c("bwd_dq_offset_cross29_n3", "seg", (5, 16, 7), 29, None, _F("seg", "small", 2, "cross"),
       _Bk("workgroup", 1, "cross", "atomics", why="grad-unaligned"), flags=("dq_off1",)),
    # ---- sbl_attention_seg2_fwd: the dual launch and the two-launch fallback
    _c("dual_self_causal", "seg2", (3, 16, 9), 0, "causal", _F("dual", "small", 1, "self"), None),
    _c("dual_cross29", "seg2", (5, 16, 7, 1), 29, None, _F("dual", "small", 2, "cross"), None),
    _c("dual_cross13", "seg2", (4, 2), 13, None, _F("dual", "small", 1, "cross"), None),
    _c("dual_self_idle_waves", "seg2", (7,), 0, "causal", _F("dual", "small", 1, "self"), None, B=1, H=1),
    _c("dual_cross29_idle_waves", "seg2", (16,), 29, None, _F("dual", "small", 2, "cross"), None, B=1, H=1),
    _c("dual_cross13_idle_waves", "seg2", (3,), 13, None, _F("dual", "small", 1, "cross"), None, B=1, H=1),
    _c("two_qtile_self29", "seg2", (29,), 0, "causal", _F("two", "qtile", 2, "self"), None),
    _c("two_qtile_cross20x32", "seg2", (20,), 32, None, _F("two", "qtile", 2, "cross"), None),
    _c("two_qtile_cross17x5", "seg2", (17,), 5, None, _F("two", "qtile", 1, "cross"), None),
    _c("two_wg_multiseg_cross29", "seg2", (12, 20), 29, None, _F("two", "workgroup", 1, "cross", "multiseg>16"), None),
    _c("two_wg_multiseg_self", "seg2", (5, 20, 1), 0, "causal", _F("two", "workgroup", 1, "self", "multiseg>16"), None),
    _c("two_wg_keys33", "seg2", (5, 2), 33, None, _F("two", "workgroup", 2, "cross", "keys>32"), None),
    _c("two_wg_rows33_self", "seg2", (33,), 0, "causal", _F("two", "workgroup", 2, "self", "rows>32"), None),
    _c("two_wg_rows40x13", "seg2", (40,), 13, None, _F("two", "workgroup", 1, "cross", "rows>32"), None),
    # ---- sbl_attention_seg_grouped_fwd: B sequences read the keys of entry b / kv_group
    _c("grouped_small29_g1", "grouped", (5, 16, 1), 29, None, _F("grouped", "small", 2, "grouped"), None, kvg=1),
    _c("grouped_small13_g3", "grouped", (4, 9), 13, None, _F("grouped", "small", 1, "grouped"), None, kvg=3),
    _c("grouped_small29_idle_waves", "grouped", (16,), 29, None, _F("grouped", "small", 2, "grouped"), None, B=1, H=1),
    _c("grouped_small13_idle_waves", "grouped", (5,), 13, None, _F("grouped", "small", 1, "grouped"), None, B=1, H=1),
    _c("grouped_qtile20x32_g3", "grouped", (20,), 32, None, _F("grouped", "qtile", 2, "grouped"), None, kvg=3),
    _c("grouped_qtile17x5_g1", "grouped", (17,), 5, None, _F("grouped", "qtile", 1, "grouped"), None, kvg=1),
    _c("grouped_wg_multiseg29_g3", "grouped", (12, 20), 29, None, _F("grouped", "workgroup", 1, "grouped", "multiseg>16"), None, kvg=3),
    _c("grouped_wg_keys64_g1", "grouped", (16,), 64, None, _F("grouped", "workgroup", 2, "grouped", "keys>32"), None, kvg=1),
    _c("grouped_wg_rows33x29_g3", "grouped", (33,), 29, None, _F("grouped", "workgroup", 1, "grouped", "rows>32"), None, kvg=3),
    # ---- the compact "ends" launches of the last decoder layer: seg_L are the FULL prefix lengths
    _c("ends_n1", "ends", (7,), 29, None, _F("ends", "small", 2, "cross"), _Bk("small", 2, "cross", entry="ends")),
    _c("ends_n1_row1_idle_waves", "ends", (1,), 32, None, _F("ends", "small", 2, "cross"), _Bk("small", 2, "cross", entry="ends"), B=1, H=1),
    _c("ends_n3", "ends", (1, 2, 9), 29, None, _F("ends", "small", 2, "cross"), _Bk("small", 2, "cross", "lds", 3, entry="ends")),
    _c("ends_n3_keys13", "ends", (40, 1, 2), 13, None, _F("ends", "small", 1, "cross"), _Bk("small", 1, "cross", "lds", 3, entry="ends")),
    _c("ends_n1_keys13_idle_waves", "ends", (2,), 13, None, _F("ends", "small", 1, "cross"), _Bk("small", 1, "cross", entry="ends"), B=1, H=1),
    _c("ends_n9", "ends", R1_9, 32, None, _F("ends", "small", 2, "cross"), _Bk("small", 2, "cross", "lds", 8, entry="ends")),
    _c("ends_n16", "ends", R1_16, 29, None, _F("ends", "small", 2, "cross"), _Bk("small", 2, "cross", "lds", 8, entry="ends")),
    _c("ends_n2", "ends", (1, 7), 29, None, _F("ends", "small", 2, "cross"), _Bk("small", 2, "cross", "lds", 2, entry="ends")),
    _c("ends_n5", "ends", (16, 1, 2, 9, 3), 32, None, _F("ends", "small", 2, "cross"), _Bk("small", 2, "cross", "lds", 5, entry="ends")),
    _c("ends_n2_keys13", "ends", (2, 5), 13, None, _F("ends", "small", 1, "cross"), _Bk("small", 1, "cross", "lds", 2, entry="ends")),
    _c("ends_n5_keys13", "ends", (1, 2, 3, 4, 5), 13, None, _F("ends", "small", 1, "cross"), _Bk("small", 1, "cross", "lds", 5, entry="ends")),
    _c("ends_n9_keys13", "ends", R1_9, 13, None, _F("ends", "small", 1, "cross"), _Bk("small", 1, "cross", "lds", 8, entry="ends")),
    _c("ends_n8", "ends", R1_8, 32, None, _F("ends", "small", 2, "cross"), _Bk("small", 2, "cross", "lds", 8, entry="ends")),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)
FAMILIES = ("flat", "peaked")
# `planted` runs once per forward kernel body (and once under a tensor mask and in the ends form)
PLANTED = ("small_self_causal", "small_cross29_n5", "qtile_self32_causal", "wg_rows64_self_causal", "wg_mask29x29", "ends_n3")


# ------------------------------------------------------------------------------------------------ dropout hash
M64 = (1 << 64) - 1


def rand_u32(seed, offset, idx):
    """sbl_common.h sbl_rand_u32: one 32-bit draw per (seed, stream offset, element index), uint64 arithmetic mod 2^64"""
    idx = np.asarray(idx, dtype=np.uint64)
    base = np.uint64((int(seed) + 0x9E3779B97F4A7C15 * (int(offset) + 1)) & M64)
    with np.errstate(over="ignore"):
        z = base + idx * np.uint64(0xD1B54A32D192ED03)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint32)


def drop_thresh(p):
    """sbl_common.h sbl_drop_thresh: (uint32_t)((double)(float)p * 2^32), clamped"""
    t = float(np.float32(p)) * 4294967296.0
    return int(min(max(t, 0.0), 4294967295.0))


def keep_mask(seed, offset, idx, p):
    """sbl_keep: draw >= threshold"""
    return rand_u32(seed, offset, idx) >= np.uint32(drop_thresh(p))


def keep_scale(p):
    """the launchers' `1.f / (1.f - drop_p)` in float32"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def p_offsets(segL, B, H, Lk_fixed):
    """start (floats) of every segment's (H*B, L, Lk) probability block, and the total"""
    off, tot = [], 0
    for L in segL:
        off.append(tot)
        tot += H * B * L * (Lk_fixed or L)
    return off, tot


def mask_index_full(segL, B, H, Lk_fixed, s, h, b, i, j):
    """full layout: the element's place in the probability buffer - block s, then (h*B + b, i, j) of (H*B, L, Lk)"""
    L = segL[s]
    Lk = Lk_fixed or L
    return p_offsets(segL, B, H, Lk_fixed)[0][s] + ((h * B + b) * L + i) * Lk + j


def mask_index_qtile(L, Lk, B, H, h, b, tile, r, j):
    """query tiles: row r of tile `tile` is row 16*tile + r of the one (H*B, L, Lk) block the call documents"""
    return ((h * B + b) * L + 16 * tile + r) * Lk + j


def mask_index_ends(segL, B, H, Lk_fixed, s, h, b, kk, j):
    """ends: compact row kk (0 or 1) of sequence (s, b) stands for position kk*(L-1) of the full layout"""
    return mask_index_full(segL, B, H, Lk_fixed, s, h, b, kk * (segL[s] - 1), j)


# ------------------------------------------------------------------------------------------------ problems of a case
def q_lengths(c):
    """lengths of the query segments as the buffers hold them (the ends form holds min(2, L) rows per sequence)"""
    return tuple(min(2, L) for L in c.segL) if c.entry == "ends" else c.segL


def rows_q(c):
    return c.B * sum(q_lengths(c))


def rows_k(c):
    return (c.B // c.kvg) * c.Lk if c.Lk else rows_q(c)


def problems(c, mutant=None):
    """One dict per (segment, head, batch entry): the rows of q / k it reads, where its probabilities sit in the flat buffer
    (pidx, (Lq, Lk) int64) and the dropout index of each (midx).  `mutant` plants the index bugs of the emulation."""
    Lq_list = q_lengths(c)
    poff, _ = p_offsets(Lq_list, c.B, c.H, c.Lk)
    poff_full, _ = p_offsets(c.segL, c.B, c.H, c.Lk)
    out, row = [], 0
    for s, Lq in enumerate(Lq_list):
        Lk = c.Lk or Lq
        ii, jj = np.meshgrid(np.arange(Lq), np.arange(Lk), indexing="ij")
        for h in range(c.H):
            for b in range(c.B):
                qrows = row + b * Lq + np.arange(Lq)
                krows = (b // c.kvg) * Lk + np.arange(Lk) if c.Lk else qrows
                blk = (b * c.H + h) if mutant == "p_bh" else (h * c.B + b)
                pidx = poff[s] + (blk * Lq + ii) * Lk + jj
                if c.entry == "ends":
                    step = c.segL[s] if mutant == "ends_step" else c.segL[s] - 1
                    midx = poff_full[s] + ((h * c.B + b) * c.segL[s] + ii * step) * Lk + jj
                else:
                    midx = poff[s] + ((h * c.B + b) * Lq + ii) * Lk + jj
                if mutant == "no_poff":
                    midx = midx - (poff_full[s] if c.entry == "ends" else poff[s])
                out.append(dict(s=s, h=h, b=b, Lq=Lq, Lk=Lk, qrows=qrows, krows=krows, pidx=pidx, midx=midx))
        row += c.B * Lq
    return out


def documented_mask_index(c, pr):
    """The (Lq, Lk) dropout indices of problem `pr` from the layout functions above, element by element (the test of the
    table checks problems() against this; it is what the float64 reference uses)."""
    out = np.empty((pr["Lq"], pr["Lk"]), dtype=np.int64)
    for i in range(pr["Lq"]):
        for j in range(pr["Lk"]):
            if c.entry == "ends":
                out[i, j] = mask_index_ends(c.segL, c.B, c.H, c.Lk, pr["s"], pr["h"], pr["b"], i, j)
            elif len(c.segL) == 1 and 16 < c.segL[0] <= 32 and c.mask != "tensor":
                out[i, j] = mask_index_qtile(c.segL[0], pr["Lk"], c.B, c.H, pr["h"], pr["b"], i // 16, i % 16, j)
            else:
                out[i, j] = mask_index_full(c.segL, c.B, c.H, c.Lk, pr["s"], pr["h"], pr["b"], i, j)
    return out


def visible(c, pr, mask, mutant=None):
    """(Lq, Lk) bool: key j is visible to query i"""
    Lq, Lk = pr["Lq"], pr["Lk"]
    ii, jj = np.meshgrid(np.arange(Lq), np.arange(Lk), indexing="ij")
    if c.mask == "causal":
        if mutant == "causal_off1":
            return jj <= ii + 1
        if mutant == "causal_qtile" and c.fwd.kernel == "qtile":
            return jj <= ii % 16
        return jj <= ii
    if c.mask == "tensor":
        m = mask[pr["b"]]
        if mutant == "mask_bji":
            m = mask.reshape(c.B, Lk, Lq)[pr["b"]].T
        return m == 0
    return np.ones((Lq, Lk), dtype=bool)


# ------------------------------------------------------------------------------------------------ inputs
def _u(c, what, shape, direction):
    return detfill.uniform("ar.%s.%s%s" % (c.name, what, "#1" if direction else ""), shape)


def make_inputs(c, family, direction=0, full_row=False):
    """float32 q (rows_q, H*64), k, v (rows_k, H*64), dout like q, and the uint8 tensor mask (B, Lq, Lk) or None.
    flat: detfill.uniform in [-1, 1).  peaked: every (row, head) slice of q scaled so that, among its visible keys, the score
    spread exceeds 110 and the top score leads by at least 6.  planted: q = 8 * (one visible key), keys 0 and 1 exact copies,
    q = 0 for the last batch entry.  full_row: the tensor mask hides every key of row 2 of batch entry B-1."""
    HD = c.H * 64
    Rq, Rk = rows_q(c), rows_k(c)
    inp = dict(q=_u(c, "q", (Rq, HD), direction), k=_u(c, "k", (Rk, HD), direction), v=_u(c, "v", (Rk, HD), direction),
               do=_u(c, "do", (Rq, HD), direction), mask=None)
    if c.mask == "tensor":
        m = (_u(c, "m", (c.B, c.segL[0], c.Lk), 0) > 0.3).astype(np.uint8)
        m[:, :, 0] = 0
        if full_row:
            m[c.B - 1, 2, :] = 1
        inp["mask"] = m
    if family == "flat":
        return inp
    q, k = inp["q"].copy(), inp["k"].copy()
    prs = problems(c)
    if family == "planted":
        for pr in prs:                                   # keys first: every problem that shares them sees the same copy
            cols = slice(pr["h"] * 64, pr["h"] * 64 + 64)
            if pr["Lk"] >= 2:
                k[pr["krows"][1], cols] = k[pr["krows"][0], cols]
        for pr in prs:
            cols = slice(pr["h"] * 64, pr["h"] * 64 + 64)
            vis = visible(c, pr, inp["mask"])
            for i in range(pr["Lq"]):
                js = np.flatnonzero(vis[i])
                if c.B > 1 and pr["b"] == c.B - 1 or not len(js):
                    q[pr["qrows"][i], cols] = 0.0
                else:
                    q[pr["qrows"][i], cols] = np.float32(8.0) * k[pr["krows"][js[(3 * i + 1) % len(js)]], cols]
        inp["q"], inp["k"] = q, k
        return inp
    assert family == "peaked", family
    for pr in prs:
        cols = slice(pr["h"] * 64, pr["h"] * 64 + 64)
        vis = visible(c, pr, inp["mask"])
        s = (q[pr["qrows"], cols].astype(np.float64) @ k[pr["krows"], cols].astype(np.float64).T) * SCALE
        for i in range(pr["Lq"]):
            sv = np.sort(s[i][vis[i]])
            if len(sv) < 2:
                continue                                  # a single visible key: p = 1 whatever the scale
            assert sv[-1] > sv[-2], "tie at the top of a flat row"
            f = max(110.0 / (sv[-1] - sv[0]), 6.0 / (sv[-1] - sv[-2]))
            q[pr["qrows"][i], cols] = (q[pr["qrows"][i], cols].astype(np.float64) * f).astype(np.float32)
    inp["q"] = q
    return inp


# ------------------------------------------------------------------------------------------------ float64 reference + bounds
def expf_rel(ax):
    """allowed relative error of __expf at |x| = ax: EXPF_C * (|x| + 2) * U (module docstring)"""
    return EXPF_C * (ax + 2.0) * U


def _pad32(n):
    return (n + 31) // 32 * 32


def forward_problem(qq, kk, vv, vis, keep, ks):
    """One (Lq, 64) x (Lk, 64) problem in float64: p, its bound Ep, the positions that must be exactly 1, pd = dropped p and
    its bound, o and its bound (first order, before SLACK; the derivations are in reference()'s docstring)."""
    Lk32 = _pad32(kk.shape[0])
    s = (qq @ kk.T) * SCALE
    Es = C_DOT64 * U * SCALE * (np.abs(qq) @ np.abs(kk).T)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.where(vis, s, -np.inf).max(1, keepdims=True)
        x = np.where(vis, s - m, -np.inf)
        e = np.where(vis, np.exp(x), 0.0)
    tot = e.sum(1, keepdims=True)
    p = np.divide(e, tot, out=np.zeros_like(e), where=tot > 0)      # a row without a visible key: p = 0 (sbl_hip.h)
    ax = np.where(vis, np.abs(np.where(vis, x, 0.0)), 0.0)
    r = np.where(vis, Es + U * ax + expf_rel(ax), 0.0)
    Ep = np.where(vis, p * (r + (p * r).sum(1, keepdims=True) + C_SUM * U) + TINY, 0.0)
    one = vis & (vis.sum(1, keepdims=True) == 1)
    Ep[one] = 0.0                                                    # exp(0) / exp(0): exactly 1
    pd = np.where(keep, p * ks, 0.0)
    Epd = np.where(keep & vis, ks * (Ep + 3 * U * p) + TINY, 0.0)
    o = pd @ vv
    Eo = Epd @ np.abs(vv) + (Lk32 + 2) * U * (pd @ np.abs(vv))
    return p, Ep, one, pd, Epd, o, Eo


def step_reference(q, K, V):
    """One query per (slot, head) against its own keys (the decode-step kernels): q (S, H*64), K / V (S, n, H*64) float32 ->
    (o, bound) in float64 with the bounds of reference(); lane-wise 64-term dot products, a 64-lane softmax, n serial adds."""
    S, n, HD = K.shape
    o, Eo = np.zeros((S, HD)), np.zeros((S, HD))
    vis = np.ones((1, n), dtype=bool)
    for b in range(S):
        for h in range(HD // 64):
            cols = slice(h * 64, h * 64 + 64)
            r = forward_problem(q[b:b + 1, cols].astype(np.float64), K[b][:, cols].astype(np.float64), V[b][:, cols].astype(np.float64),
                                vis, vis, 1.0)
            o[b, cols], Eo[b, cols] = r[5][0], SLACK * (r[6][0] + TINY)
    return o, Eo


def peak_rows(q, K):
    """The `peaked` scaling for step_reference's shapes: every (slot, head) slice of q scaled as in make_inputs."""
    q = q.copy()
    for b in range(K.shape[0]):
        for h in range(K.shape[2] // 64):
            cols = slice(h * 64, h * 64 + 64)
            sv = np.sort(K[b][:, cols].astype(np.float64) @ q[b, cols].astype(np.float64) * SCALE)
            if len(sv) >= 2:
                q[b, cols] = (q[b, cols].astype(np.float64) * max(110.0 / (sv[-1] - sv[0]), 6.0 / (sv[-1] - sv[-2]))).astype(np.float32)
    return q


def reference(c, inp, drop_p=0.0, seed=0, offset=0):
    """float64 forward and backward of a case from its float32 inputs, with the keep mask rand_u32 gives at the documented
    indices.  Returns {name: (value, bound)} for p (flat, as the buffer holds it), o, dq, dk, dv, and `single`: the flat
    positions whose probability must be exactly 1 (the only visible key of their row).
    Bounds (U = 2^-24, first order, then * SLACK):
      s    = scale * sum_d q k        |ds| <= C_DOT64 U scale sum|q k|                                   =: Es
      p_j  = e_j / sum e, e_j = exp(s_j - m).  The shift m cancels exactly, whichever key the computed maximum sits at, so
             rel(e_j) <= r_j = Es_j + U |x_j| (the subtraction) + expf_rel(|x_j|), and
             rel(p_j) <= r_j + sum_l p_l r_l + C_SUM U;  |dp_j| <= p_j * that + TINY                     =: Ep
      pd   = keep ? p * keep_scale : 0 (keep_scale itself rounded: 2 U, the product 1 U)                 Epd = ks (Ep + 3 U p) + TINY
      o    = sum_j pd v               |do| <= sum_j Epd |v| + (Lk32 + 2) U sum_j pd |v|,  Lk32 = keys padded to 32 (MFMA steps)
      dv   = sum_i pd dO              likewise over the queries (Lq32 + 2), summed over the segments that share keys, plus
             nseg U sum|contributions| for that sum (LDS or atomics, any order)
      dpd  = sum_d dO v               C_DOT64 U sum|dO v|;   dp = keep ? dpd * ks : 0:  Edp = ks (Edpd + 3 U |dpd|)
      dot  = sum_j p dp               Edot = sum_j (Ep |dp| + p Edp) + C_SUM U sum_j p |dp|
      ds   = p (dp - dot) scale       Eds = scale (Ep |dp - dot| + p (Edp + Edot) + 4 U p |dp - dot|) + TINY
      dq   = sum_j ds k               sum_j Eds |k| + (Lk32 + 2) U sum_j |ds k|;   dk = sum_i ds q likewise over queries/segments.
    The backward runs from the kernel's own float32 p, whose error Ep is part of every line above."""
    HD = c.H * 64
    q, k, v, do = (inp[n].astype(np.float64) for n in ("q", "k", "v", "do"))
    ks = float(keep_scale(drop_p)) if drop_p else 1.0
    _, ptot = p_offsets(q_lengths(c), c.B, c.H, c.Lk)
    P, EP = np.zeros(ptot), np.zeros(ptot)
    single = np.zeros(ptot, dtype=bool)
    O, EO = np.zeros((rows_q(c), HD)), np.zeros((rows_q(c), HD))
    DQ, EDQ = np.zeros_like(O), np.zeros_like(O)
    DK, EDK, ADK = (np.zeros((rows_k(c), HD)) for _ in range(3))
    DV, EDV, ADV = (np.zeros((rows_k(c), HD)) for _ in range(3))
    nshare = len(c.segL) if c.Lk else 1
    for pr in problems(c):
        cols = slice(pr["h"] * 64, pr["h"] * 64 + 64)
        qq, kk, vv, gg = q[pr["qrows"], cols], k[pr["krows"], cols], v[pr["krows"], cols], do[pr["qrows"], cols]
        vis = visible(c, pr, inp["mask"])
        keep = np.ones_like(vis)
        if drop_p:
            keep = keep_mask(seed, offset, documented_mask_index(c, pr), drop_p)
        Lk32, Lq32 = _pad32(pr["Lk"]), _pad32(pr["Lq"])
        p, Ep, one, pd, Epd, o1, Eo1 = forward_problem(qq, kk, vv, vis, keep, ks)
        P[pr["pidx"]], EP[pr["pidx"]], single[pr["pidx"]] = p, Ep, one
        O[pr["qrows"], cols], EO[pr["qrows"], cols] = o1, Eo1
        # backward
        dpd = gg @ vv.T
        Edpd = C_DOT64 * U * (np.abs(gg) @ np.abs(vv).T)
        dp = np.where(keep, dpd * ks, 0.0)
        Edp = np.where(keep, ks * (Edpd + 3 * U * np.abs(dpd)), 0.0)
        dot = (p * dp).sum(1, keepdims=True)
        Edot = (Ep * np.abs(dp) + p * Edp).sum(1, keepdims=True) + C_SUM * U * (p * np.abs(dp)).sum(1, keepdims=True)
        g = dp - dot
        ds = p * g * SCALE
        Eds = np.where(vis, SCALE * (Ep * np.abs(g) + p * (Edp + Edot) + 4 * U * p * np.abs(g)) + TINY, 0.0)
        DQ[pr["qrows"], cols] = ds @ kk
        EDQ[pr["qrows"], cols] = Eds @ np.abs(kk) + (Lk32 + 2) * U * (np.abs(ds) @ np.abs(kk))
        dk1, dv1 = ds.T @ qq, pd.T @ gg
        DK[pr["krows"], cols] += dk1
        DV[pr["krows"], cols] += dv1
        ADK[pr["krows"], cols] += np.abs(dk1)
        ADV[pr["krows"], cols] += np.abs(dv1)
        EDK[pr["krows"], cols] += Eds.T @ np.abs(qq) + (Lq32 + 2) * U * (np.abs(ds).T @ np.abs(qq))
        EDV[pr["krows"], cols] += Epd.T @ np.abs(gg) + (Lq32 + 2) * U * (pd.T @ np.abs(gg))
    EDK += nshare * U * ADK
    EDV += nshare * U * ADV
    for E in (EO, EDQ, EDK, EDV):
        E += TINY                                                        # the float32 result itself, flushed below 2^-126
    ref = dict(p=(P, SLACK * EP), o=(O, SLACK * EO), dq=(DQ, SLACK * EDQ), dk=(DK, SLACK * EDK), dv=(DV, SLACK * EDV))
    ref["single"] = single
    return ref


def compare(ref, out, names=("p", "o", "dq", "dk", "dv")):
    """{name: largest |out - ref| / bound}; where the bound is 0 the value must be exact, else the ratio is inf.  NaN -> inf."""
    ratios = {}
    for n in names:
        if out.get(n) is None:
            continue
        val, bound = ref[n]
        got = np.asarray(out[n], dtype=np.float64).reshape(val.shape)
        err = np.abs(got - val)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
        ratio = np.where(np.isfinite(got), ratio, np.inf)
        ratios[n] = float(ratio.max()) if ratio.size else 0.0
    return ratios


def exact_failures(c, inp, ref, out, family):
    """The assertions that hold bit for bit, as a list of messages (empty: all hold):
    a row with a single visible key (row 0 under the causal mask) has p exactly 1; masked positions are exactly 0 (that one is
    already part of compare(): their bound is 0); planted: the two copied keys get bit-identical probabilities."""
    bad = []
    if out.get("p") is None:
        return bad
    p = np.asarray(out["p"], dtype=np.float32)
    if not np.all(p[ref["single"]] == np.float32(1.0)):
        bad.append("a row with one visible key does not have p == 1")
    if family == "planted":
        for pr in problems(c):
            if pr["Lk"] < 2:
                continue
            vis = visible(c, pr, inp["mask"])
            both = vis[:, 0] & vis[:, 1]
            blk = p[pr["pidx"]]
            if not np.array_equal(blk[both, 0].view(np.uint32), blk[both, 1].view(np.uint32)):
                bad.append("duplicate keys 0 and 1 differ in problem (s=%d, h=%d, b=%d)" % (pr["s"], pr["h"], pr["b"]))
                break
    return bad


# ------------------------------------------------------------------------------------------------ float32 emulation
MUTANTS = ("no_max", "max16", "causal_off1", "causal_qtile", "mask_bji", "ends_step", "no_poff", "ks_fwd_only", "scale2_dq",
           "dkv_last", "p_bh")


def emulate_f32(c, inp, drop_p=0.0, seed=0, offset=0, mutant=None):
    """numpy float32 emulation of the kernels' order of operations - score, max, exp, sum, divide, dropout, PV, and the
    backward chain from its own float32 p - with the buffer layouts and dropout indices of the kernels.  `mutant` plants one
    of MUTANTS.  Only for checking the bounds and the case table on the CPU."""
    f32 = np.float32
    HD = c.H * 64
    q, k, v, do = (inp[n] for n in ("q", "k", "v", "do"))
    ks = keep_scale(drop_p) if drop_p else f32(1.0)
    _, ptot = p_offsets(q_lengths(c), c.B, c.H, c.Lk)
    P = np.zeros(ptot, dtype=f32)
    O, DQ = np.zeros((rows_q(c), HD), dtype=f32), np.zeros((rows_q(c), HD), dtype=f32)
    DK, DV = np.zeros((rows_k(c), HD), dtype=f32), np.zeros((rows_k(c), HD), dtype=f32)
    nseg = len(c.segL)
    with np.errstate(all="ignore"):
        for pr in problems(c, mutant):
            cols = slice(pr["h"] * 64, pr["h"] * 64 + 64)
            qq, kk, vv, gg = q[pr["qrows"], cols], k[pr["krows"], cols], v[pr["krows"], cols], do[pr["qrows"], cols]
            vis = visible(c, pr, inp["mask"], mutant)
            keep = np.ones_like(vis)
            if drop_p:
                keep = keep_mask(seed, offset, pr["midx"], drop_p)
            s = (qq @ kk.T) * f32(SCALE)
            sm = np.where(vis, s, f32(-np.inf))
            if mutant == "no_max":
                m = np.zeros((pr["Lq"], 1), dtype=f32)
            elif mutant == "max16":
                m = sm[:, :16].max(1, keepdims=True)
                m = np.where(np.isfinite(m), m, f32(0.0))
            else:
                m = sm.max(1, keepdims=True)
            e = np.where(vis, np.exp((s - m).astype(f32)), f32(0.0)).astype(f32)
            tot = e.sum(1, keepdims=True, dtype=f32)
            p = np.where(tot > 0, e / tot, f32(0.0)).astype(f32)
            P[pr["pidx"]] = p
            pd = np.where(keep, p * ks, f32(0.0)).astype(f32)
            O[pr["qrows"], cols] = pd @ vv
            ksb = f32(1.0) if mutant == "ks_fwd_only" else ks
            pdb = np.where(keep, p * ksb, f32(0.0)).astype(f32)
            dp = np.where(keep, (gg @ vv.T) * ksb, f32(0.0)).astype(f32)
            dot = (p * dp).sum(1, keepdims=True, dtype=f32)
            ds = (p * (dp - dot) * f32(SCALE)).astype(f32)
            DQ[pr["qrows"], cols] = (ds @ kk) * (f32(SCALE) if mutant == "scale2_dq" else f32(1.0))
            if mutant == "dkv_last" and c.Lk and pr["s"] != nseg - 1:
                continue
            DK[pr["krows"], cols] += ds.T @ qq
            DV[pr["krows"], cols] += pdb.T @ gg
    out = dict(p=P, o=O, dq=DQ, dk=DK, dv=DV)
    if c.entry == "grouped":
        out["p"] = None
    return out
