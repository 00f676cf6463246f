"""The host dispatch of sbl_gemm_f32 / sbl_gemm2_f32 restated in Python, and the case table of the route-aware GEMM tests.

route() / route_gemm2() follow csrc/gemm.hip line by line (pure integer arithmetic, no torch, no GPU) and return the
leaf of the dispatch tree a call lands on:

    Leaf(family, layout, vec, ku, splits, reduction)
      family     "skinny" | "tiled64" | "tiled128"             (sbl_profile_last_kernel() 1 | 2 | 3)
      layout     "nt" (ta, tb) = (0, 1) | "nn" (0, 0) | "tn" (1, 0) | "tt" (1, 1) | "dual" (sbl_gemm2_f32's own launch)
      vec        float4 loaders (True) or scalar ones (False); None for the skinny kernel
      ku         KU of the tile engine (4 | 2 | 1), or (NW, U) of the skinny kernel
      splits     gridDim.z of the launch: the K slices that really run (the host's `splits` after sbl_launch_gemm rounds
                 the chunk up to whole macro steps, e.g. K = 196 asks for 3 and runs 2 at KU = 4)
      reduction  "none" | "slabs" (in-launch slab sum) | "atomics" (float atomics on C) | "forced1" (split-K wanted, no
                 usable workspace and a non-plain epilogue: splits set back to 1)

Every threshold below is a copy; the comment next to it names the line it mirrors.  A change to one of those lines must
be made here too - tests/test_gemm_routes_gpu.py asserts the kernel family of every launch against route(), so a
threshold that moved without this file fails there.

CASES / GEMM2_CASES carry, next to each shape, the leaf it is meant to hit, written by hand (never computed by route());
tests/test_gemm_routes_cpu.py checks route(case) == case.leaf and that the table reaches every leaf of LEAVES.
"""
import collections

Leaf = collections.namedtuple("Leaf", "family layout vec ku splits reduction")
KERNEL_ID = {"skinny": 1, "tiled64": 2, "tiled128": 3}      # csrc/sbl_common.h: SBL_KID_SKINNY / TILED64 / TILED128
KID_SEG_WGRAD = 7                                            # SBL_KID_SEG_WGRAD (both merged weight-gradient entry points)

WS_COUNTERS = 4096                  # gemm.hip: SBL_WS_COUNTERS
WS_FULL = 16 << 20                  # ops.py: WS_BYTES
WS_SHORT = 4 * WS_COUNTERS          # the smallest workspace the ABI accepts: counters only, no slab
BIG_MIN_TILES = 4096                # tuning.h: sbl_big_min_tiles
SPLIT_TILES, SPLIT_TARGET, SPLIT_MAX = 192, 256, 8        # gemm.hip sbl_gemm_f32: split_tiles, split_target, "splits > 8"
SK_MAX_M, SK_MAX_T, SK_SQ_ROWS = 512, 2048, 1536          # gemm.hip sbl_gemm_f32: max_m, max_t, sq_rows
SK_SQ_AREA = 512 * 512                                    # ... and the 512L * 512 of shape_ok
KU2_TILES = 512                                           # gemm.hip: "tiles64 * splits > 512" (both entry points)
G2_MAX_M, G2_MAX_T, G2_SQ_ROWS = 128, 2048, 768           # gemm.hip sbl_gemm2_f32: max_m, max_t, sq_rows
G2_SPLIT_TILES, G2_SPLIT_TARGET, G2_SPLIT_MAX = 192, 256, 8      # tuning.h: sbl_gemm2_split_tiles / _target / _max
BK = 16                             # tile_loaders.h: SBL_BK

LAYOUT = {(0, 1): "nt", (0, 0): "nn", (1, 0): "tn", (1, 1): "tt"}


def cdiv(a, b):
    return (a + b - 1) // b


def skinny_nwu(K):
    """skinny_gemm.h sbl_launch_skinny: (NW, U) by K."""
    return (8, 8) if K >= 1024 else (8, 4) if K >= 512 else (4, 4)


def grid_z(K, splits, ku):
    """mfma_gemm.h sbl_launch_gemm / sbl_launch_gemm2: kchunk rounded up to whole macro steps, nz = cdiv(K, kchunk)."""
    mk = ku * BK
    return cdiv(K, cdiv(cdiv(K, splits), mk) * mk)


def route(ta, tb, M, N, K, lda, ldb, aligned, bias=False, relu=False, mask=False, accumulate=False, ws_bytes=WS_FULL):
    """Leaf of sbl_gemm_f32.  aligned: both operand pointers are 16-byte aligned; ws_bytes None: ws == NULL.
    (accumulate chooses the store mode and the memset of the atomics path, never the route.)"""
    layout = LAYOUT[(ta, tb)]
    vec = aligned and lda % 4 == 0 and ldb % 4 == 0
    if not ta or tb:
        vec = vec and K % 4 == 0
    if ta:
        vec = vec and M % 4 == 0
    if not tb:
        vec = vec and N % 4 == 0
    plain = not (bias or relu or mask)
    tiles64 = cdiv(M, 64) * cdiv(N, 64)
    big = M >= 1024 and N >= 256 and tiles64 >= BIG_MIN_TILES
    splits, reduction = 1, "none"
    if not big and tiles64 < SPLIT_TILES and K >= 128:
        splits = max(1, min(cdiv(SPLIT_TARGET, tiles64), K // 64, SPLIT_MAX))
    if splits > 1:
        need = 4 * WS_COUNTERS + tiles64 * splits * 64 * 64 * 4
        if ws_bytes is not None and tiles64 < WS_COUNTERS and need <= ws_bytes:
            reduction = "slabs"
        elif plain:
            reduction = "atomics"
        else:
            splits, reduction = 1, "forced1"
    # the skinny kernel takes its shapes whatever the split logic above decided
    a_kc, b_kc = not ta, bool(tb)
    al_ok = (not a_kc or (aligned and lda % 4 == 0)) and (not b_kc or (aligned and ldb % 4 == 0))
    k_ok = (not a_kc and not b_kc) or K % 8 == 0
    tiles32 = cdiv(M, 32) * cdiv(N, 32)
    if ta:
        shape_ok = (K <= SK_MAX_M and tiles32 <= SK_MAX_T) or (M * N <= SK_SQ_AREA and K <= SK_SQ_ROWS)
    else:
        shape_ok = (M <= SK_MAX_M and tiles32 <= SK_MAX_T) or (N * K <= SK_SQ_AREA and M <= SK_SQ_ROWS)
    if shape_ok and al_ok and k_ok and not (ta and tb):
        return Leaf("skinny", layout, None, skinny_nwu(K), 1, "none")
    if big:
        return Leaf("tiled128", layout, vec, 1, 1, "none")
    ku = 1 if not vec else 2 if tiles64 * splits > KU2_TILES else 4
    return Leaf("tiled64", layout, vec, ku, grid_z(K, splits, ku), reduction)


def route_gemm2(M, N, K, lda, ldb, aligned, bias=False, relu=False, ws_bytes=WS_FULL):
    """Leaves of sbl_gemm2_f32: one Leaf with layout "dual" for its own launch, or - the two-launch fallback - the leaf
    of the sbl_gemm_f32(0, 1, ...) call it makes twice."""
    vec = aligned and lda % 4 == 0 and ldb % 4 == 0 and K % 8 == 0
    tiles64 = cdiv(M, 64) * cdiv(N, 64)
    big = M >= 1024 and N >= 256 and 2 * tiles64 >= BIG_MIN_TILES
    if not vec or big:
        return route(0, 1, M, N, K, lda, ldb, aligned, bias, relu, False, False, ws_bytes)
    tiles32 = cdiv(M, 32) * cdiv(N, 32)
    if (M <= G2_MAX_M and tiles32 <= G2_MAX_T) or (N * K <= SK_SQ_AREA and M <= G2_SQ_ROWS):
        return Leaf("skinny", "dual", None, skinny_nwu(K), 1, "none")
    splits, reduction = 1, "none"
    if 2 * tiles64 < G2_SPLIT_TILES and K >= 128:
        splits = max(1, min(cdiv(G2_SPLIT_TARGET, 2 * tiles64), K // 64, G2_SPLIT_MAX))
    if splits > 1:
        need = 4 * WS_COUNTERS + 2 * tiles64 * splits * 64 * 64 * 4
        if ws_bytes is not None and 2 * tiles64 < WS_COUNTERS and need <= ws_bytes:
            reduction = "slabs"
        else:
            splits, reduction = 1, "forced1"
    ku = 2 if 2 * tiles64 * splits > KU2_TILES else 4
    return Leaf("tiled64", "dual", True, ku, grid_z(K, splits, ku), reduction)


# --------------------------------------------------------------------------- every reachable leaf
def leaf_key(leaf):
    """Identity of a leaf for the coverage check (the slice count is a property of the case, not of the branch)."""
    return (leaf.family, leaf.layout, leaf.vec, leaf.ku, leaf.reduction)


def all_leaves():
    """Every reachable leaf key of the two dispatch trees.
    Not reachable, and therefore not listed: KU = 2 together with a split (a split needs tiles < 192 and then
    tiles * splits < 256 + 192 <= 512); 128x128 tiles with a split (`!big` guards the split); a dual launch with scalar
    loaders or atomics (sbl_gemm2_f32 falls back to two launches / to splits = 1 instead)."""
    out = set()
    for lay in ("nt", "nn", "tn"):
        for nwu in ((4, 4), (8, 4), (8, 8)):
            out.add(("skinny", lay, None, nwu, "none"))
    for lay in ("nt", "nn", "tn", "tt"):
        for vec, ku in ((True, 4), (False, 1)):
            for red in ("none", "slabs", "atomics", "forced1"):
                out.add(("tiled64", lay, vec, ku, red))
        out.add(("tiled64", lay, True, 2, "none"))
        for vec in (True, False):
            out.add(("tiled128", lay, vec, 1, "none"))
    for nwu in ((4, 4), (8, 4), (8, 8)):
        out.add(("skinny", "dual", None, nwu, "none"))
    for red in ("none", "slabs", "forced1"):
        out.add(("tiled64", "dual", True, 4, red))
    out.add(("tiled64", "dual", True, 2, "none"))
    return out


# --------------------------------------------------------------------------- case table
# pa / pb: floats added to the smallest legal lda / ldb;  off: the operand pointers are offset by this many floats from a
# 16-byte boundary (0 or 1);  epi: any of "b" bias, "r" ReLU, "m" ReLU mask (ldm = N + 3), "+" accumulate, "c" a_colsum;
# ws: "full" (16 MiB) | "short" (16 KiB, counters only) | None (NULL).
Case = collections.namedtuple("Case", "name ta tb M N K pa pb off epi ws leaf")
TA_TB = {v: k for k, v in LAYOUT.items()}
CASES = []


def _add(leaf, lay, M, N, K, epi="", pa=0, pb=0, off=0, ws="full"):
    ta, tb = TA_TB[lay]
    name = "%s_%dx%dx%d_%s_p%d%d_o%d_%s" % (lay, M, N, K, epi or "plain", pa, pb, off, ws or "nows")
    assert name not in [c.name for c in CASES], name
    CASES.append(Case(name, ta, tb, M, N, K, pa, pb, off, epi, ws, leaf))


def SK(lay, nw, u):
    return Leaf("skinny", lay, None, (nw, u), 1, "none")


def T64(lay, vec, ku, splits=1, red="none"):
    return Leaf("tiled64", lay, vec, ku, splits, red)


def T128(lay, vec):
    return Leaf("tiled128", lay, vec, 1, 1, "none")


# ---- skinny kernel: K = 8 (NW = 4, waves 1-3 empty), 72 (ragged per = 24), 512 (NW = 8, U = 4), 1024 (U = 8); clamped rows
for _lay in ("nt", "nn", "tn"):
    _c = "c" if _lay == "tn" else ""
    _add(SK(_lay, 4, 4), _lay, 1, 70, 8, "b")
    _add(SK(_lay, 4, 4), _lay, 31, 33, 8, "+" + _c, pa=4)
    _add(SK(_lay, 4, 4), _lay, 33, 31, 72, "r", pb=8)
    _add(SK(_lay, 4, 4), _lay, 70, 1, 72, "m")
    _add(SK(_lay, 4, 4), _lay, 70, 70, 72, "brm+" + _c, pa=4, pb=4)
    _add(SK(_lay, 8, 4), _lay, 33, 70, 512, "b+" + _c)
    _add(SK(_lay, 8, 4), _lay, 70, 31, 512, "m", pa=8, pb=4)
    _add(SK(_lay, 8, 8), _lay, 31, 70, 1024, "br")
    _add(SK(_lay, 8, 8), _lay, 70, 33, 1024, _c, pb=4)
    _add(SK(_lay, 4, 4), _lay, 70, 256, 72, "b" + _c)          # NT = 8: XCD remap on
    _add(SK(_lay, 4, 4), _lay, 70, 225, 72, "m" + _c)          # NT = 8 with a ragged last column tile
    _add(SK(_lay, 4, 4), _lay, 70, 193, 72, "+")               # NT = 7: remap off
    _add(SK(_lay, 4, 4), _lay, 33, 70, 72, ws=None)            # (the split logic never applies: K < 128)
_add(SK("nt", 8, 4), "nt", 600, 512, 512, "b")                 # second shape rule: N * K <= 512 * 512, M <= 1536
_add(SK("nn", 8, 4), "nn", 600, 512, 512, "+")
_add(SK("tn", 8, 4), "tn", 512, 512, 600, "c")                 # ... its transA form: M * N <= 512 * 512, K <= 1536
_add(SK("nt", 4, 4), "nt", 64, 64, 256, ws=None)               # plain split wanted, no workspace: the library clears C, then
_add(SK("nt", 4, 4), "nt", 64, 64, 256, "+", ws=None)          # the skinny kernel takes the shape anyway (and must not clear on +=)
for _k in (1, 7, 13):                                          # K % 8 != 0 on the m-contiguous layout (per-element k guards)
    _add(SK("tn", 4, 4), "tn", 33, 31, _k, "c" if _k != 7 else "b+c")
_add(SK("tn", 4, 4), "tn", 70, 70, 13, "m", off=1)             # no alignment rule for m-contiguous operands
_add(SK("tn", 4, 4), "tn", 45, 256, 72, "+c", pa=3)            # a_colsum with M % 32 != 0 and the remap on, odd lda

# ---- 64x64 tiles.  nt / nn stay off the skinny route through K % 8 == 4 or the one-float offset, tt is never skinny, tn
# needs K > 1536 (small M * N) or M * N > 512 * 512 with K > 512.
for _lay in ("nt", "nn", "tt"):
    _add(T64(_lay, True, 4), _lay, 100, 72, 4, "b")
    _add(T64(_lay, True, 4), _lay, 100, 72, 20, "m+", pa=4, pb=8)
    _add(T64(_lay, True, 4), _lay, 100, 72, 36, "br")
    _add(T64(_lay, False, 1), _lay, 101, 70, 20, "b", off=1)
    _add(T64(_lay, False, 1), _lay, 101, 70, 37, "rm+")
    _add(T64(_lay, True, 4, 2, "slabs"), _lay, 100, 72, 132, "b")       # slices 128 + 4
    _add(T64(_lay, True, 4, 2, "slabs"), _lay, 100, 72, 196, "m+")      # asks for 3, runs 128 + 68
    _add(T64(_lay, True, 4, 2, "slabs"), _lay, 100, 72, 132, "br", pa=4)
    _add(T64(_lay, True, 4, 2, "slabs"), _lay, 100, 72, 132)
    _add(T64(_lay, True, 4, 2, "atomics"), _lay, 100, 72, 132, ws="short")
    _add(T64(_lay, True, 4, 2, "atomics"), _lay, 100, 72, 196, "+", ws=None)
    _add(T64(_lay, True, 4, 2, "atomics"), _lay, 100, 72, 132, ws=None)             # the library's 2-D memset clears M x N
    _add(T64(_lay, True, 4, 1, "forced1"), _lay, 100, 72, 132, "b", ws=None)
    _add(T64(_lay, True, 4, 1, "forced1"), _lay, 100, 72, 196, "m+", ws="short")
    _add(T64(_lay, False, 1, 2, "slabs"), _lay, 101, 70, 132, "b", off=1)           # slices 80 + 52
    _add(T64(_lay, False, 1, 3, "slabs"), _lay, 101, 70, 196, "rm+", off=1)         # slices 80 + 80 + 36
    _add(T64(_lay, False, 1, 3, "atomics"), _lay, 101, 70, 197, "+", ws="short")
    _add(T64(_lay, False, 1, 2, "atomics"), _lay, 101, 70, 133, ws=None)
    _add(T64(_lay, False, 1, 1, "forced1"), _lay, 101, 70, 133, "r", ws=None)
    _add(T64(_lay, True, 2), _lay, 1088, 2048, 36, "b")                             # 544 tiles > 512: KU = 2
_add(T64("tt", True, 4), "tt", 100, 70, 20, "c")                                    # a_colsum on (1, 1), no split
_add(T64("tt", True, 4, 2, "slabs"), "tt", 100, 70, 132, "c")
_add(T64("tt", True, 4), "tt", 100, 60, 20, "c")                                    # ONE column tile: a_colsum fed by any tile
_add(T64("tn", True, 4, 7, "slabs"), "tn", 100, 60, 1540, "c")                      # row but y == 0 would then be missing
_add(T64("tt", True, 4, 2, "atomics"), "tt", 100, 70, 196, "+c", ws=None)
_add(T64("tt", False, 1, 3, "slabs"), "tt", 101, 70, 196, "bc")
_add(T64("tn", True, 4), "tn", 900, 900, 516, "bc")                                 # 225 tiles: no split, not skinny
_add(T64("tn", False, 1), "tn", 900, 900, 516, "+c", off=1)
_add(T64("tn", True, 2), "tn", 1500, 1500, 20, "m")                                 # 2209 32x32 tiles > 2048: not skinny
_add(T64("tn", True, 4, 7, "slabs"), "tn", 100, 72, 1540, "b+c")                    # asks for 8, runs 6 x 256 + 4
_add(T64("tn", True, 4, 7, "slabs"), "tn", 100, 72, 1540, "c", pa=4, pb=4)
_add(T64("tn", True, 4, 7, "atomics"), "tn", 100, 72, 1540, "c", ws="short")
_add(T64("tn", True, 4, 7, "atomics"), "tn", 100, 72, 1540, "+c", ws=None)
_add(T64("tn", True, 4, 1, "forced1"), "tn", 100, 72, 1540, "rc", ws="short")
_add(T64("tn", False, 1, 8, "slabs"), "tn", 101, 70, 1541, "mc")
_add(T64("tn", False, 1, 8, "atomics"), "tn", 101, 70, 1541, "c", ws=None)
_add(T64("tn", False, 1, 1, "forced1"), "tn", 101, 70, 1541, "b+c", ws=None)

# ---- 128x128 tiles (M >= 1024, N >= 256, >= 4096 64x64 tiles); K tiny so that the float64 reference costs nothing
_add(T128("nt", True), "nt", 4096, 4096, 36, "br")             # the FFN's epilogue
_add(T128("nt", False), "nt", 4096, 4096, 20, "+", off=1)
_add(T128("nn", True), "nn", 4096, 4096, 20, "m")
_add(T128("nn", False), "nn", 4096, 4096, 36, "b", off=1)
_add(T128("tn", True), "tn", 4096, 4096, 36, "c")
_add(T128("tn", False), "tn", 4096, 4096, 20, "+c", off=1)
_add(T128("tt", True), "tt", 4096, 4096, 20, "b+")
_add(T128("tt", False), "tt", 4096, 4096, 36, "r", off=1)

# ---- sbl_gemm2_f32: (name, M, N, K, pa, pb, off, bias, relu, ws, leaf)
Case2 = collections.namedtuple("Case2", "name M N K pa pb off bias relu ws leaf")
GEMM2_CASES = []


def _add2(leaf, M, N, K, bias=True, relu=False, pa=0, pb=0, off=0, ws="full"):
    name = "g2_%dx%dx%d_%s%s_p%d%d_o%d_%s" % (M, N, K, "b" if bias else "", "r" if relu else "", pa, pb, off, ws or "nows")
    GEMM2_CASES.append(Case2(name, M, N, K, pa, pb, off, bias, relu, ws, leaf))


_add2(SK("dual", 4, 4), 70, 58, 72)
_add2(SK("dual", 8, 4), 33, 70, 512, bias=False, pa=4)
_add2(SK("dual", 8, 8), 70, 33, 1024, relu=True)
_add2(SK("dual", 8, 4), 600, 512, 512)                                   # N * K <= 512 * 512, M <= 768
_add2(T64("dual", True, 4), 776, 64, 64, pa=8)                           # M > 768, K < 128: no split; M % 64 == 8
_add2(T64("dual", True, 4, 2, "slabs"), 776, 64, 128, relu=True)
_add2(T64("dual", True, 4, 2, "slabs"), 776, 60, 136, bias=False, pb=8)  # slices 128 + 8
_add2(T64("dual", True, 4, 1, "forced1"), 776, 64, 128, ws=None)
_add2(T64("dual", True, 4, 1, "forced1"), 776, 64, 136, ws="short")
_add2(T64("dual", True, 2), 776, 1344, 64)                               # 2 * 273 tiles > 512
_add2(T64("nt", True, 4), 100, 72, 36)                                   # K % 8 != 0: two sbl_gemm_f32 launches
_add2(T64("nt", False, 1), 101, 70, 40, off=1)                           # unaligned operands: two launches
_add2(T64("nt", True, 2), 1024, 8192, 40, bias=False)                    # 2 * 2048 tiles: "big" for the pair, not for each


# --------------------------------------------------------------------------- error bound of the rounded checks
U = 2.0 ** -24                      # fp32 unit roundoff
DROPPED6 = 2.0 ** -26               # include/sbl_hip.h, mode 6: plane products dropped per fp32 product, relative to |a b|


def extra_roundings(leaf, bias, accumulate, prec="f32"):
    """c of the bound (K + c) * U * (|A||B| + |bias| + |C0|): fp32 additions on an output element's path beyond the K
    fused multiply-adds of its K chain(s), counted from the launch geometry:
      splits - 1   the slab sum of the last-arriving workgroup, or the float atomics of the other slices;
      NW           the skinny kernel's LDS meet (0 + NW partial tiles);
      1            the 512-thread split-bf16 workgroups of an unsplit 64x64 launch meet once in LDS (bf16_tile.h, NH = 2);
      1 each       bias, and the += onto the previous C."""
    c = leaf.splits - 1
    if leaf.family == "skinny":
        c += leaf.ku[0]
    elif leaf.family == "tiled64" and prec != "f32" and leaf.splits == 1:
        c += 1
    return c + (1 if bias else 0) + (1 if accumulate else 0)


def dropped(leaf, prec):
    """Relative weight of the plane products mode `prec` drops on this leaf (the skinny kernel is exact fp32 in every mode)."""
    return DROPPED6 if prec == "bf16x6" and leaf.family != "skinny" else 0.0
