"""The host dispatch of the trunk convolutions restated in Python, and the case table of the route-aware convolution tests.

route_fwd() / route_dgrad() / route_wgrad() follow csrc/conv.hip (sbl_conv2d_fwd, conv2d_dgrad_impl, sbl_conv2d_wgrad,
conv_tile, wgrad_splits), csrc/conv_patch.h (sbl_conv_patch_tile, sbl_launch_conv_patch), csrc/conv_patch_wgrad.h
(sbl_conv_patch_wgrad_geom, sbl_launch_conv_patch_wgrad), csrc/mfma_gemm.h (sbl_launch_gemm, sbl_launch_gemm_tailsplit) and
the constants of csrc/tuning.h line by line - pure integer arithmetic, no torch, no GPU - and return the launch leaf:

    Leaf(family, tile, tr, g, classes, launches, splits)
      family    "gather" | "tailsplit" | "pm" | "patch" | "classes" | "patch_wgrad" | "pm_wgrad" | "wgrad"
                (sbl_profile_last_route() family 1 .. 8, include/sbl_hip.h)
      tile      (BM, BN) of the tile engine, None for the two patch-resident kernels
      tr, g     tile geometry of the patch-resident kernels: TR rows of one image (g == 1) or g whole images; 0 elsewhere
      classes   parity classes of a stride-2 input gradient that launch (4 for 3x3, 1 for 1x1); 0 elsewhere
      launches  kernel launches = stamp slots (2 for the tail split, else 1)
      splits    workgroups that meet on one output element: K slices of the tail split's second launch (slab sum), gridDim.z
                of a weight gradient (float atomics), gridDim.x of the patch-resident weight gradient (float atomics)

Every threshold below is a copy; the comment next to it names the line it mirrors.  tests/test_conv_routes_gpu.py asserts
the route the library reports against these functions, so a threshold that moves without this file fails there, and
tests/test_conv_routes_cpu.py holds route(case) to the leaf written BY HAND next to every case (never computed here).

Not reachable, and therefore not in all_leaves():
  * the two patch-resident kernels under "f32" (no fp32 instantiation: g_sbl_prec == 0 is refused first) - under f32 a
    "patch" case lands on "gather" or "pm", a "patch_wgrad" case on "wgrad" or "pm_wgrad";
  * "pm" on other tiles than 64x64 (launch_conv_pm is instantiated for 64x64 only), "pm" for 1x1 or stride-2 convolutions;
  * "tailsplit" for position-major, patch-resident or parity-class launches (only launch_conv_gemm tries it);
  * "pm_wgrad" with Cin % 128 != 0 or Cout < 128, "wgrad" on 128x128 tiles for stride 2 (sbl_wg_s2_small);
  * 128x64 tiles for weight gradients (square tiles only).

What the GPU module can compare with the library is what sbl_profile_last_route() and the stamp-slot count report: family,
tile, (TR, G) and launches.  `classes` and `splits` are NOT reported by the library; they are held to the hand-written
leaves on the CPU only, and on the GPU they enter through c of the rounded bound (extra_roundings) - a drift of wgrad_splits,
grid_z or the tail split's slice count in this mirror alone would loosen or tighten that bound, not fail a route assertion.
"""
import collections

Leaf = collections.namedtuple("Leaf", "family tile tr g classes launches splits")
FAMILY_ID = {"gather": 1, "tailsplit": 2, "pm": 3, "patch": 4, "classes": 5, "patch_wgrad": 6, "pm_wgrad": 7, "wgrad": 8}
TILE_ID = {None: 0, (64, 64): 1, (128, 64): 2, (128, 128): 3}      # csrc/sbl_common.h: sbl_route_tile
KID = {"fwd": 4, "dgrad": 5, "wgrad": 6}                           # csrc/sbl_common.h: SBL_KID_CONV_FWD / DGRAD / WGRAD

PRECS = ("f32", "bf16x6", "bf16x3", "bf16")
NPLANES = {"bf16x6": 3, "bf16x3": 2, "bf16": 1}      # conv_patch.h sbl_launch_conv_patch: npl
WS_COUNTERS = 4096                  # conv.hip: kConvWsCounters
WS_FULL = 16 << 20                  # ops.py: WS_BYTES
WS_SHORT = 4 * WS_COUNTERS          # the smallest workspace the entry points accept: counters only
WS_BYTES = {"full": WS_FULL, "short": WS_SHORT, None: None}
BK = 16                             # tile_loaders.h: SBL_BK
PM_MAX_HW = 121                     # tuning.h: sbl_pm_max_hw
WG_S2_SMALL = True                  # tuning.h: sbl_wg_s2_small
WG_S2_TARGET = 1536                 # tuning.h: sbl_wg_s2_target
WG_TARGET_BIG, WG_TARGET_SMALL = 1536, 3072      # conv.hip sbl_conv2d_wgrad: "big ? 1536 : 3072"
PM_WG64_MAX_M = 512                 # tuning.h: sbl_pm_wg64_max_m
PATCH_WGRAD_CUS = 256               # tuning.h: sbl_patch_wgrad_cus
KNOB5_DEFAULT, KNOB9_DEFAULT = 2, 30             # conv.hip: g_sbl_route = {2, 30}
CP_PIXB = 64                        # conv_patch.h: SBL_CP_PIXB
CP_BUDGET = 80 * 1024               # conv_patch.h sbl_conv_patch_tile: budget
CP_CAP = 512                        # conv_patch.h sbl_launch_conv_patch: cap (two workgroups per CU)
PWG_THREADS, PWG_XQ, PWG_DQ = 768, 5, 3          # conv_patch_wgrad.h: SBL_PWG_THREADS / _XQ / _DQ
PWG_LDS = 160 * 1024                # conv_patch_wgrad.h fits(): "<= 160 * 1024"
PWG_MIN_PIX = 80                    # conv_patch_wgrad.h: "G * TR * W < 80"


def cdiv(a, b):
    return (a + b - 1) // b


def out_dim(H, K, stride, pad):
    """conv.hip out_dim."""
    return (H + 2 * pad - K) // stride + 1


def conv_tile(N, t128, t128x64, waste_rule, no128):
    """conv.hip conv_tile."""
    waste128 = waste_rule and N >= 128 and 512 <= t128 < 1024 and cdiv(t128, 256) * 256 / t128 > 1.25
    skip128 = waste128 or no128
    if N >= 128 and t128 >= 512 and not skip128:
        return (128, 128)
    if (N < 128 or skip128) and t128x64 >= 512:
        return (128, 64)
    return (64, 64)


def patch_tile(H, W, nplanes):
    """conv_patch.h sbl_conv_patch_tile: (TR, G), or None where the map does not take the patch-resident kernel."""
    best = 0
    for tr in range(1, H + 1):
        if tr * W <= 256 and ((tr + 2) * (W + 2) + 64) * CP_PIXB * nplanes <= CP_BUDGET:
            best = tr
    if best >= H:
        g = 256 // (H * W)
        while g > 1 and (g * (H + 2) * (W + 2) + 64) * CP_PIXB * nplanes > CP_BUDGET:
            g -= 1
        g = max(g, 1)
        return (H, g) if g * H * W >= 224 or (g == 1 and H * W >= 160) else None
    if best <= 0:
        return None
    tr = cdiv(H, cdiv(H, best))
    return (tr, 1) if tr >= 4 and tr * W >= 160 else None


def patch_launch(prec, knob5, H, W, C, Nout):
    """conv_patch.h sbl_launch_conv_patch: (TR, G) or None (nothing launched)."""
    if not knob5 or prec == "f32" or C % 64 != 0 or Nout % 64 != 0:
        return None
    return patch_tile(H, W, NPLANES[prec])


def patch_grid(NIMG, H, Nout, tr, g):
    """conv_patch.h sbl_launch_conv_patch: (ntiles, gridDim.x)."""
    tpi = cdiv(H, tr)
    ntiles = cdiv(NIMG, g) if g > 1 else NIMG * tpi
    gy = Nout // 64
    capx = max(CP_CAP // gy, 1)
    return ntiles, min(ntiles, capx)


def patch_wgrad_geom(NIMG, H, W, nplanes):
    """conv_patch_wgrad.h sbl_conv_patch_wgrad_geom: dict of the PwgGeom fields, or None."""
    max_xrows = PWG_XQ * PWG_THREADS // 16
    max_pix = PWG_DQ * PWG_THREADS // 16 // 16 * 16
    PW = W + 4

    def fits(tr, g):
        xr, px = g * (tr + 2) * PW, g * tr * W
        dr = cdiv(px, 16) * 16
        return xr <= max_xrows and px <= max_pix and (xr + dr) * 128 * nplanes + dr * 4 <= PWG_LDS
    best = 0
    for tr in range(1, H + 1):
        if fits(tr, 1):
            best = tr
    if best <= 0:
        return None
    G = 1
    if best >= H:
        TR = H
        while fits(H, G + 1):
            G += 1
    else:
        TR = cdiv(H, cdiv(H, best))
    if G * TR * W < PWG_MIN_PIX:
        return None
    tpi = cdiv(H, TR)
    return {"TR": TR, "G": G, "tpi": tpi, "ntiles": cdiv(NIMG, G) if G > 1 else NIMG * tpi, "PW": PW, "PH": TR + 2,
            "xrows": G * (TR + 2) * PW, "dyrows": cdiv(G * TR * W, 16) * 16}


def patch_wgrad_launch(prec, knob9, NIMG, H, W, Cin, Cout):
    """conv_patch_wgrad.h sbl_launch_conv_patch_wgrad: (geometry, gridDim.x) or None."""
    if not knob9 or prec == "f32" or Cin % 64 != 0 or Cout % 64 != 0 or H * W < knob9:
        return None
    gm = patch_wgrad_geom(NIMG, H, W, NPLANES[prec])
    if gm is None:
        return None
    combos = (Cin // 64) * (Cout // 64)
    gx = min(max(PATCH_WGRAD_CUS // combos, 1), gm["ntiles"])
    return gm, gx


def tailsplit(M, N, K, BM, BN, ws_bytes):
    """mfma_gemm.h sbl_launch_gemm_tailsplit (KU = 1): gridDim.z of the split launch, or 0 where it does not apply."""
    X, Y = cdiv(M, BM), cdiv(N, BN)
    T = X * Y
    if ws_bytes is None or T <= 256 or T > 2048:
        return 0
    XA = (T // 256) * 256 // Y
    rem = T - XA * Y
    if XA <= 0 or rem <= 0 or rem > 176:
        return 0
    sp = min(256 // rem, K // (4 * BK), 8)
    if sp < 2 or rem > WS_COUNTERS:
        return 0
    if 4 * WS_COUNTERS + rem * sp * BM * BN * 4 > ws_bytes:
        return 0
    return cdiv(K, cdiv(cdiv(K, sp), BK) * BK)


def grid_z(K, splits):
    """mfma_gemm.h sbl_launch_gemm (KU = 1)."""
    return cdiv(K, cdiv(cdiv(K, splits), BK) * BK)


def wgrad_splits(target, tiles, K):
    """conv.hip wgrad_splits."""
    return max(1, min(cdiv(target, tiles), K // 256))


def pm_ok(Ho, Wo, k, stride):
    """conv.hip conv_pm_ok."""
    return k == 3 and stride == 1 and Ho * Wo <= PM_MAX_HW


def _gather(M, N, K, tile, ws_bytes):
    """conv.hip launch_tailsplit_or_plain."""
    nz = tailsplit(M, N, K, tile[0], tile[1], ws_bytes)
    if nz:
        return Leaf("tailsplit", tile, 0, 0, 0, 2, nz)
    return Leaf("gather", tile, 0, 0, 0, 1, 1)


def route_fwd(prec, knob5, NIMG, H, W, Cin, Cout, k, stride, stats=False, ws_bytes=WS_FULL):
    """Leaf of sbl_conv2d_fwd (the statistics epilogue never changes the route of a forward)."""
    pad = 1 if k == 3 else 0
    Ho, Wo = out_dim(H, k, stride, pad), out_dim(W, k, stride, pad)
    M, N, K = NIMG * Ho * Wo, Cout, k * k * Cin
    if k == 3 and stride == 1:
        t = patch_launch(prec, knob5, H, W, Cin, Cout)
        if t:
            return Leaf("patch", None, t[0], t[1], 0, 1, 1)
    if pm_ok(Ho, Wo, k, stride):
        return Leaf("pm", (64, 64), 0, 0, 0, 1, 1)
    tile = conv_tile(N, cdiv(M, 128) * cdiv(N, 128), cdiv(M, 128) * cdiv(N, 64), True, False)
    return _gather(M, N, K, tile, ws_bytes)


def dgrad_classes(NIMG, H, W, k):
    """conv.hip conv2d_dgrad_impl, stride 2: [(ph, pw, rows M, taps)] heaviest first (stable insertion as in the source)."""
    pad = 1 if k == 3 else 0
    cls = []
    for ph in (0, 1):
        for pw in (0, 1):
            taps = [(kh, kw) for kh in range(k) for kw in range(k) if (ph + pad - kh) % 2 == 0 and (pw + pad - kw) % 2 == 0]
            Mc = NIMG * ((H - ph + 1) // 2) * ((W - pw + 1) // 2)
            if not taps or Mc == 0:
                continue
            at = len(cls)
            while at > 0 and len(cls[at - 1][3]) < len(taps):
                at -= 1
            cls.insert(at, (ph, pw, Mc, taps))
    return cls


def route_dgrad(prec, knob5, NIMG, H, W, Cin, Cout, k, stride, sums=False, ws_bytes=WS_FULL):
    """Leaf of conv2d_dgrad_impl; sums: the launch carries the BatchNorm-backward sums (the addend never routes)."""
    N = Cin
    if stride == 2:
        cls = dgrad_classes(NIMG, H, W, k)
        t128 = sum(cdiv(c[2], 128) * cdiv(N, 128) for c in cls)
        t128x64 = sum(cdiv(c[2], 128) * cdiv(N, 64) for c in cls)
        return Leaf("classes", conv_tile(N, t128, t128x64, False, sums), 0, 0, len(cls), 1, 1)
    M, K = NIMG * H * W, k * k * Cout
    if k == 3:
        t = patch_launch(prec, knob5, H, W, Cout, Cin)
        if t:
            return Leaf("patch", None, t[0], t[1], 0, 1, 1)
    if pm_ok(H, W, k, stride):
        return Leaf("pm", (64, 64), 0, 0, 0, 1, 1)
    tile = conv_tile(N, cdiv(M, 128) * cdiv(N, 128), cdiv(M, 128) * cdiv(N, 64), True, sums)
    return _gather(M, N, K, tile, ws_bytes)


def route_wgrad(prec, knob9, NIMG, H, W, Cin, Cout, k, stride):
    """Leaf of sbl_conv2d_wgrad."""
    pad = 1 if k == 3 else 0
    Ho, Wo = out_dim(H, k, stride, pad), out_dim(W, k, stride, pad)
    M, N, K = Cout, k * k * Cin, NIMG * Ho * Wo
    big = M >= 128 and N >= 1152 and not (stride == 2 and WG_S2_SMALL)
    target = WG_S2_TARGET if stride == 2 else (WG_TARGET_BIG if big else WG_TARGET_SMALL)
    if k == 3 and stride == 1:
        t = patch_wgrad_launch(prec, knob9, NIMG, H, W, Cin, Cout)
        if t:
            return Leaf("patch_wgrad", None, t[0]["TR"], t[0]["G"], 0, 1, t[1])
    if pm_ok(Ho, Wo, k, stride) and big and M >= 128 and Cin % 128 == 0:
        T = 64 if M <= PM_WG64_MAX_M else 128
        return Leaf("pm_wgrad", (T, T), 0, 0, 0, 1, wgrad_splits(target if T == 128 else 2 * target, cdiv(M, T) * cdiv(N, T), K))
    T = 128 if big and M >= 128 else 64
    return Leaf("wgrad", (T, T), 0, 0, 0, 1, grid_z(K, wgrad_splits(target, cdiv(M, T) * cdiv(N, T), K)))


def route_code(leaf):
    """What sbl_profile_last_route() reports for the leaf (include/sbl_hip.h)."""
    return (FAMILY_ID[leaf.family] << 24) | (TILE_ID[leaf.tile] << 20) | (leaf.tr << 10) | leaf.g


# --------------------------------------------------------------------------- every reachable leaf
def patch_kind(leaf, H):
    """rows: TR rows of an image; whole: one whole image per tile; multi: several images per tile."""
    return "multi" if leaf.g > 1 else "whole" if leaf.tr >= H else "rows"


def leaf_key(case, leaf):
    """Identity of a leaf for the coverage check: operation, stride, family, tile and - patch kernels - the kind of tile;
    stride-2 launches add the class count, weight gradients whether more than one workgroup meets on an element."""
    if leaf.family in ("patch", "patch_wgrad"):
        return (case.op, leaf.family, patch_kind(leaf, case.H))
    if leaf.family == "classes":
        return (case.op, leaf.family, leaf.tile, leaf.classes)
    if leaf.family in ("wgrad", "pm_wgrad"):
        return (case.op, leaf.family, leaf.tile, "s%d" % case.stride, leaf.splits > 1)
    return (case.op, leaf.family, leaf.tile)


T64, T128x64, T128 = (64, 64), (128, 64), (128, 128)


def all_leaves():
    """Every reachable leaf key of the three dispatch trees (module docstring: what is not reachable, and why)."""
    out = set()
    for op in ("fwd", "dgrad"):
        for t in (T64, T128x64, T128):
            out.add((op, "gather", t))
            out.add((op, "tailsplit", t))
        out.add((op, "pm", T64))
        for kind in ("rows", "whole", "multi"):
            out.add((op, "patch", kind))
    for t in (T64, T128x64, T128):
        out.add(("dgrad", "classes", t, 4))
        out.add(("dgrad", "classes", t, 1))             # 1x1 / stride 2: the even/even class alone
    for kind in ("rows", "whole", "multi"):
        out.add(("wgrad", "patch_wgrad", kind))
    for t in (T64, T128):
        for many in (False, True):
            out.add(("wgrad", "pm_wgrad", t, "s1", many))
            out.add(("wgrad", "wgrad", t, "s1", many))
    for many in (False, True):
        out.add(("wgrad", "wgrad", T64, "s2", many))
    return out


# --------------------------------------------------------------------------- case table
# op "fwd" | "dgrad" | "wgrad";  epi: forward "" | "stats"; input gradient "" plain | "a" addend | "s" sums | "sa" sums +
# addend | "sa2" sums + addend + second BatchNorm | "c" compact output (1x1 / stride 2);  weight gradient "" | "+"
# (dw_zeroed = 1 onto previous contents);  ws "full" | "short" | None;  k5 / k9: the two sbl_set_tuning knobs;
# leaf: {precision: Leaf}, written by hand.
Case = collections.namedtuple("Case", "name op NIMG H W Cin Cout k stride epi ws k5 k9 leaf")
CASES = []


def _add(op, shape, leaf, epi="", ws="full", k5=KNOB5_DEFAULT, k9=KNOB9_DEFAULT):
    NIMG, H, W, Cin, Cout, k, stride = shape
    if isinstance(leaf, Leaf):
        leaf = (leaf,) * 4
    elif len(leaf) == 2:                                 # (f32, the three split-bf16 modes)
        leaf = (leaf[0],) + (leaf[1],) * 3
    assert len(leaf) == 4
    name = "%s_%dx%dx%d_%dto%d_k%ds%d_%s_%s_k%d_%d" % (op, NIMG, H, W, Cin, Cout, k, stride, epi or "plain", ws or "nows", k5, k9)
    assert name not in [c.name for c in CASES], name
    CASES.append(Case(name, op, NIMG, H, W, Cin, Cout, k, stride, epi, ws, k5, k9, dict(zip(PRECS, leaf))))


def GA(tile):
    return Leaf("gather", tile, 0, 0, 0, 1, 1)


def TS(tile, nz):
    return Leaf("tailsplit", tile, 0, 0, 0, 2, nz)


PM = Leaf("pm", T64, 0, 0, 0, 1, 1)


def PA(tr, g):
    return Leaf("patch", None, tr, g, 0, 1, 1)


def CL(tile, n):
    return Leaf("classes", tile, 0, 0, n, 1, 1)


def PW(tr, g, gx):
    return Leaf("patch_wgrad", None, tr, g, 0, 1, gx)


def PMW(tile, splits):
    return Leaf("pm_wgrad", tile, 0, 0, 0, 1, splits)


def WG(tile, nz):
    return Leaf("wgrad", tile, 0, 0, 0, 1, nz)


# ---- forward, 3x3 / stride 1, patch-resident in the split-bf16 modes (f32: per-tap gather above 121 pixels, else position-major)
_add("fwd", (3, 22, 22, 64, 64, 3, 1), (GA(T64), PA(11, 1)), "stats")               # even row split 11 + 11
_add("fwd", (3, 23, 22, 64, 64, 3, 1), (GA(T64), PA(8, 1)))                         # uneven: 8 + 8 + 7
_add("fwd", (3, 13, 13, 64, 128, 3, 1), (GA(T64), PA(13, 1)), "stats")              # one whole image per tile
_add("fwd", (5, 11, 11, 64, 64, 3, 1), (PM, PA(11, 2)), "stats")                    # two images per tile, last tile one
_add("fwd", (10, 6, 6, 64, 64, 3, 1), (PM, PM, PA(6, 7), PA(6, 7)), "stats")        # 7 per tile, last tile 3
_add("fwd", (7, 7, 7, 64, 64, 3, 1), (PM, PM, PA(7, 5), PA(7, 5)))                  # 5 per tile, last tile 2
_add("fwd", (19, 4, 4, 64, 64, 3, 1), (PM, PM, PA(4, 16), PA(4, 16)), "stats")      # 16 per tile, last tile 3
_add("fwd", (14, 4, 5, 64, 128, 3, 1), (PM, PM, PA(4, 12), PA(4, 12)))              # 12 per tile, last tile 2
_add("fwd", (30, 3, 3, 64, 64, 3, 1), (PM, PM, PM, PA(3, 28)), "stats")             # 28 per tile at one plane only, last tile 2
_add("fwd", (5, 9, 9, 64, 64, 3, 1), (PM, PM, PA(9, 3), PA(9, 3)), "stats")         # refused at three planes by 64 bytes
_add("fwd", (5, 8, 8, 64, 64, 3, 1), (PM, PM, PA(8, 4), PA(8, 4)))                  # refused at three planes (3 images: 192 pixels)
# persistent workgroups that walk two tiles, 514 tiles on 512 workgroups (f32: 972 128x64 tiles, 204 left over: no tail split)
_add("fwd", (257, 22, 22, 64, 64, 3, 1), (GA(T128x64), PA(11, 1)), "stats")
_add("fwd", (1027, 11, 11, 64, 64, 3, 1), (PM, PA(11, 2)), "stats")
_add("fwd", (8211, 4, 4, 64, 64, 3, 1), (PM, PM, PA(4, 16), PA(4, 16)), "stats")
_add("fwd", (14366, 3, 3, 64, 64, 3, 1), (PM, PM, PM, PA(3, 28)))
# ---- forward, position-major in every mode: knob 5 = 0, a map no plane count accepts (4x11: 5 images = 220 pixels), C % 64 != 0
_add("fwd", (150, 3, 3, 64, 64, 3, 1), PM, "stats", k5=0)                           # 64-row tiles inside one position and across two
_add("fwd", (70, 6, 6, 64, 64, 3, 1), PM, k5=0)                                     # every tile straddles two positions
_add("fwd", (9, 5, 4, 64, 64, 3, 1), PM, "stats", k5=0)                             # a tile covers 7 positions
_add("fwd", (70, 4, 11, 64, 64, 3, 1), PM, "stats")
_add("fwd", (9, 5, 4, 48, 80, 3, 1), PM, "stats")                                   # multiples of 16, not of 64
# ---- forward, per-tap gather: f32, knob 5 = 0, C % 64 != 0; the three tiles; waste_rule; tail split taken and refused
_add("fwd", (3, 22, 22, 64, 64, 3, 1), GA(T64), "stats", k5=0)
_add("fwd", (3, 14, 14, 48, 80, 3, 1), GA(T64), "stats")
_add("fwd", (456, 12, 12, 16, 16, 1, 1), GA(T128x64), "stats")                      # 513 128x64 tiles (512 would stay on 64x64)
_add("fwd", (455, 12, 12, 16, 128, 1, 1), GA(T128), "stats")                        # 512 128x128 tiles
_add("fwd", (533, 12, 12, 16, 128, 1, 1), GA(T128x64))                              # 600 128x128 tiles round up by 28 %: waste_rule
_add("fwd", (40, 22, 22, 64, 64, 3, 1), TS(T64, 5), "stats", k5=0)                  # 303 tiles = 256 + 47 split 5 ways
_add("fwd", (40, 22, 22, 128, 64, 1, 1), TS(T64, 2), "stats")                       # K = 128: 2 slices of 4 steps
_add("fwd", (40, 22, 22, 128, 64, 1, 1), GA(T64), "stats", ws=None)                 # no workspace: one plain launch
_add("fwd", (40, 22, 22, 128, 64, 1, 1), GA(T64), ws="short")                       # counters only: one plain launch
_add("fwd", (533, 12, 12, 128, 64, 1, 1), TS(T128x64, 2), "stats")                  # 600 tiles = 512 + 88 split 2 ways
_add("fwd", (551, 12, 12, 128, 128, 1, 1), TS(T128, 2))                             # 620 tiles = 512 + 108 split 2 ways
# ---- forward, stride 2
_add("fwd", (5, 22, 22, 64, 128, 3, 2), GA(T64), "stats")
_add("fwd", (5, 22, 22, 64, 128, 3, 2), GA(T64))
_add("fwd", (3, 7, 5, 64, 64, 3, 2), GA(T64), "stats")                              # odd map: 4 x 3 outputs
_add("fwd", (5, 22, 22, 64, 128, 1, 2), GA(T64))
_add("fwd", (3, 7, 5, 32, 48, 1, 2), GA(T64), "stats")

# ---- input gradient, stride 1 (Cin = output channels N of the GEMM, Cout = depth)
_add("dgrad", (3, 22, 22, 64, 64, 3, 1), (GA(T64), PA(11, 1)), "sa")
_add("dgrad", (3, 23, 22, 64, 128, 3, 1), (GA(T64), PA(8, 1)), "s")
_add("dgrad", (3, 13, 13, 128, 64, 3, 1), (GA(T64), PA(13, 1)), "a")
_add("dgrad", (5, 11, 11, 64, 64, 3, 1), (PM, PA(11, 2)), "sa2")
_add("dgrad", (10, 6, 6, 64, 64, 3, 1), (PM, PM, PA(6, 7), PA(6, 7)), "a")
_add("dgrad", (7, 7, 7, 64, 64, 3, 1), (PM, PM, PA(7, 5), PA(7, 5)), "sa")
_add("dgrad", (19, 4, 4, 64, 64, 3, 1), (PM, PM, PA(4, 16), PA(4, 16)))
_add("dgrad", (14, 5, 4, 64, 64, 3, 1), (PM, PM, PA(5, 12), PA(5, 12)), "s")
_add("dgrad", (30, 3, 3, 64, 64, 3, 1), (PM, PM, PM, PA(3, 28)), "sa2")
_add("dgrad", (5, 9, 9, 64, 64, 3, 1), (PM, PM, PA(9, 3), PA(9, 3)), "sa")
_add("dgrad", (257, 22, 22, 64, 64, 3, 1), (GA(T128x64), PA(11, 1)), "sa")          # two tiles per workgroup, sums carried over
_add("dgrad", (8211, 4, 4, 64, 64, 3, 1), (PM, PM, PA(4, 16), PA(4, 16)), "s")
_add("dgrad", (70, 4, 11, 64, 64, 3, 1), PM, "s")
_add("dgrad", (150, 3, 3, 64, 64, 3, 1), PM, "sa", k5=0)
_add("dgrad", (9, 5, 4, 48, 80, 3, 1), PM, "sa2")
_add("dgrad", (9, 5, 4, 80, 48, 3, 1), PM)
_add("dgrad", (3, 22, 22, 64, 64, 3, 1), GA(T64), "", k5=0)
_add("dgrad", (3, 14, 14, 48, 80, 3, 1), GA(T64), "sa2")
_add("dgrad", (456, 12, 12, 16, 16, 1, 1), GA(T128x64), "a")
_add("dgrad", (455, 12, 12, 128, 16, 1, 1), GA(T128))                               # 512 128x128 tiles ...
_add("dgrad", (455, 12, 12, 128, 16, 1, 1), GA(T128), "a")
_add("dgrad", (455, 12, 12, 128, 16, 1, 1), GA(T128x64), "s")                       # ... and the no128 arm with the sums epilogue
_add("dgrad", (533, 12, 12, 128, 16, 1, 1), GA(T128x64))                            # waste_rule
_add("dgrad", (40, 22, 22, 64, 128, 1, 1), TS(T64, 2), "sa")                        # the last arriver runs the sums epilogue
_add("dgrad", (40, 22, 22, 64, 128, 1, 1), GA(T64), "s", ws=None)
_add("dgrad", (40, 22, 22, 64, 128, 1, 1), GA(T64), "a", ws="short")
_add("dgrad", (533, 12, 12, 64, 128, 1, 1), TS(T128x64, 2), "s")
_add("dgrad", (551, 12, 12, 128, 128, 1, 1), TS(T128, 2), "a")
# every epilogue flavour on every stride-1 route (the flavours listed above are left out here)
for _shape, _leaf, _have in (((3, 22, 22, 64, 64, 3, 1), (GA(T64), PA(11, 1)), ("sa",)),            # gather (f32) / patch, row split
                             ((5, 11, 11, 64, 64, 3, 1), (PM, PA(11, 2)), ("sa2",)),                # position-major (f32) / patch, 2 images
                             ((70, 4, 11, 64, 64, 3, 1), PM, ("s",)),                               # position-major in every mode
                             ((3, 14, 14, 48, 80, 3, 1), GA(T64), ("sa2",)),                        # gather in every mode
                             ((40, 22, 22, 64, 128, 1, 1), TS(T64, 2), ("sa",))):                   # tail split in every mode
    for _epi in ("", "a", "s", "sa", "sa2"):
        if _epi not in _have:
            _add("dgrad", _shape, _leaf, _epi)
# ---- input gradient, stride 2: parity classes
_add("dgrad", (5, 22, 22, 64, 128, 3, 2), CL(T64, 4))
_add("dgrad", (2, 7, 5, 64, 64, 3, 2), CL(T64, 4), "sa")                            # odd H and W, compact addend on class (0, 0), one BatchNorm
_add("dgrad", (2, 5, 3, 64, 64, 3, 2), CL(T64, 4), "s")                             # 1-pixel-wide sub-grids of the odd-column classes
_add("dgrad", (3, 2, 2, 32, 48, 3, 2), CL(T64, 4), "sa2")                           # 2x2 map: every class one pixel per image
_add("dgrad", (2, 6, 7, 48, 32, 3, 2), CL(T64, 4), "a")
_add("dgrad", (136, 22, 22, 16, 16, 3, 2), CL(T128x64, 4), "s")                     # 4 x 129 = 516 128x64 tiles
_add("dgrad", (136, 22, 22, 128, 16, 3, 2), CL(T128, 4))                            # 516 128x128 tiles
_add("dgrad", (136, 22, 22, 128, 16, 3, 2), CL(T128x64, 4), "s")                    # no128
_add("dgrad", (5, 22, 22, 64, 128, 1, 2), CL(T64, 1))                               # 1x1: the even/even class alone, odd pixels zero
_add("dgrad", (3, 7, 5, 32, 48, 1, 2), CL(T64, 1))
_add("dgrad", (5, 22, 22, 64, 128, 1, 2), CL(T64, 1), "c")                          # compact output
_add("dgrad", (3, 7, 5, 32, 48, 1, 2), CL(T64, 1), "c")
_add("dgrad", (544, 22, 22, 16, 16, 1, 2), CL(T128x64, 1))                          # 544 * 121 even pixels = 515 128x64 tiles
_add("dgrad", (544, 22, 22, 16, 16, 1, 2), CL(T128x64, 1), "c")
_add("dgrad", (65700, 1, 2, 128, 16, 1, 2), CL(T128, 1))                            # 1x2 maps: 514 128x128 tiles, every second pixel zero
_add("dgrad", (65700, 1, 2, 128, 16, 1, 2), CL(T128, 1), "c")

# ---- weight gradient
_add("wgrad", (3, 22, 22, 64, 64, 3, 1), (WG(T64, 5), PW(6, 1, 12)))                # rows 6 + 6 + 6 + 4; f32: K = 1452 in 5 slices
_add("wgrad", (3, 23, 22, 64, 128, 3, 1), (WG(T64, 5), PW(6, 1, 12)), "+")          # rows 6 + 6 + 6 + 5; K = 1518
_add("wgrad", (3, 24, 22, 64, 64, 3, 1), (WG(T64, 6), PW(6, 1, 12)))                # even row split 6 + 6 + 6 + 6; f32: K = 1584
_add("wgrad", (5, 11, 11, 64, 64, 3, 1), (WG(T64, 2), PW(11, 1, 5)))                # one image per tile; K = 605
_add("wgrad", (10, 6, 6, 64, 64, 3, 1), (WG(T64, 1), PW(6, 3, 4)), "+")             # 3 images per tile, last tile one; K = 360
_add("wgrad", (65, 22, 22, 64, 64, 3, 1), (WG(T64, 116), PW(6, 1, 256)))            # 260 tiles on 256 workgroups (f32: K = 31460 asks
                                                                                    # for 122 slices, chunks of 272 make 116)
_add("wgrad", (17, 22, 22, 128, 128, 3, 1), (WG(T128, 31), PW(6, 1, 64)))           # 68 tiles on 64 workgroups per channel block
                                                                                    # (f32: K = 8228 asks for 32, chunks of 272 make 31)
_add("wgrad", (40, 5, 5, 64, 64, 3, 1), WG(T64, 3))                                 # knob 9: 25 pixels < 30
_add("wgrad", (30, 12, 3, 64, 64, 3, 1), WG(T64, 4))                                # 2 images per tile = 72 pixels < 80: refused
_add("wgrad", (3, 22, 22, 64, 64, 3, 1), WG(T64, 5), k9=0)
_add("wgrad", (9, 5, 5, 128, 128, 3, 1), PMW(T64, 1))                               # position-major (25 pixels: knob 9 keeps the patch kernel out)
_add("wgrad", (21, 5, 5, 128, 128, 3, 1), PMW(T64, 2), "+")
_add("wgrad", (9, 5, 5, 128, 640, 3, 1), PMW(T128, 1))                              # Cout > 512: 128x128 tiles
_add("wgrad", (21, 5, 5, 128, 640, 3, 1), PMW(T128, 2))
_add("wgrad", (7, 11, 11, 128, 128, 3, 1), PMW(T64, 3), k9=0)                       # 11x11: the largest position-major map
_add("wgrad", (9, 5, 5, 144, 128, 3, 1), WG(T128, 1))                               # Cin % 128 != 0: plain 128x128
_add("wgrad", (3, 14, 14, 128, 128, 3, 1), WG(T128, 2), k9=0)                       # 196 pixels > 121: plain 128x128, K = 588
_add("wgrad", (5, 22, 22, 64, 128, 3, 2), WG(T64, 2))                               # stride 2: 64x64 tiles, K = 605
_add("wgrad", (60, 6, 6, 128, 128, 3, 2), WG(T64, 2), "+")                          # 128+ channels at stride 2 stay on 64x64; K = 540
_add("wgrad", (3, 7, 5, 64, 64, 3, 2), WG(T64, 1))                                  # K = 36
_add("wgrad", (5, 22, 22, 64, 128, 1, 2), WG(T64, 2))                               # 1x1 / stride 2
_add("wgrad", (3, 7, 5, 32, 48, 1, 2), WG(T64, 1), "+")


def route(case, prec):
    c = case
    if c.op == "fwd":
        return route_fwd(prec, c.k5, c.NIMG, c.H, c.W, c.Cin, c.Cout, c.k, c.stride, c.epi == "stats", WS_BYTES[c.ws])
    if c.op == "dgrad":
        return route_dgrad(prec, c.k5, c.NIMG, c.H, c.W, c.Cin, c.Cout, c.k, c.stride, "s" in c.epi, WS_BYTES[c.ws])
    return route_wgrad(prec, c.k9, c.NIMG, c.H, c.W, c.Cin, c.Cout, c.k, c.stride)


# --------------------------------------------------------------------------- error bound of the rounded checks
U = 2.0 ** -24                      # fp32 unit roundoff
DROPPED6 = 2.0 ** -26               # include/sbl_hip.h, mode 6: plane products dropped per fp32 product, relative to |a b|


def extra_roundings(leaf, addend=False, previous=False):
    """c of the bound (K + c) * U * conv(|a|, |b|): fp32 additions on an output element's path beyond its K products:
      splits - 1   slab additions of the tail split's last arriver / float atomics of the other weight-gradient workgroups;
      1            the first atomic onto the zeroed (or previous) dw of a weight gradient;
      1 each       the addend, the previous contents of dw."""
    c = leaf.splits - 1
    if leaf.family in ("wgrad", "pm_wgrad", "patch_wgrad"):
        c += 1
    return c + (1 if addend else 0) + (1 if previous else 0)
