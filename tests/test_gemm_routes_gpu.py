"""The dense GEMM family, leaf by leaf of its host dispatch: sbl_gemm_f32, sbl_gemm2_f32, sbl_wgrad_seg_f32,
sbl_wgrad_group_f32 and sbl_colsum_f32 through the C ABI (ops.call), on tensors and a workspace this module allocates.

Every launch is checked three ways:
  * route: sbl_profile_last_kernel() is the family tests/gemm_routes.py predicts for the case (1 skinny, 2 64x64 tiles,
    3 128x128 tiles; 7 for the merged weight gradients) - a case that lands on another kernel FAILS;
  * frame: C lives in a buffer with ldc = N + 4 and a guard row above and below; pad columns, guard rows and the guards
    around a_colsum hold a sentinel that must survive bit for bit; operand padding (lda / ldb beyond the extent) is NaN, so
    a read beyond the extent poisons the output; the workspace is handed over with zero counters and NaN slabs, and
    the 4096 counters must be zero again after every launch;
  * value: EXACT in all four precisions on integer data (operands, bias, previous C and a_colsum in [-3, 3], mask in
    {-1, 0, 1}: one bf16 plane holds them, every fp32 partial sum in any order is an integer below 2^24, so the output
    must equal the integer result whatever the route, split count or precision), and ROUNDED under f32 and bf16x6 on
    detfill.uniform data against float64 with the derived elementwise bound
        |C - ref| <= (K + c) * U * (|A||B| + |bias| + |C0|)_mn   (+ 2^-26 * (|A||B|)_mn under bf16x6 on the tile engine)
    U = 2^-24; c = gemm_routes.extra_roundings(): slab additions or atomics (splits - 1), the skinny waves' LDS meet
    (NW), the wave-group meet of the unsplit split-bf16 64x64 launches (1), bias (1), += (1).  Why it is a bound: an
    output is a sum of K products (+ bias + C0) in some order; each product enters through one fused multiply-add and
    each further addition rounds once, so a term passes through at most K + c roundings of relative size U applied to
    partial sums no larger than the sum of magnitudes.  The a_colsum bound is the same over |A|: (K + c) * U *
    (sum_k |A| + |previous|), c = splits + 1 (K + 1 terms meet in K additions whatever the order of the atomics).
    Under bf16x6 one fp32 product is six exact plane products accumulated by v_mfma_f32_32x32x16_bf16, 16 k at a time;
    how often that instruction rounds inside is not documented, so the bound keeps one rounding per product plus the
    dropped planes, as include/sbl_hip.h states the mode - the measured ratios below say it holds with room.

check() prints the worst err / bound ratio of every comparison; the worst one measured on an MI355X is in each test's
docstring.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gemm_routes as R
from sbl_for_multilingual_lip_reading_amd import detfill

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = R.U
PRECS = ("f32", "bf16x6", "bf16x3", "bf16")
ROUNDED_PRECS = ("f32", "bf16x6")
SENT = -777.25                       # guard value (not an integer: never a legal exact result)
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def ops():
    from sbl_for_multilingual_lip_reading_amd import _lib, ops as _ops
    _lib.load()
    assert torch.cuda.is_available()
    prev = _ops.get_matmul_precision()
    yield _ops
    _ops.set_matmul_precision(prev)


@pytest.fixture(scope="module")
def wsbuf():
    return torch.zeros(R.WS_FULL // 4, dtype=torch.float32, device=DEV)


# --------------------------------------------------------------------------- helpers
def S():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    return None if t is None else t.data_ptr()


def kid():
    from sbl_for_multilingual_lip_reading_amd import _lib
    return _lib.load().sbl_profile_last_kernel()


def f64(a):
    return np.asarray(a, dtype=np.float64)


def ints(name, shape, hi=3):
    """Integers in [-hi, hi] as float32, a function of (name, shape)."""
    return np.rint(detfill.uniform(name, shape) * np.float32(hi)).astype(np.float32)


def fill(kind, name, shape):
    return ints(name, shape) if kind == "int" else detfill.uniform(name, shape)


def operand(a, ld, off):
    """Device copy of the 2-D host array `a` with row stride ld >= a.shape[1], `off` floats past a 16-byte boundary, NaN
    in the padding.  Returns (flat buffer, view that starts at the operand)."""
    rows, cols = a.shape
    buf = torch.full((rows * ld + 4,), NAN, dtype=torch.float32, device=DEV)
    view = buf[off:off + rows * ld].view(rows, ld)
    view[:, :cols] = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return buf, view


class Frame:
    """An M x N output inside (M + 2) x (N + 4): sentinel guard rows and pad columns around `init`."""

    def __init__(self, M, N, init):
        self.M, self.N, self.ld = M, N, N + 4
        self.buf = torch.full((M + 2, N + 4), SENT, dtype=torch.float32, device=DEV)
        self.buf[1:M + 1, :N] = init
        self.C = self.buf[1:M + 1]

    def ptr(self):
        return self.C.data_ptr()

    def out(self):
        return self.C[:, :self.N]

    def check_frame(self, what):
        g = self.buf.clone()
        g[1:self.M + 1, :self.N] = SENT
        assert bool((g == SENT).all()), what + ": a guard row or pad column was written"


def check(what, got, ref, bound):
    """|got - ref| <= bound elementwise, on the device in float64 (bound None: exact).  Returns worst err / bound."""
    got = got.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what + ": non-finite output"
    err = (got - ref).abs()
    if bound is None:
        bad = int((err != 0).sum())
        assert bad == 0, "%s: %d of %d elements differ from the integer result (max %.3e)" % (what, bad, ref.numel(), float(err.max()))
        return 0.0
    ratio = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                        torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    worst = float(ratio.max())
    print("%-60s worst err/bound %.3f  (max err %.3e)" % (what, worst, float(err.max())))
    assert worst <= 1.0, "%s: err/bound %.3f at flat index %d" % (what, worst, int(ratio.argmax()))
    return worst


def arm(ws, nbytes):
    """Hand the workspace over: zero counters, NaN slabs.  Returns (pointer, bytes)."""
    if nbytes is None:
        return None, 0
    ws[:R.WS_COUNTERS] = 0
    ws[R.WS_COUNTERS:] = NAN
    return ws.data_ptr(), nbytes


def counters_zero(ws, what):
    assert bool((ws[:R.WS_COUNTERS].view(torch.int32) == 0).all()), what + ": tile counters not re-armed"


WS_BYTES = {"full": R.WS_FULL, "short": R.WS_SHORT, None: None}


# --------------------------------------------------------------------------- sbl_gemm_f32
@functools.lru_cache(maxsize=2)
def gemm_problem(case, kind):
    """Device inputs, float64 reference and bound magnitudes of one (case, data kind), shared by the precisions."""
    c = case
    ar = (c.K, c.M) if c.ta else (c.M, c.K)
    br = (c.N, c.K) if c.tb else (c.K, c.N)
    A, B = fill(kind, "gr.A." + c.name, ar), fill(kind, "gr.B." + c.name, br)
    bias = fill(kind, "gr.b." + c.name, (c.N,)) if "b" in c.epi else None
    mask = ints("gr.m." + c.name, (c.M, c.N), 1) if "m" in c.epi else None
    C0 = fill(kind, "gr.C." + c.name, (c.M, c.N)) if "+" in c.epi else None
    cs0 = fill(kind, "gr.s." + c.name, (c.M,)) if "c" in c.epi else None
    opA, opB = (f64(A).T if c.ta else f64(A)), (f64(B).T if c.tb else f64(B))
    ref, mag = opA @ opB, np.abs(opA) @ np.abs(opB)
    prod_mag = mag
    if bias is not None:
        ref, mag = ref + f64(bias), mag + np.abs(f64(bias))
    if "r" in c.epi:
        ref = np.maximum(ref, 0.0)                       # 1-Lipschitz: the bound carries over
    if mask is not None:
        ref = np.where(mask > 0, ref, 0.0)
    if C0 is not None:
        ref, mag = ref + f64(C0), mag + np.abs(f64(C0))
    d = {"ref": torch.from_numpy(ref).to(DEV), "mag": torch.from_numpy(mag).to(DEV), "prod_mag": torch.from_numpy(prod_mag).to(DEV)}
    if cs0 is not None:
        d["cs_ref"] = torch.from_numpy(f64(cs0) + opA.sum(1)).to(DEV)
        d["cs_mag"] = torch.from_numpy(np.abs(f64(cs0)) + np.abs(opA).sum(1)).to(DEV)
    lda, ldb = ar[1] + c.pa, br[1] + c.pb
    d["lda"], d["ldb"] = lda, ldb
    d["Abuf"], d["A"] = operand(A, lda, c.off)
    d["Bbuf"], d["B"] = operand(B, ldb, c.off)
    d["bias"] = None if bias is None else torch.from_numpy(bias).to(DEV)
    d["mask"] = None
    if mask is not None:
        d["mbuf"], d["mask"] = operand(mask, c.N + 3, 0)
    d["C0"] = None if C0 is None else torch.from_numpy(C0).to(DEV)
    d["cs0"] = None if cs0 is None else torch.from_numpy(cs0).to(DEV)
    return d


def run_gemm(ops, ws, case, kind, precs):
    c, d = case, gemm_problem(case, kind)
    leaf = R.route(c.ta, c.tb, c.M, c.N, c.K, d["lda"], d["ldb"], c.off == 0, "b" in c.epi, "r" in c.epi, "m" in c.epi,
                   "+" in c.epi, WS_BYTES[c.ws])
    assert leaf == c.leaf
    worst = 0.0
    for prec in precs:
        what = "%s %s %s" % (c.name, kind, prec)
        ops.set_matmul_precision(prec)
        fr = Frame(c.M, c.N, NAN if d["C0"] is None else d["C0"])
        cs = None
        if d["cs0"] is not None:
            cs = Frame(1, c.M, d["cs0"])
        wp, wb = arm(ws, WS_BYTES[c.ws])
        ops.call("sbl_gemm_f32", c.ta, c.tb, c.M, c.N, c.K, P(d["A"]), d["lda"], P(d["B"]), d["ldb"], fr.ptr(), fr.ld,
                 P(d["bias"]), int("r" in c.epi), P(d["mask"]), c.N + 3 if d["mask"] is not None else 0, int("+" in c.epi),
                 None if cs is None else cs.ptr(), wp, wb, S())
        assert kid() == R.KERNEL_ID[leaf.family], "%s: ran kernel family %d, route() says %s" % (what, kid(), leaf.family)
        counters_zero(ws, what)
        fr.check_frame(what)
        cextra = R.extra_roundings(leaf, "b" in c.epi, "+" in c.epi, prec)
        bound = None if kind == "int" else (c.K + cextra) * U * d["mag"] + R.dropped(leaf, prec) * d["prod_mag"]
        worst = max(worst, check(what, fr.out(), d["ref"], bound))
        if cs is not None:
            cs.check_frame(what + " a_colsum")
            cb = None if kind == "int" else (c.K + leaf.splits + 1) * U * d["cs_mag"]
            worst = max(worst, check(what + " a_colsum", cs.out()[0], d["cs_ref"], cb))
    return worst


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_gemm_exact(ops, wsbuf, case):
    """Integer data, all four precisions: C and a_colsum EQUAL the integer result on every leaf; kernel family, guard
    frame and re-armed counters checked after every launch."""
    run_gemm(ops, wsbuf, case, "int", PRECS)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_gemm_rounded(ops, wsbuf, case):
    """Uniform data under f32 and bf16x6 against float64 within the derived bound of the module docstring.
    measured (worst err / bound over all cases): C 0.43 under f32 and 0.30 under bf16x6, both at 100x72x4 + bias on the (1, 1)
    layout (the shortest K: the bound has the least slack there); a_colsum 0.11."""
    run_gemm(ops, wsbuf, case, "uni", ROUNDED_PRECS)


# --------------------------------------------------------------------------- sbl_gemm2_f32
@functools.lru_cache(maxsize=2)
def gemm2_problem(case, kind):
    c = case
    d = {"lda": c.K + c.pa, "ldb": c.K + c.pb, "A": [], "B": [], "bias": [], "ref": [], "mag": [], "prod_mag": [], "keep": []}
    for t in (0, 1):
        A, B = fill(kind, "g2.A%d." % t + c.name, (c.M, c.K)), fill(kind, "g2.B%d." % t + c.name, (c.N, c.K))
        bias = fill(kind, "g2.b%d." % t + c.name, (c.N,)) if c.bias else None
        ref, mag = f64(A) @ f64(B).T, np.abs(f64(A)) @ np.abs(f64(B)).T
        d["prod_mag"].append(torch.from_numpy(mag).to(DEV))
        if bias is not None:
            ref, mag = ref + f64(bias), mag + np.abs(f64(bias))
        if c.relu:
            ref = np.maximum(ref, 0.0)
        ab, av = operand(A, d["lda"], c.off)
        bb, bv = operand(B, d["ldb"], c.off)
        d["keep"] += [ab, bb]
        d["A"].append(av)
        d["B"].append(bv)
        d["bias"].append(None if bias is None else torch.from_numpy(bias).to(DEV))
        d["ref"].append(torch.from_numpy(ref).to(DEV))
        d["mag"].append(torch.from_numpy(mag).to(DEV))
    return d


def run_gemm2(ops, ws, case, kind, precs):
    c, d = case, gemm2_problem(case, kind)
    leaf = R.route_gemm2(c.M, c.N, c.K, d["lda"], d["ldb"], c.off == 0, c.bias, c.relu, WS_BYTES[c.ws])
    assert leaf == c.leaf
    worst = 0.0
    for prec in precs:
        what = "%s %s %s" % (c.name, kind, prec)
        ops.set_matmul_precision(prec)
        fr = [Frame(c.M, c.N, NAN) for _ in (0, 1)]
        wp, wb = arm(ws, WS_BYTES[c.ws])
        ops.call("sbl_gemm2_f32", c.M, c.N, c.K, P(d["A"][0]), P(d["A"][1]), d["lda"], P(d["B"][0]), P(d["B"][1]), d["ldb"],
                 fr[0].ptr(), fr[1].ptr(), fr[0].ld, P(d["bias"][0]), P(d["bias"][1]), int(c.relu), wp, wb, S())
        assert kid() == R.KERNEL_ID[leaf.family], "%s: ran kernel family %d, route() says %s" % (what, kid(), leaf.family)
        counters_zero(ws, what)
        cextra = R.extra_roundings(leaf, c.bias, False, prec)
        for t in (0, 1):
            fr[t].check_frame(what)
            bound = None if kind == "int" else (c.K + cextra) * U * d["mag"][t] + R.dropped(leaf, prec) * d["prod_mag"][t]
            worst = max(worst, check("%s [%d]" % (what, t), fr[t].out(), d["ref"][t], bound))
    return worst


@pytest.mark.parametrize("case", R.GEMM2_CASES, ids=lambda c: c.name)
def test_gemm2_exact(ops, wsbuf, case):
    """Both problems of sbl_gemm2_f32 equal their integer results in all four precisions: dual skinny, dual tiled with
    and without the split, no / short workspace (splits = 1), and the two-launch fallbacks."""
    run_gemm2(ops, wsbuf, case, "int", PRECS)


@pytest.mark.parametrize("case", R.GEMM2_CASES, ids=lambda c: c.name)
def test_gemm2_rounded(ops, wsbuf, case):
    """Uniform data under f32 and bf16x6 within the derived bound.
    measured: 0.12 under f32, 0.10 under bf16x6 (1024x8192x40, the two-launch fallback)."""
    run_gemm2(ops, wsbuf, case, "uni", ROUNDED_PRECS)


# --------------------------------------------------------------------------- sbl_wgrad_seg_f32
# (name, M, N, segment rows, lda - M, colsum?)  -> loaders / tiles as gemm.hip chooses them:
SEG_CASES = [
    ("unaligned_nosplit", 101, 70, (5, 37), 3, True),              # SegMC<64, false>; 42 rows < 128: one slice
    ("unaligned_1seg", 101, 70, (300,), 3, True),                  # one segment, 2 slices
    ("unaligned_3split", 100, 72, (130, 77, 200), 0, False),       # 407 rows: 3 slices, segment edges inside a 16-deep step
    ("aligned64", 100, 72, (16, 48, 64, 144), 4, True),            # SegMC<64, true>, 2 slices
    ("aligned64_16seg", 60, 132, (16,) * 16, 0, True),             # 16 segments of one step each
    ("aligned64_1col", 132, 60, (32, 96), 0, True),                # one column tile: a_colsum must come from the y == 0 tiles
    ("aligned128", 2048, 512, (128, 128), 0, True),                # 64 128x128 tiles >= 48: SegMC<128, true>, 2 slices
]


def seg_splits(M, N, rows):
    """gemm.hip sbl_wgrad_seg_f32: tile, splits (seg_target = 768, chunks >= 128 rows)."""
    K = sum(rows)
    aligned = all(r % 16 == 0 for r in rows)
    T = 128 if aligned and R.cdiv(M, 128) * R.cdiv(N, 128) >= 48 else 64
    tiles = R.cdiv(M, T) * R.cdiv(N, T)
    return max(1, min(R.cdiv(768, tiles), K // 128))


@functools.lru_cache(maxsize=2)
def seg_problem(name, M, N, rows, pa, colsum, kind):
    lda, ldb = M + pa + (-(M + pa)) % 4, N + (-N) % 4
    A = [fill(kind, "sg.A%d.%s" % (i, name), (r, M)) for i, r in enumerate(rows)]
    B = [fill(kind, "sg.B%d.%s" % (i, name), (r, N)) for i, r in enumerate(rows)]
    C0 = fill(kind, "sg.C." + name, (M, N))
    cs0 = fill(kind, "sg.s." + name, (M,)) if colsum else None
    Ac, Bc = f64(np.concatenate(A)), f64(np.concatenate(B))
    d = {"lda": lda, "ldb": ldb, "C0": torch.from_numpy(C0).to(DEV),
         "ref": torch.from_numpy(f64(C0) + Ac.T @ Bc).to(DEV), "mag": torch.from_numpy(np.abs(f64(C0)) + np.abs(Ac).T @ np.abs(Bc)).to(DEV),
         "prod_mag": torch.from_numpy(np.abs(Ac).T @ np.abs(Bc)).to(DEV)}
    d["A"] = [operand(a, lda, 0) for a in A]
    d["B"] = [operand(b, ldb, 0) for b in B]
    d["cs0"] = None
    if colsum:
        d["cs0"] = torch.from_numpy(cs0).to(DEV)
        d["cs_ref"] = torch.from_numpy(f64(cs0) + Ac.sum(0)).to(DEV)
        d["cs_mag"] = torch.from_numpy(np.abs(f64(cs0)) + np.abs(Ac).sum(0)).to(DEV)
    return d


def run_seg(ops, name, M, N, rows, pa, colsum, kind, precs):
    d = seg_problem(name, M, N, rows, pa, colsum, kind)
    K, n, splits = sum(rows), len(rows), seg_splits(M, N, rows)
    worst = 0.0
    for prec in precs:
        what = "wgrad_seg %s %s %s" % (name, kind, prec)
        ops.set_matmul_precision(prec)
        fr = Frame(M, N, d["C0"])
        cs = Frame(1, M, d["cs0"]) if colsum else None
        ops.call("sbl_wgrad_seg_f32", n, (ctypes.c_void_p * n)(*[v.data_ptr() for _, v in d["A"]]), d["lda"],
                 (ctypes.c_void_p * n)(*[v.data_ptr() for _, v in d["B"]]), d["ldb"], (ctypes.c_int * n)(*rows), M, N,
                 fr.ptr(), fr.ld, None if cs is None else cs.ptr(), S())
        assert kid() == R.KID_SEG_WGRAD, what
        fr.check_frame(what)
        # every slice adds its partial with one float atomic onto C: splits additions beyond the K chain
        bound = None if kind == "int" else (K + splits) * U * d["mag"] + (R.DROPPED6 if prec == "bf16x6" else 0.0) * d["prod_mag"]
        worst = max(worst, check(what, fr.out(), d["ref"], bound))
        if cs is not None:
            cs.check_frame(what + " a_colsum")
            worst = max(worst, check(what + " a_colsum", cs.out()[0], d["cs_ref"], None if kind == "int" else (K + splits + 1) * U * d["cs_mag"]))
    return worst


@pytest.mark.parametrize("name,M,N,rows,pa,colsum", SEG_CASES, ids=[c[0] for c in SEG_CASES])
def test_wgrad_seg_exact(ops, name, M, N, rows, pa, colsum):
    """C += sum_s A_s^T B_s and a_colsum += column sums, integer data, all four precisions: equal to the integer result
    for unaligned segments, aligned 64x64 and 128x128 tiles, 1 and 16 segments, one and several K slices, lda > M,
    a_colsum NULL."""
    run_seg(ops, name, M, N, rows, pa, colsum, "int", PRECS)


@pytest.mark.parametrize("name,M,N,rows,pa,colsum", SEG_CASES, ids=[c[0] for c in SEG_CASES])
def test_wgrad_seg_rounded(ops, name, M, N, rows, pa, colsum):
    """Uniform data under f32 and bf16x6: (K + splits) * U * (|A|^T |B| + |C0|) (+ 2^-26 |A|^T |B|).
    measured: C 0.08 under f32, 0.06 under bf16x6 (42 rows, one slice); a_colsum 0.02."""
    run_seg(ops, name, M, N, rows, pa, colsum, "uni", ROUNDED_PRECS)


# --------------------------------------------------------------------------- sbl_wgrad_group_f32
GROUP_SHAPES = [(4, 4), (60, 132), (512, 2048), (128, 128), (132, 60), (64, 260), (4, 132), (256, 4)]
GROUP_CASES = [(1, 1), (8, 1), (9, 3), (17, 1), (17, 3), (1, 3)]      # (nprob, nseg): 8 | 9 | 17 cross SBL_GROUP_WRITE = 8
GROUP_ROWS = {1: (48,), 3: (16, 32, 16)}


def group_shapes(nprob):
    """The big problem once (first for nprob == 1 ... so that a single problem is not trivial), small ones around it."""
    out = []
    for p in range(nprob):
        s = GROUP_SHAPES[p % len(GROUP_SHAPES)]
        out.append((60, 132) if s == (512, 2048) and p >= len(GROUP_SHAPES) else s)
    if nprob == 1:
        out = [(60, 132)]
    return out


@functools.lru_cache(maxsize=2)
def group_problem(nprob, nseg, kind):
    rows = GROUP_ROWS[nseg]
    probs = []
    for p, (M, N) in enumerate(group_shapes(nprob)):
        tag = "%d.%d.%d" % (nprob, nseg, p)
        lda, ldb = M + (4 if p % 3 == 1 else 0), N + (8 if p % 3 == 2 else 0)
        A = [fill(kind, "gp.A%d.%s" % (s, tag), (r, M)) for s, r in enumerate(rows)]
        B = [fill(kind, "gp.B%d.%s" % (s, tag), (r, N)) for s, r in enumerate(rows)]
        C0 = fill(kind, "gp.C." + tag, (M, N))
        has_cs = p % 4 != 3                                 # every fourth problem: colsum NULL
        cs0 = fill(kind, "gp.s." + tag, (M,)) if has_cs else None
        Ac, Bc = f64(np.concatenate(A)), f64(np.concatenate(B))
        q = {"M": M, "N": N, "lda": lda, "ldb": ldb, "C0": torch.from_numpy(C0).to(DEV),
             "A": [operand(a, lda, 0) for a in A], "B": [operand(b, ldb, 0) for b in B],
             "ref": torch.from_numpy(f64(C0) + Ac.T @ Bc).to(DEV),
             "mag": torch.from_numpy(np.abs(f64(C0)) + np.abs(Ac).T @ np.abs(Bc)).to(DEV),
             "prod_mag": torch.from_numpy(np.abs(Ac).T @ np.abs(Bc)).to(DEV), "cs0": None}
        if has_cs:
            q["cs0"] = torch.from_numpy(cs0).to(DEV)
            q["cs_ref"] = torch.from_numpy(f64(cs0) + Ac.sum(0)).to(DEV)
            q["cs_mag"] = torch.from_numpy(np.abs(f64(cs0)) + np.abs(Ac).sum(0)).to(DEV)
        probs.append(q)
    return probs


def launch_group(ops, probs, rows, table):
    """One sbl_wgrad_group_f32 call on fresh frames; returns (C frames, colsum frames)."""
    n, k = len(probs), len(rows)
    fr = [Frame(q["M"], q["N"], q["C0"]) for q in probs]
    cs = [Frame(1, q["M"], q["cs0"]) if q["cs0"] is not None else None for q in probs]
    arr = lambda ct, vals: (ct * len(vals))(*vals)      # noqa: E731
    ops.call("sbl_wgrad_group_f32", n, k, arr(ctypes.c_int, list(rows)),
             arr(ctypes.c_void_p, [v.data_ptr() for q in probs for _, v in q["A"]]), arr(ctypes.c_long, [q["lda"] for q in probs]),
             arr(ctypes.c_void_p, [v.data_ptr() for q in probs for _, v in q["B"]]), arr(ctypes.c_long, [q["ldb"] for q in probs]),
             arr(ctypes.c_int, [q["M"] for q in probs]), arr(ctypes.c_int, [q["N"] for q in probs]),
             arr(ctypes.c_void_p, [f.ptr() for f in fr]), arr(ctypes.c_long, [f.ld for f in fr]),
             arr(ctypes.c_void_p, [None if c is None else c.ptr() for c in cs]), table.data_ptr(), table.numel(), S())
    assert kid() == R.KID_SEG_WGRAD
    return fr, cs


def run_group(ops, nprob, nseg, kind, precs):
    from sbl_for_multilingual_lip_reading_amd import _lib
    probs, rows = group_problem(nprob, nseg, kind), GROUP_ROWS[nseg]
    K = sum(rows)
    table = torch.empty(_lib.load().sbl_wgrad_group_table_bytes(nprob), dtype=torch.uint8, device=DEV)
    worst = 0.0
    for prec in precs:
        ops.set_matmul_precision(prec)
        fr, cs = launch_group(ops, probs, rows, table)
        fr2, cs2 = launch_group(ops, probs, rows, table)      # no atomics on C: a second run is bit-equal
        for p, q in enumerate(probs):
            what = "wgrad_group n%d s%d %s %s [%d: %dx%d]" % (nprob, nseg, kind, prec, p, q["M"], q["N"])
            fr[p].check_frame(what)
            assert torch.equal(fr[p].buf, fr2[p].buf), what + ": second run differs"
            # one workgroup per tile over the whole K, C += acc: one addition beyond the K chain
            bound = None if kind == "int" else (K + 1) * U * q["mag"] + (R.DROPPED6 if prec == "bf16x6" else 0.0) * q["prod_mag"]
            worst = max(worst, check(what, fr[p].out(), q["ref"], bound))
            if cs[p] is not None:
                cs[p].check_frame(what + " colsum")
                worst = max(worst, check(what + " colsum", cs[p].out()[0], q["cs_ref"], None if kind == "int" else (K + 2) * U * q["cs_mag"]))
    return worst


@pytest.mark.parametrize("nprob,nseg", GROUP_CASES)
def test_wgrad_group_exact(ops, nprob, nseg):
    """All problems of one grouped launch equal their integer results in all four precisions, for problem counts on both
    sides of the descriptor-write batch (1, 8, 9, 17), one and three segments, mixed shapes from 4x4 to 512x2048, some
    colsum NULL; nprob = 1 goes to the ABI directly (ops.wgrad_group would reroute it).  A second run is bit-equal."""
    run_group(ops, nprob, nseg, "int", PRECS)


@pytest.mark.parametrize("nprob,nseg", GROUP_CASES)
def test_wgrad_group_rounded(ops, nprob, nseg):
    """Uniform data under f32 and bf16x6: (K + 1) * U * (|A|^T |B| + |C0|) (+ 2^-26 |A|^T |B|); colsum (K + 2) * U * ...
    measured: C 0.10 under f32, 0.07 under bf16x6 (nprob = 17); colsum 0.02."""
    run_group(ops, nprob, nseg, "uni", ROUNDED_PRECS)


# --------------------------------------------------------------------------- sbl_colsum_f32
@pytest.mark.parametrize("M", [1, 63, 65, 4097])
@pytest.mark.parametrize("N", [1, 64, 65])
def test_colsum(ops, M, N):
    """out[n] (+)= sum_m X[m, n] with ldx = N + 3 (NaN padding), overwrite and +=: exact on integers; on uniform data
    within depth * U * (sum_m |X| + |out0|), depth = the longest chain of additions a term goes through: cdiv(rpb, 4)
    in its thread, 3 across the row groups in LDS, one atomic per row block (gy <= 64; M = 4097 gives gy = 64 and a
    ragged rows_per_block = 65), one for the previous value, + 1 for the second-order terms.
    measured: 0.03 (65 x 64, +=)."""
    ops.set_matmul_precision("f32")
    gy = min(R.cdiv(M, 64), 64)
    depth = R.cdiv(R.cdiv(M, gy), 4) + 3 + gy + 1 + 1
    for kind in ("int", "uni"):
        X, o0 = fill(kind, "cs.X", (M, N)), fill(kind, "cs.o", (N,))
        xb, xv = operand(X, N + 3, 0)
        for acc in (0, 1):
            what = "colsum %dx%d %s acc%d" % (M, N, kind, acc)
            out = Frame(1, N, torch.from_numpy(o0).to(DEV) if acc else NAN)
            ops.call("sbl_colsum_f32", xv.data_ptr(), N + 3, out.ptr(), M, N, acc, S())
            out.check_frame(what)
            ref = f64(X).sum(0) + (f64(o0) if acc else 0.0)
            mag = np.abs(f64(X)).sum(0) + (np.abs(f64(o0)) if acc else 0.0)
            check(what, out.out()[0], torch.from_numpy(ref).to(DEV), None if kind == "int" else torch.from_numpy(depth * U * mag).to(DEV))
