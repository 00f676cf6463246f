"""The trunk convolutions, leaf by leaf of their host dispatch: sbl_conv2d_fwd, sbl_conv2d_dgrad, sbl_conv2d_dgrad_bnstats,
sbl_conv2d_dgrad_fused, sbl_conv1x1s2_dgrad_compact, sbl_conv2d_wgrad, sbl_conv_weight_pack and sbl_conv_wgrad_unpack through
the C ABI, on tensors and a workspace this module allocates, every case of tests/conv_routes.py under all four precisions.

Every launch is checked for its route, its frame and its values:
  * route: sbl_profile_last_route() is the leaf tests/conv_routes.py predicts for (case, precision) - family, tile and, for
    the patch-resident kernels, (TR, G) - sbl_profile_last_kernel() is 4 / 5 / 6, and the sbl_profile_used() delta is the
    leaf's launch count (2 for the tail split).  A case that lands elsewhere FAILS.  (The library does not report the class
    count or the K splits of a leaf: those fields are held to the hand-written table on the CPU and enter here through c of
    the rounded bound only);
  * frame: y, dx, compact dx, dw, stats and sums live between guard blocks of a sentinel that must survive bit for bit;
    x, dy, the packed weights, the addend and the BatchNorm operands sit between NaN guard blocks, so a read beyond an
    operand poisons the output; the workspace is handed over with zero counters and NaN slabs and the 4096 counters must be
    zero again after every launch; outputs are NaN-prefilled, so an element the launch never writes fails the value check
    (the non-compact 1x1 / stride-2 gradient must leave every odd pixel exactly zero: the reference holds zeros there);
  * value, EXACT in all four precisions on integer data: x, w, dy, addend in [-hi, hi] (hi = 3, narrowed per case by
    data_range() until the condition below holds), pre in [-2, 2], mean in [-1, 1], invstd in {0.5, 1, 2}, act = relu(xhat):
    one bf16 plane holds every operand and every fp32 partial sum is an integer below 2^24, so y, dx, dw equal the integer
    convolution (torch conv2d / conv2d_input / conv2d_weight in float64 on the CPU) and stats / sums equal the integer sums,
    whatever the route, split count or precision.  The condition is asserted per case before any launch: the sum of
    magnitudes of every output element is below 2^24, and R * max |term| < 2^24 for every statistics term (v, v^2, g,
    g * xhat, g * xhat2), R = the rows one fp32 partial can cover: 256 for the tile engine (a wave's column partial spans at
    most 128 rows), 256 * tiles per persistent workgroup for the patch-resident kernel;
  * value, EXACT on integers that need two and three bf16 planes (wide_ints(): a few odd 9-bit and 17-bit values among
    {-1, 0, 1}, placed so that no product passes 2^18 and every sum of magnitudes stays below 2^23): f32 and bf16x6 must give
    the integer convolution, bf16x3 and bf16 the value tests/bf16_model.py defines for the mode - a dropped, doubled or
    mis-paired plane moves an output by at least 1, which the rounded bound below (loose at K = 576) would let through;
  * value, ROUNDED on detfill.uniform data: under f32 and bf16x6 against float64, under bf16x3 and bf16 against
    tests/bf16_model.py (the mode's plane products summed in float64), elementwise
        |out - ref| <= (K + c) * U * conv(|a|, |b|)  (+ |addend| + |previous| inside the magnitude)
                       + 2^-26 * conv(|a|, |b|) under bf16x6,
    U = 2^-24.  K is the contraction length of THAT output element: channels times the taps that are in bounds for it
    (border pixels, parity classes and the position-major kernels contract over fewer taps), for a weight gradient the
    pixels its tap can reach times the images.  c = conv_routes.extra_roundings(): slab additions of the tail split or float
    atomics of the other weight-gradient workgroups (splits - 1), the atomic onto dw (1), the addend (1), previous dw (1).
    Why it is a bound: an output is a sum of K products (+ addend + previous) in some order; each product enters through one
    fused multiply-add and each further addition rounds once, so a term passes through at most K + c roundings of relative
    size U applied to partial sums no larger than the sum of magnitudes.  Under the split-bf16 modes a product is up to six
    exact plane products accumulated by v_mfma_f32_32x32x16_bf16 sixteen k at a time; the bound keeps one rounding per fp32
    product plus the dropped planes of mode 6, as include/sbl_hip.h states the modes.
    Statistics are compared with float64 sums over the kernel's OWN stored output (the convolution's error does not enter):
        |stat - sum| <= D * U * sum |term|,
    D = the fp32 partial depth read from the epilogues + the roundings of the term itself: tile engine (mfma_gemm.h
    EpiStore::tile + sbl_tile_finish) 16 rows per 32-row block and lane x BM / 64 blocks + 1 cross-half shuffle; patch-resident
    kernel (conv_patch.h) 16 pixels per thread and tile x tiles per workgroup + 16 pixel groups met in LDS; the double atomics
    that follow do not round at this scale.  The term adds 1 rounding (v * v, g * xhat) and xhat = (x - mean) * invstd two
    more.  stat_depth() is that count.

check() prints the worst err / bound ratio of every comparison; the worst one measured on an MI355X is in each test's
docstring.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_model
import conv_routes as R
from sbl_for_multilingual_lip_reading_amd import detfill

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = R.U
SENT = -777.25                       # guard value (not an integer: never a legal exact result)
NAN = float("nan")
GUARD = 4096                         # elements of a guard block (a multiple of 4: operands stay 16-byte aligned)
LIMIT = float(1 << 24)


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


def lib():
    from sbl_for_multilingual_lip_reading_amd import _lib
    return _lib.load()


def ints(name, shape, hi):
    return np.rint(detfill.uniform(name, shape) * np.float32(hi)).astype(np.float32)


def wide_ints(name, shape, axis, role, K):
    """Integers that need two and three bf16 planes, placed so that every product and every sum stays exact in fp32:
    mostly {-1, 0, 1}; where index % 4 along `axis` (the contraction's channel / image index) is 2 or 3, a fraction
    min(1/8, K^-1/2) of odd 9-bit values +-[257, 511] (two planes); where it is `role` (0 for the first operand, 1 for the
    second), a fraction min(1/16, 4/K) of odd 17-bit values +-[65537, 131071] (three planes).  The two operands therefore
    never meet wide x 17-bit (2^26+), 9-bit x 9-bit products (< 2^18) meet about once per output and 17-bit x narrow ones about
    four times: sums of magnitudes stay far below 2^24 (asserted in problem())."""
    base = ints(name, shape, 1)
    u = detfill.uniform(name + ".sel", shape)      # |u| below the fraction selects, |u| / fraction is the value, sign(u) the sign
    sign, mag = np.where(u < 0, np.float32(-1), np.float32(1)), np.abs(u)
    idx = np.arange(shape[axis]) % 4
    sel = idx.reshape([-1 if i == axis else 1 for i in range(len(shape))])
    p2, p3 = np.float32(min(1.0 / 8, K ** -0.5)), np.float32(min(1.0 / 16, 4.0 / K))
    two, three = (sel >= 2) & (mag < p2), (sel == role) & (mag < p3)
    out = np.where(two, sign * (257 + 2 * np.floor(mag / p2 * 127)), base)
    out = np.where(three, sign * (65537 + 2 * np.floor(mag / p3 * 32767)), out)
    return out.astype(np.float32)


class Framed:
    """`shape` elements between two guard blocks.  Outputs: sentinel guards (must survive); operands: NaN guards."""

    def __init__(self, shape, init, guard=SENT, dtype=torch.float32):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), guard, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if isinstance(init, np.ndarray):
            init = torch.from_numpy(np.ascontiguousarray(init))
        if isinstance(init, torch.Tensor):
            self.t.copy_(init.to(dtype))
        else:
            self.t.fill_(init)

    def ptr(self):
        return self.t.data_ptr()

    def check_frame(self, what):
        assert bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[-GUARD:] == SENT).all()), what + ": a guard block was written"


def operand(a):
    return Framed(tuple(a.shape), a, guard=NAN)


def P(f):
    return None if f is None else f.ptr()


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
    bound = bound.expand_as(err)
    ratio = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                        torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    worst = float(ratio.max())
    print("%-72s worst err/bound %.3f  (max err %.3e)" % (what, worst, float(err.max())))
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


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def dev64(t):
    return t.to(torch.float64).to(DEV)


# --------------------------------------------------------------------------- the operation of a case, on the CPU
def geometry(c):
    pad = 1 if c.k == 3 else 0
    return pad, R.out_dim(c.H, c.k, c.stride, pad), R.out_dim(c.W, c.k, c.stride, pad)


def bilinear_fn(c):
    """fn(a, b) of the case: forward (x, w) -> y, input gradient (dy, w) -> dx, weight gradient (x, dy) -> dw; NCHW / OIHW."""
    pad, Ho, Wo = geometry(c)
    if c.op == "fwd":
        return lambda a, b: F.conv2d(a, b, None, c.stride, pad)
    if c.op == "dgrad":
        return lambda a, b: torch.nn.grad.conv2d_input((a.shape[0], b.shape[1], c.H, c.W), b, a, c.stride, pad)
    return lambda a, b: torch.nn.grad.conv2d_weight(a, (b.shape[1], a.shape[1], c.k, c.k), b, c.stride, pad)


def contraction_length(c):
    """K of every output element: the products that really enter it (one-channel convolution of ones, times the channels)."""
    pad, Ho, Wo = geometry(c)
    one = torch.ones
    if c.op == "fwd":
        return F.conv2d(one(1, 1, c.H, c.W, dtype=torch.float64), one(1, 1, c.k, c.k, dtype=torch.float64), None, c.stride, pad) * c.Cin
    if c.op == "dgrad":
        return torch.nn.grad.conv2d_input((1, 1, c.H, c.W), one(1, 1, c.k, c.k, dtype=torch.float64),
                                          one(1, 1, Ho, Wo, dtype=torch.float64), c.stride, pad) * c.Cout
    return torch.nn.grad.conv2d_weight(one(1, 1, c.H, c.W, dtype=torch.float64), (1, 1, c.k, c.k),
                                       one(1, 1, Ho, Wo, dtype=torch.float64), c.stride, pad) * c.NIMG


def rows_per_partial(c):
    """R of the exactness condition: the rows one fp32 statistics partial can cover, over the four precisions."""
    rows = 256
    for prec in R.PRECS:
        leaf = c.leaf[prec]
        if leaf.family == "patch":
            ntiles, gx = R.patch_grid(c.NIMG, c.H, c.Cin if c.op == "dgrad" else c.Cout, leaf.tr, leaf.g)
            rows = max(rows, 256 * R.cdiv(ntiles, gx))
    return rows


VAR = {3: 19.0 / 6.0, 2: 1.5, 1: 0.5}      # variance of rint(u * hi), u uniform in [-1, 1)


def data_range(c):
    """hi of the integer data: 3, narrowed to 2 or 1 for the cases with statistics until the largest term is safely small:
    with sigma^2 = K * var^2 the variance of an output and 6 sigma its largest value, R * (6 sigma)^2 < 2^24 for the forward's
    v^2 and R * 6 * (6 sigma + hi) < 2^24 for the input gradient's g * xhat (|xhat| <= (2 + 1) * 2).  A rule on the shape alone;
    the real condition is asserted on the reference in problem()."""
    if c.op == "wgrad" or c.epi in ("", "a", "c"):
        return 3
    K, rows = c.k * c.k * (c.Cin if c.op == "fwd" else c.Cout), rows_per_partial(c)
    for hi in (3, 2, 1):
        top = 6.0 * (K * VAR[hi] ** 2) ** 0.5
        if (rows * top * top if c.op == "fwd" else rows * 6.0 * (top + hi)) < LIMIT:
            return hi
    return 1


def stat_depth(c, leaf, xhat):
    """D of the statistics bound (module docstring)."""
    if leaf.family == "patch":
        ntiles, gx = R.patch_grid(c.NIMG, c.H, c.Cin if c.op == "dgrad" else c.Cout, leaf.tr, leaf.g)
        d = 16 * R.cdiv(ntiles, gx) + 16
    else:
        d = 16 * (leaf.tile[0] // 64) + 1
    return d + 1 + (2 if xhat else 0)


def problem(c, kind):
    """Device operands, float64 reference and bound magnitudes of one (case, data kind); run_case builds it once and hands
    it to the four precisions."""
    pad, Ho, Wo = geometry(c)
    hi = data_range(c) if kind == "int" else 1 if kind == "planes" else 0
    tag = c.name + "."

    def fill(name, shape, h=None):
        return torch.from_numpy(detfill.uniform(tag + name, shape) if kind == "uni" else ints(tag + name, shape, h or hi))

    def fill2(name, shape, axis, role):      # the two operands of the contraction
        if kind != "planes":
            return fill(name, shape)
        Kmax = c.NIMG * Ho * Wo if c.op == "wgrad" else c.k * c.k * (c.Cin if c.op == "fwd" else c.Cout)
        return torch.from_numpy(wide_ints(tag + name, shape, axis, role, Kmax))
    d = {"hi": hi, "extra": {}}
    # axis: the dimension of each operand that indexes the contraction (channels; images for a weight gradient)
    if c.op == "fwd":
        a, b = fill2("x", (c.NIMG, c.Cin, c.H, c.W), 1, 0), fill2("w", (c.Cout, c.Cin, c.k, c.k), 1, 1)
    elif c.op == "dgrad":
        a, b = fill2("dy", (c.NIMG, c.Cout, Ho, Wo), 1, 0), fill2("w", (c.Cout, c.Cin, c.k, c.k), 0, 1)
    else:
        a, b = fill2("x", (c.NIMG, c.Cin, c.H, c.W), 0, 0), fill2("dy", (c.NIMG, c.Cout, Ho, Wo), 0, 1)
    w = b
    fn = bilinear_fn(c)
    d["a"], d["b"], d["fn"] = a, b, fn
    ref = fn(a.double(), b.double())
    mag = prod_mag = fn(a.double().abs(), b.double().abs())
    d["K"] = contraction_length(c)
    if c.op == "wgrad":
        to_dev = lambda t: dev64(t.permute(0, 2, 3, 1).contiguous())      # noqa: E731  OIHW -> OHWI
        d["x"], d["dy"] = operand(nhwc(a)), operand(nhwc(b))
        d["prev"] = None
        if c.epi == "+":
            prev = fill("prev", (c.Cout, c.k, c.k, c.Cin))
            d["prev"] = prev.to(DEV)
            ref, mag = ref + prev.permute(0, 3, 1, 2).double(), mag + prev.permute(0, 3, 1, 2).double().abs()
        d["unpack_prev"] = fill("uprev", (c.Cout, c.Cin, c.k, c.k)).to(DEV)
    else:
        to_dev = lambda t: dev64(nhwc(t))      # noqa: E731
        d["src"] = operand(nhwc(a))
        # the library packs the weights: OIHW -> OHWI and the input-gradient image, plus a zeroed double block
        wd = operand(w)
        d["w_ohwi"] = Framed((c.Cout, c.k, c.k, c.Cin), NAN)
        d["w_dg"] = Framed((c.Cin, c.k, c.k, c.Cout), NAN)
        zero = Framed((37,), NAN, dtype=torch.float64)
        from sbl_for_multilingual_lip_reading_amd import ops as _ops
        _ops.call("sbl_conv_weight_pack", wd.ptr(), d["w_ohwi"].ptr(), d["w_dg"].ptr(), c.Cout, c.Cin, c.k, c.k, zero.ptr(), 31, S())
        assert torch.equal(d["w_ohwi"].t, w.permute(0, 2, 3, 1).to(DEV)) and torch.equal(d["w_dg"].t, w.permute(1, 2, 3, 0).to(DEV))
        zero.check_frame(c.name + " weight_pack zero block")
        assert bool((zero.t[:31] == 0).all()) and bool(torch.isnan(zero.t[31:]).all()), c.name + ": weight_pack zeroed other than nzero doubles"
        for f in (d["w_ohwi"], d["w_dg"]):      # the packed weights are operands from here on: NaN guards
            f.check_frame(c.name + " weight_pack")
            f.buf[:GUARD] = NAN
            f.buf[-GUARD:] = NAN
    if c.op == "dgrad" and "a" in c.epi:
        if c.stride == 2:
            add = fill("add", (c.NIMG, c.Cin, (c.H + 1) // 2, (c.W + 1) // 2))
            full = torch.zeros(c.NIMG, c.Cin, c.H, c.W, dtype=torch.float64)
            full[:, :, ::2, ::2] = add.double()
        else:
            add = fill("add", (c.NIMG, c.Cin, c.H, c.W))
            full = add.double()
        d["addend"] = operand(nhwc(add))
        ref, mag = ref + full, mag + full.abs()
    if c.op == "dgrad" and "s" in c.epi:
        shp = (c.NIMG, c.H, c.W, c.Cin)
        if kind != "uni":
            pre = [torch.from_numpy(ints(tag + "pre%d" % i, shp, 2)) for i in (0, 1)]
            mean = [torch.from_numpy(ints(tag + "mu%d" % i, (c.Cin,), 1)) for i in (0, 1)]
            inv = [torch.from_numpy(np.exp2(ints(tag + "is%d" % i, (c.Cin,), 1)).astype(np.float32)) for i in (0, 1)]
        else:
            pre = [torch.from_numpy(detfill.uniform(tag + "pre%d" % i, shp)) for i in (0, 1)]
            mean = [0.1 * torch.from_numpy(detfill.uniform(tag + "mu%d" % i, (c.Cin,))) for i in (0, 1)]
            inv = [1.0 + 0.2 * torch.from_numpy(detfill.uniform(tag + "is%d" % i, (c.Cin,))) for i in (0, 1)]
        act = ((pre[0] - mean[0]) * inv[0]).clamp_min(0)
        d["act"], d["pre"], d["mean"], d["inv"] = operand(act), [operand(t) for t in pre], [operand(t) for t in mean], [operand(t) for t in inv]
        d["gate"] = (act > 0).to(DEV)
        d["xhat"] = [((pre[i].double() - mean[i].double()) * inv[i].double()).to(DEV) for i in (0, 1)]
    assert float(mag.max()) < LIMIT / (2 if kind == "planes" else 1)      # (planes: |p0| + |p1| + |p2| may exceed |x| a little)
    d["ref"], d["mag"], d["prod_mag"] = to_dev(ref), to_dev(mag), to_dev(prod_mag)
    if c.op == "wgrad":
        d["Kdev"] = dev64(d["K"].permute(0, 2, 3, 1).contiguous())           # (1, k, k, 1)
    else:
        d["Kdev"] = dev64(nhwc(d["K"]))                                      # (1, h, w, 1)
    if kind == "int":      # the exactness condition on the statistics partials
        rows = rows_per_partial(c)
        if c.op == "fwd" and c.epi == "stats":
            assert rows * float(d["ref"].abs().max()) ** 2 < LIMIT, (c.name, hi, rows, float(d["ref"].abs().max()))
        if c.op == "dgrad" and "s" in c.epi:
            g = d["ref"] * d["gate"]
            worst = max(float(g.abs().max()), float((g * d["xhat"][0]).abs().max()), float((g * d["xhat"][1]).abs().max()))
            assert rows * worst < LIMIT, (c.name, hi, rows, worst)
    return d


def reference(d, c, kind, prec):
    """The value a precision is held to: float64 (integer data, f32, bf16x6) or the bf16 model of the mode (bf16x3, bf16)."""
    if kind == "int" or prec in ("f32", "bf16x6"):
        return d["ref"]
    if prec not in d["extra"]:
        r = bf16_model.bilinear(d["fn"], d["a"], d["b"], prec)
        r = dev64(r.permute(0, 2, 3, 1).contiguous())
        if c.op == "wgrad" and d["prev"] is not None:
            r = r + d["prev"].double()
        if c.op == "dgrad" and "a" in c.epi:
            add = d["addend"].t.double()
            if c.stride == 2:
                r[:, ::2, ::2, :] += add
            else:
                r = r + add
        d["extra"][prec] = r
    return d["extra"][prec]


def out_bound(d, c, kind, prec, leaf):
    if kind != "uni":
        return None
    cextra = R.extra_roundings(leaf, addend=c.op == "dgrad" and "a" in c.epi, previous=c.op == "wgrad" and c.epi == "+")
    return (d["Kdev"] + cextra) * U * d["mag"] + (R.DROPPED6 if prec == "bf16x6" else 0.0) * d["prod_mag"]


# --------------------------------------------------------------------------- one launch, route-checked
class Launch:
    """Brackets one entry-point call: profile slots on, route / kernel id / slot delta / counters checked after it."""

    def __init__(self, ops, ws, c, prec, what):
        self.ops, self.ws, self.c, self.prec, self.what = ops, ws, c, prec, what
        self.stamps = torch.zeros(2 * 64, dtype=torch.int64, device=DEV)

    def call(self, leaf, name, *args):
        L = lib()
        assert L.sbl_profile_begin(self.stamps.data_ptr(), 64) == 0
        try:
            self.ops.call(name, *args)
            used = L.sbl_profile_used()
        finally:
            L.sbl_profile_end()
        what = "%s %s" % (self.what, name)
        assert L.sbl_profile_last_kernel() == R.KID[self.c.op], what
        got = L.sbl_profile_last_route()
        assert got == R.route_code(leaf), "%s: ran route 0x%08x (family %d, tile %d, TR %d, G %d), conv_routes says %s" % (
            what, got, got >> 24, (got >> 20) & 15, (got >> 10) & 1023, got & 1023, leaf)
        assert used == leaf.launches, "%s: %d launches, conv_routes says %d" % (what, used, leaf.launches)
        counters_zero(self.ws, what)


def knobs(ops, c):
    ops.call("sbl_set_tuning", 5, c.k5)
    ops.call("sbl_set_tuning", 9, c.k9)


def restore(ops):
    ops.call("sbl_set_tuning", 5, R.KNOB5_DEFAULT)
    ops.call("sbl_set_tuning", 9, R.KNOB9_DEFAULT)


def column_sums(t):
    return t.reshape(-1, t.shape[-1]).sum(0)


def run_fwd(ops, ws, c, kind, prec, d, leaf, what):
    pad, Ho, Wo = geometry(c)
    y = Framed((c.NIMG, Ho, Wo, c.Cout), NAN)
    stats = None
    if c.epi == "stats":      # integer data: stats_zeroed = 0 on a NaN-prefilled buffer; uniform data: the caller's zeros
        stats = Framed((2 * c.Cout,), NAN if kind == "int" else 0.0, dtype=torch.float64)
    wp, wb = arm(ws, R.WS_BYTES[c.ws])
    Launch(ops, ws, c, prec, what).call(leaf, "sbl_conv2d_fwd", d["src"].ptr(), d["w_ohwi"].ptr(), y.ptr(), P(stats), int(kind != "int"),
                                        c.NIMG, c.H, c.W, c.Cin, c.Cout, c.k, c.k, c.stride, pad, wp, wb, S())
    y.check_frame(what + " y")
    worst = check(what + " y", y.t, reference(d, c, kind, prec), out_bound(d, c, kind, prec, leaf))
    if stats is not None:
        stats.check_frame(what + " stats")
        v = y.t.double()
        ref = torch.cat([column_sums(v), column_sums(v * v)])
        bound = None
        if kind != "int":      # (two-plane integers: outputs of millions, their squares are not exact in fp32 - held to the bound)
            depth = stat_depth(c, leaf, False)
            bound = U * torch.cat([(depth - 1) * column_sums(v.abs()), depth * column_sums(v * v)])
        worst = max(worst, check(what + " stats", stats.t, ref, bound))
    return worst


def run_dgrad(ops, ws, c, kind, prec, d, leaf, what):
    pad, Ho, Wo = geometry(c)
    shape = (c.NIMG, c.H, c.W, c.Cin)
    L = Launch(ops, ws, c, prec, what)
    wp, wb = arm(ws, R.WS_BYTES[c.ws])
    geo = (c.NIMG, c.H, c.W, c.Cin, c.Cout, c.k, c.k, c.stride, pad)
    sums = None
    if c.epi == "c":
        dx = Framed((c.NIMG, (c.H + 1) // 2, (c.W + 1) // 2, c.Cin), NAN)
        L.call(leaf, "sbl_conv1x1s2_dgrad_compact", d["src"].ptr(), d["w_dg"].ptr(), dx.ptr(), c.NIMG, c.H, c.W, c.Cin, c.Cout, wp, wb, S())
        dx.check_frame(what + " dx")
        ref, bound = reference(d, c, kind, prec)[:, ::2, ::2, :], out_bound(d, c, kind, prec, leaf)
        return check(what + " compact dx", dx.t, ref, None if bound is None else bound[:, ::2, ::2, :])
    dx = Framed(shape, NAN)
    if c.epi == "":
        L.call(leaf, "sbl_conv2d_dgrad", d["src"].ptr(), d["w_dg"].ptr(), dx.ptr(), *geo, wp, wb, S())
    else:
        two = c.epi.endswith("2")
        if "s" in c.epi:      # integer data: sums_zeroed = 0 on a NaN-prefilled buffer; uniform data: the caller's zeros
            sums = Framed(((4 if two else 2) * c.Cin,), NAN if kind == "int" else 0.0, dtype=torch.float64)
        if c.epi == "s":
            L.call(leaf, "sbl_conv2d_dgrad_bnstats", d["src"].ptr(), d["w_dg"].ptr(), dx.ptr(), *geo, wp, wb, d["act"].ptr(), d["pre"][0].ptr(),
                   d["mean"][0].ptr(), d["inv"][0].ptr(), sums.ptr(), int(kind != "int"), S())
        else:
            bn = [None] * 7      # act, pre, mean, invstd, pre2, mean2, invstd2
            if "s" in c.epi:
                bn[:4] = [d["act"].ptr(), d["pre"][0].ptr(), d["mean"][0].ptr(), d["inv"][0].ptr()]
            if two:
                bn[4:] = [d["pre"][1].ptr(), d["mean"][1].ptr(), d["inv"][1].ptr()]
            L.call(leaf, "sbl_conv2d_dgrad_fused", d["src"].ptr(), d["w_dg"].ptr(), dx.ptr(), *geo, wp, wb, P(d.get("addend")), *bn, P(sums),
                   int(kind != "int"), S())
    dx.check_frame(what + " dx")
    worst = check(what + " dx", dx.t, reference(d, c, kind, prec), out_bound(d, c, kind, prec, leaf))
    if c.epi == "s":
        # the plain entry point on the same operands: the same dx bits (its own route: no sums, so no no128 arm)
        dx0 = Framed(shape, NAN)
        wp, wb = arm(ws, R.WS_BYTES[c.ws])
        leaf0 = R.route_dgrad(prec, c.k5, c.NIMG, c.H, c.W, c.Cin, c.Cout, c.k, c.stride, False, R.WS_BYTES[c.ws])
        L.call(leaf0, "sbl_conv2d_dgrad", d["src"].ptr(), d["w_dg"].ptr(), dx0.ptr(), *geo, wp, wb, S())
        dx0.check_frame(what + " dx (plain)")
        assert torch.equal(dx0.t, dx.t), what + ": sbl_conv2d_dgrad_bnstats and sbl_conv2d_dgrad differ in dx"
    if sums is not None:
        sums.check_frame(what + " sums")
        g = dx.t.double() * d["gate"]
        parts, mags = [column_sums(g), column_sums(g * d["xhat"][0])], [column_sums(g.abs()), column_sums((g * d["xhat"][0]).abs())]
        depth = [stat_depth(c, leaf, False) - 1, stat_depth(c, leaf, True)]
        if c.epi.endswith("2"):
            parts += [column_sums(g), column_sums(g * d["xhat"][1])]
            mags += [column_sums(g.abs()), column_sums((g * d["xhat"][1]).abs())]
            depth += depth
        bound = None
        if kind != "int":
            bound = torch.cat([dd * U * m for dd, m in zip(depth, mags)])
        worst = max(worst, check(what + " sums", sums.t, torch.cat(parts), bound))
    return worst


def run_wgrad(ops, ws, c, kind, prec, d, leaf, what):
    pad, Ho, Wo = geometry(c)
    acc = c.epi == "+"
    dw = Framed((c.Cout, c.k, c.k, c.Cin), d["prev"] if acc else NAN)
    arm(ws, R.WS_FULL)
    Launch(ops, ws, c, prec, what).call(leaf, "sbl_conv2d_wgrad", d["x"].ptr(), d["dy"].ptr(), dw.ptr(), c.NIMG, c.H, c.W, c.Cin, c.Cout, c.k, c.k,
                                        c.stride, pad, int(acc), S())
    dw.check_frame(what + " dw")
    worst = check(what + " dw", dw.t, reference(d, c, kind, prec), out_bound(d, c, kind, prec, leaf))
    # both forms of the unpack: one fp32 assignment / addition per element, so torch's own fp32 result is the exact reference
    for accumulate in (0, 1):
        out = Framed((c.Cout, c.Cin, c.k, c.k), d["unpack_prev"] if accumulate else NAN)
        ops.call("sbl_conv_wgrad_unpack", dw.ptr(), out.ptr(), c.Cout, c.Cin, c.k, c.k, accumulate, S())
        out.check_frame(what + " unpack")
        want = dw.t.permute(0, 3, 1, 2)
        assert torch.equal(out.t, d["unpack_prev"] + want if accumulate else want.contiguous()), "%s: unpack (accumulate %d)" % (what, accumulate)
    return worst


RUN = {"fwd": run_fwd, "dgrad": run_dgrad, "wgrad": run_wgrad}


def run_case(ops, ws, c, kind):
    d = problem(c, kind)
    worst = 0.0
    try:
        knobs(ops, c)
        for prec in R.PRECS:
            leaf = R.route(c, prec)
            assert leaf == c.leaf[prec]
            ops.set_matmul_precision(prec)
            worst = max(worst, RUN[c.op](ops, ws, c, kind, prec, d, leaf, "%s %s %s" % (c.name, kind, prec)))
    finally:
        restore(ops)
    return worst


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_conv_exact(ops, wsbuf, case):
    """Integer data, all four precisions: y / dx / compact dx / dw and both halves of stats / sums EQUAL the integer result on
    every leaf; route, kernel id, launch count, guard blocks and re-armed counters checked after every launch; bnstats gives
    the bits of the plain input gradient; dw_zeroed = 1 adds onto the previous contents; both unpack forms; weight pack.
    No tolerance: nothing to measure."""
    run_case(ops, wsbuf, case, "int")


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_conv_rounded(ops, wsbuf, case):
    """Uniform data: f32 and bf16x6 against float64, bf16x3 and bf16 against tests/bf16_model.py, within the derived bounds of
    the module docstring (outputs elementwise, statistics against float64 sums over the kernel's own output).
    measured (worst err / bound over all cases, MI355X): y 0.31 / dx 0.33 / dw 0.14 under f32 (the K = 16 cases, 1x1 with 16
    input channels: the bound has the least slack at the shortest K), 0.10 / 0.13 / 0.17 under bf16x6, 0.09 / 0.13 / 0.14 under
    bf16x3, 0.09 / 0.11 / 0.05 under bf16; stats 0.15 (bf16x6, 1x1 / stride 2 on a 7x5 map), sums 0.09 (f32, 2x2 map)."""
    run_case(ops, wsbuf, case, "uni")


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_conv_planes_exact(ops, wsbuf, case):
    """Integer operands that need two and three bf16 planes (wide_ints), every product and sum still exact in fp32: under f32
    and bf16x6 (all plane pairs the values need are among its six) y / dx / dw EQUAL the integer convolution, under bf16x3 and
    bf16 they EQUAL tests/bf16_model.py - a dropped, doubled or mis-paired plane changes an output by at least 1.  Statistics
    (outputs of millions: their squares leave fp32's exact range) are held to the rounded bound over the stored output.
    measured: stats 0.17 (bf16, 1x1 / stride 2 on a 7x5 map); sums came out exact."""
    run_case(ops, wsbuf, case, "planes")
