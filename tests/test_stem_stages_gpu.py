"""The stem (csrc/stem.hip) stage by stage through the C ABI: sbl_stem_conv_fwd, sbl_stem_bn_relu_pool_fwd,
sbl_stem_bwd_reduce, sbl_stem_wgrad and the two uint8-source entry points, on buffers this module allocates, each
against the float64 reference of tests/stem_reference.py at the cases of its table (one partial tile, T < 5, odd tile
counts, partial tiles both ways, and tile counts above every persistent grid's cap).

Every launch is checked two ways:
  * frame: every output (conv_out, stats, pooled, argmax, sums, dw, dgamma, dbeta) is a view into a larger buffer with
    64 sentinel elements before and after it (-777.25; 0xEE for the argmax bytes) and is prefilled with NaN (0xEE);
    afterwards the guards must be untouched and no element of the extent may still hold the prefill.  The fp32 clip
    sits between NaN guards, so a load outside the clip that reaches an MFMA poisons the output.  (The uint8 frames of
    the raw source have no such guard - every byte is a legal table index - so a byte load outside the frames shows
    only through the value comparison.)
  * value, EXACT tier, all four precisions, no tolerance: integer data chosen so that (asserted on the reference alone,
    tests/test_stem_reference_cpu.py) every fp32 partial sum in any order is representable - conv_out, the statistics,
    pooled, every argmax byte, the reduction's sums and dw must equal the reference bit for bit.  The argmax is an
    INPUT of the backward entry points, so they also run on a synthetic one that carries every code at every window
    class, codes into the pool's padding included.
  * value, ROUNDED tier, small cases, detfill data: elementwise derived bounds, U = 2^-24.
      forward (f32, bf16x6)  |conv_out - ref| <= (246 + c) U (|x| * |w|)  (+ 2^-26 (|x| * |w|) under bf16x6), c = 0:
          an output element is ONE accumulator element over the whole padded K in both kernels (stem_conv_fwd_kernel:
          the `for ks < ST_KP / 2` MFMA loop, stored from acc0 / acc1 directly; sb_tile_compute: acc[c] over the 18
          k-steps) - no partial sums of one output meet anywhere.
          stats against the float64 sums of the conv_out the kernel itself wrote: <= (n + 1) U sum|terms|,
          n = stem_reference.stats_chain(): 16 rows per tile and thread + 1 shuffle add + 3 (f32: red[0] + .. + red[3])
          or 8 (bf2: eight partials from 0); one tile per thread on these cases, n = 20 / 25.
      pool (once: the kernel has no precision)  |pooled - ref| <= 4 U (|(v - mu) is gamma| + |beta|) at the window's
          maximum; the recorded argmax must be a non-padding tap whose float64 y is within twice that of the maximum.
      reduce  |sums - ref| <= (n + 1) U sum|g| and (n + 4) U sum|g xhat|, n = stem_reference.reduce_chain(): pixels per
          thread (ceil(Wo / 16) per row walked) + 16 partials; the data has no y within 8 U (|xhat gamma| + |beta|) of
          the ReLU threshold, so the fp32 (y > 0) decisions are the float64 ones.
      wgrad (f32, bf16x6; fed the reference's sums)
          |dw - ref| <= sum_pix 8 U |gamma is| (|g| + |mg| + |xhat| |mgx|) |patch| + (P + c) U sum_pix |dconv| |patch|
          (+ 2^-26 sum |dconv| |patch| under bf16x6), P = the pixels whose tap k lies inside the clip
          (stem_reference.contributing_pixels(), per k), c = stem_reference.wgrad_meets(): one float atomic per workgroup
          (two for taps k >= 224, the tap tile two wavefronts share in stem_wgrad_tr_kernel).
    bf16x3 and bf16 split an in-kernel fp32 value (dconv) into bf16 planes, so their weight gradient has no tight
    rounded reference: for them the exact tier is the test.  Their forward has an operand-rounded test in
    tests/test_reduced_precision_gpu.py.

check() prints the worst err / bound ratio of every comparison; the worst measured on an MI355X is in each test's
docstring.

Measured on an MI355X: the module's 175 tests take 4.7 - 5.3 s in all (the slowest, the first 900-tile launch, 1.2 s
with the host reference; every other test under 0.5 s).  Worst err / bound: conv_out 0.016, stats 0.111, pooled 0.623 (no argmax
byte differed from the float64 first maximum), sums 0.089, dw 0.253.  No kernel bug was found: every exact comparison
held bit for bit in all four precisions.  That the tests can fail was shown on a scratch build with five value-only
changes to csrc/stem.hip: `>=` for `>` in the pool (test_pool_exact, test_pool_above_its_grid_cap), the `ph0 + 1 < Hp` mask
dropped from stem_gather_apply (test_reduce_exact, test_reduce_rounded, test_reduce_above_its_grid_cap), the `pw0 + 1 < Wp`
mask dropped from stem_wgrad_tr_kernel's own gather (test_wgrad_exact and test_u8_source_exact in the three split-bf16
modes, test_wgrad_rounded[bf16x6]), st_koff(100) off by one column (test_conv_fwd_exact, test_conv_fwd_rounded,
test_wgrad_exact and test_wgrad_rounded under f32 only - the split-bf16 forward, which does not use st_koff, passed),
st_raw_resolve taking min(sf, 1) for the source frame (test_u8_source_exact's conv_out in the split-bf16 modes, where
nothing else touches the forward: on 2x5x20x36 the first wrong element is the first of clip n = 1, the only clip
that reads frames 2 and 3).
"""
import numpy as np
import pytest
import torch

import stem_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = R.U
PRECS = ("f32", "bf16x6", "bf16x3", "bf16")
ROUNDED_PRECS = ("f32", "bf16x6")
SENT = -777.25                       # guard value (not an integer: never a legal exact result)
SENT_U8 = 0xEE                       # guard and prefill of the argmax bytes (a stored code is 0..8)
G = 64                               # guard elements on each side
NAN = float("nan")
ROUNDED = [c for c in R.CASES if c.rounded]
ids = lambda c: c.name


@pytest.fixture(scope="module", autouse=True)
def ops():
    from sbl_for_multilingual_lip_reading_amd import _lib, ops as _ops
    _lib.load()
    assert torch.cuda.is_available()
    prev = _ops.get_matmul_precision()
    yield _ops
    _ops.set_matmul_precision(prev)


# --------------------------------------------------------------------------- helpers
def S():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    return t.data_ptr()


class Frame:
    """An output of `shape` inside a buffer with G sentinel elements on each side, prefilled with NaN (0xEE for bytes)."""

    def __init__(self, what, shape, dtype=torch.float32):
        self.what, self.n, self.u8 = what, int(np.prod(shape)), dtype == torch.uint8
        self.buf = torch.full((self.n + 2 * G,), SENT_U8 if self.u8 else SENT, dtype=dtype, device=DEV)
        self.t = self.buf[G:G + self.n].view(shape)
        if not self.u8:
            self.t.fill_(NAN)

    def ptr(self):
        return self.t.data_ptr()

    def check(self):
        guard = torch.cat([self.buf[:G], self.buf[G + self.n:]])
        assert bool((guard == (SENT_U8 if self.u8 else SENT)).all()), self.what + ": a guard element was written"
        left = int((self.t == SENT_U8).sum()) if self.u8 else int(torch.isnan(self.t).sum())
        assert left == 0, "%s: %d of %d elements still hold the prefill" % (self.what, left, self.n)
        return self.t


def guarded_clip(x):
    """The fp32 clip between NaN guards."""
    buf = torch.full((x.size + 2 * G,), NAN, dtype=torch.float32, device=DEV)
    v = buf[G:G + x.size].view(x.shape)
    v.copy_(torch.from_numpy(x))
    return buf, v


def dev(a):
    return (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a.contiguous()).to(DEV)


def check(what, got, ref, bound):
    """|got - ref| <= bound elementwise in float64, on the device `ref` lives on (bound None: exact).  Returns worst
    err / bound."""
    got = got.to(ref.device).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what + ": non-finite output"
    err = (got - ref).abs()
    if bound is None:
        bad = int((err != 0).sum())
        assert bad == 0, "%s: %d of %d elements differ from the exact result (max %.3e, first at flat index %d)" % (
            what, bad, ref.numel(), float(err.max()), int((err != 0).reshape(-1).to(torch.uint8).argmax()))
        return 0.0
    ratio = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                        torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    worst = float(ratio.max())
    print("%-64s worst err/bound %.3f  (max err %.3e)" % (what, worst, float(err.max())))
    assert worst <= 1.0, "%s: err/bound %.3f at flat index %d" % (what, worst, int(ratio.argmax()))
    return worst


_DEV = {}


def inputs(tier, name):
    """(reference dict, device tensors) of one (tier, case), built once and left unchanged."""
    key = (tier, name)
    if key not in _DEV:
        r = {"exact": R.exact_reference, "rounded": R.rounded_reference, "raw": R.raw_reference}[tier](name)
        d = {k: dev(v) for k, v in r["in"].items() if k != "x"}
        if tier == "raw":      # no fp32 clip exists: the launches read the bytes
            d["raw"] = [dev(r["raw"][k]) for k in ("frames", "lut", "y1", "x1", "flip", "src_frame")]
        else:
            d["xbuf"], d["x"] = guarded_clip(r["in"]["x"])
        _DEV[key] = (r, d)
    return _DEV[key]


def bn_ptrs(d):
    return [P(d[k]) for k in ("mean", "invstd", "gamma", "beta")]


# --------------------------------------------------------------------------- launches
def run_conv(ops, c, d, raw=None):
    g = R.geom(c)
    conv = Frame("conv_out", (g["NT"], g["Ho"], g["Wo"], 64))
    stats = Frame("stats", (128,), torch.float64)
    if raw is None:
        ops.call("sbl_stem_conv_fwd", P(d["x"]), P(d["w"]), conv.ptr(), stats.ptr(), c.N, c.T, c.H, c.W, S())
    else:
        ops.call("sbl_stem_conv_fwd_u8", *[P(t) for t in d["raw"]], P(d["w"]), conv.ptr(), stats.ptr(), *raw["dims"], S())
    torch.cuda.synchronize()
    return conv.check().cpu(), stats.check().cpu()


def run_pool(ops, NT, Ho, Wo, conv_in, d):
    pooled = Frame("pooled", (NT, Ho // 2, Wo // 2, 64))
    argmax = Frame("argmax", (NT, Ho // 2, Wo // 2, 64), torch.uint8)
    ops.call("sbl_stem_bn_relu_pool_fwd", P(conv_in), *bn_ptrs(d), pooled.ptr(), argmax.ptr(), NT, Ho, Wo, S())
    torch.cuda.synchronize()
    return pooled.check(), argmax.check()


def run_reduce(ops, NT, Ho, Wo, conv_in, dpooled, argmax, d):
    sums = Frame("sums", (128,), torch.float64)
    ops.call("sbl_stem_bwd_reduce", P(conv_in), P(dpooled), P(argmax), *bn_ptrs(d), sums.ptr(), NT, Ho, Wo, S())
    torch.cuda.synchronize()
    return sums.check()


def run_wgrad(ops, c, d, argmax, sums, raw=None):
    dw, dgamma, dbeta = Frame("dw", (64, R.K)), Frame("dgamma", (64,)), Frame("dbeta", (64,))
    tail = [P(d["conv_in"]), P(d["dpooled"]), P(argmax), *bn_ptrs(d), P(sums), dw.ptr(), dgamma.ptr(), dbeta.ptr()]
    if raw is None:
        ops.call("sbl_stem_wgrad", P(d["x"]), *tail, c.N, c.T, c.H, c.W, S())
    else:
        ops.call("sbl_stem_wgrad_u8", *[P(t) for t in d["raw"]], *tail, *raw["dims"], S())
    torch.cuda.synchronize()
    s32 = sums.to(torch.float32)
    assert torch.equal(dgamma.check(), s32[64:]) and torch.equal(dbeta.check(), s32[:64]), "dgamma / dbeta are not (float)sums"
    return dw.check().cpu()


def conv_exact(ops, c, r, d, raw=None):
    got, stats = run_conv(ops, c, d, raw)
    check("conv_out", got, r["conv"], None)
    want = torch.cat([r["conv"].sum((0, 1, 2)), (r["conv"] * r["conv"]).sum((0, 1, 2))])
    check("stats", stats, want, None)


def wgrad_exact(ops, c, r, d, raw=None):
    for tag, am, sums in r["settings"]:
        dw = run_wgrad(ops, c, d, dev(am), dev(sums), raw)
        check("dw " + tag, dw, r["dw_" + tag], None)


# --------------------------------------------------------------------------- exact tier
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", R.CASES, ids=ids)
def test_conv_fwd_exact(ops, case, prec):
    ops.set_matmul_precision(prec)
    r, d = inputs("exact", case.name)
    conv_exact(ops, case, r, d)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", R.CASES, ids=ids)
def test_pool_exact(ops, case, prec):
    ops.set_matmul_precision(prec)
    r, d = inputs("exact", case.name)
    g = R.geom(case)
    pooled, argmax = run_pool(ops, g["NT"], g["Ho"], g["Wo"], d["conv_in"], d)
    check("pooled", pooled.cpu(), r["pooled"], None)
    bad = int((argmax.cpu() != r["code"]).sum())
    assert bad == 0, "%d argmax bytes differ" % bad


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", R.CASES, ids=ids)
def test_reduce_exact(ops, case, prec):
    """Run A: the reference's own argmax.  Run B: the synthetic one (every code at every window class; the top row's and
    left column's codes into the padding must route nowhere, the last row's and column's must count once)."""
    ops.set_matmul_precision(prec)
    r, d = inputs("exact", case.name)
    g = R.geom(case)
    for tag, am in (("own", dev(r["code"])), ("syn", d["argmax_syn"])):
        sums = run_reduce(ops, g["NT"], g["Ho"], g["Wo"], d["conv_in"], d["dpooled"], am, d)
        check("sums " + tag, sums.cpu(), r["sums_" + tag], None)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", R.CASES, ids=ids)
def test_wgrad_exact(ops, case, prec):
    """sums = 0 with the synthetic and the reference's argmax; sums = cnt (a, b) on the power-of-two cases."""
    ops.set_matmul_precision(prec)
    r, d = inputs("exact", case.name)
    wgrad_exact(ops, case, r, d)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", sorted(R.U8_CASES))
def test_u8_source_exact(ops, name, prec):
    """sbl_stem_conv_fwd_u8 / sbl_stem_wgrad_u8 against materialize() followed by the reference: random bytes, an integer
    table; 2x5x20x36 crops 20 x 36 out of 28 x 40 frames at random origins, 3x257x8x8 reads whole frames on 771 tiles and
    ends in an all -1 clip.  In both, a flipped and an unflipped clip are live, source frames >= 1 are read at n >= 1,
    a frame repeats and every live row has a -1 tail (test_stem_reference_cpu.py::test_raw_source_preconditions asserts it)."""
    ops.set_matmul_precision(prec)
    r, d = inputs("raw", name)
    conv_exact(ops, R.BY_NAME[name], r, d, r["raw"])
    wgrad_exact(ops, R.BY_NAME[name], r, d, r["raw"])


@pytest.mark.parametrize("shape", R.REDUCE_CAPS, ids=lambda s: "x".join(map(str, s)))
def test_reduce_above_its_grid_cap(ops, shape):
    """69,696 pixels: more than the 4096 workgroups x 16 pixels of the grid formula; and 4160 pixel rows of 52: more rows
    than workgroups and more columns than one trip of the column loop.  Data generated and referenced on the device."""
    NT, Ho, Wo = shape
    d = R.reduce_cap_inputs(shape, DEV)
    dd = {k: dev(d[k]) for k in ("mean", "invstd", "gamma", "beta")}
    sums = run_reduce(ops, NT, Ho, Wo, d["conv_in"], d["dpooled"], d["argmax"], dd)
    check("sums", sums, R.reduce(d["conv_in"], d["dpooled"], d["argmax"], *R.bn_args(d)), None)


def test_pool_above_its_grid_cap(ops):
    """131,648 pooled pixels: more than the 8192 blocks x 16 of one round.  Integer data generated on the device; the
    reference is the key rule in int64 (max over the taps of 2y * 16 + 8 - t) on the float64 y."""
    NT, Ho, Wo = R.POOL_CAP
    d = R.pool_cap_inputs(DEV)
    dd = {k: dev(d[k]) for k in ("mean", "invstd", "gamma", "beta")}
    pooled, argmax = run_pool(ops, NT, Ho, Wo, d["conv_in"], dd)
    y2 = 2 * R.bn(d["conv_in"], *R.bn_args(d))[1].clamp_min(0.0)
    assert R.quantum_ok(y2, 1.0)
    want, code = R.pool_key(y2.to(torch.int64))
    check("pooled", pooled, want.double() / 2, None)
    bad = int((argmax != code).sum())
    assert bad == 0, "%d argmax bytes differ" % bad


# --------------------------------------------------------------------------- rounded tier
@pytest.mark.parametrize("prec", ROUNDED_PRECS)
@pytest.mark.parametrize("case", ROUNDED, ids=ids)
def test_conv_fwd_rounded(ops, case, prec):
    """(246 + c) U (|x| * |w|), c = 0 in both kernels (module docstring).  Measured worst err / bound: conv_out 0.016
    (2x5x20x36, f32), stats 0.111 (1x1x8x8, f32)."""
    ops.set_matmul_precision(prec)
    r, d = inputs("rounded", case.name)
    got, stats = run_conv(ops, case, d)
    mag = r["conv_abs"]
    check("conv_out %s %s" % (case.name, prec), got, r["conv"], (246 + 0) * U * mag + (2.0 ** -26 * mag if prec != "f32" else 0))
    g64 = got.double()
    own = torch.cat([g64.sum((0, 1, 2)), (g64 * g64).sum((0, 1, 2))])
    terms = torch.cat([g64.abs().sum((0, 1, 2)), (g64 * g64).sum((0, 1, 2))])
    n = R.stats_chain(R.geom(case)["ntiles"], prec)
    check("stats %s %s (n = %d)" % (case.name, prec, n), stats, own, (n + 1) * U * terms)


@pytest.mark.parametrize("case", ROUNDED, ids=ids)
def test_pool_rounded(ops, case):
    """Measured worst err / bound 0.623 (2x2x32x32); no recorded position differed from the float64 first maximum."""
    r, d = inputs("rounded", case.name)
    g = R.geom(case)
    pooled, argmax = run_pool(ops, g["NT"], g["Ho"], g["Wo"], d["conv_in"], d)
    pooled, code = pooled.cpu(), argmax.cpu().to(torch.int64)
    mag = torch.stack(R.pool_taps(r["pool_mag"], 0.0))
    bound = 4 * U * mag.gather(0, r["code"].to(torch.int64).unsqueeze(0))[0]          # at the window's (float64) maximum
    check("pooled %s" % case.name, pooled, r["pooled"], bound)
    assert int(code.max()) <= 8
    valid = torch.stack(R.pool_taps(torch.ones_like(r["y"]), 0.0)).gather(0, code.unsqueeze(0))[0]
    assert bool((valid == 1).all()), "an argmax byte names a padding tap"
    y_at = torch.stack(R.pool_taps(r["y"], float("-inf"))).gather(0, code.unsqueeze(0))[0]
    short = r["pooled"] - y_at
    print("argmax %s: %d of %d positions differ from the float64 first maximum, worst shortfall / (2 bound) %.3f" % (
        case.name, int((code != r["code"].to(torch.int64)).sum()), code.numel(),
        float((short / (2 * bound).clamp_min(1e-300)).max())))
    assert bool((short <= 2 * bound).all())


@pytest.mark.parametrize("case", ROUNDED, ids=ids)
def test_reduce_rounded(ops, case):
    """Measured worst err / bound 0.089 (1x2x8x12)."""
    r, d = inputs("rounded", case.name)
    g = R.geom(case)
    sums = run_reduce(ops, g["NT"], g["Ho"], g["Wo"], d["conv_in"], d["dpooled"], dev(r["code"]), d).cpu()
    n = R.reduce_chain(g["NT"], g["Ho"], g["Wo"])
    bound = torch.cat([(n + 1) * U * r["sums_mag"][:64], (n + 4) * U * r["sums_mag"][64:]])
    check("sums %s (n = %d)" % (case.name, n), sums, r["sums"], bound)


@pytest.mark.parametrize("prec", ROUNDED_PRECS)
@pytest.mark.parametrize("case", ROUNDED, ids=ids)
def test_wgrad_rounded(ops, case, prec):
    """Measured worst err / bound 0.183 (1x2x8x12, f32); 0.253 under bf16x6 (1x3x8x8)."""
    ops.set_matmul_precision(prec)
    r, d = inputs("rounded", case.name)
    g = R.geom(case)
    dw = run_wgrad(ops, case, d, dev(r["code"]), dev(r["sums"]))
    c, Pk = R.wgrad_meets(g["ntiles"], prec), r["dw_P"]                # per tap k, broadcast over co
    bound = r["dw_form"] + (Pk + c).view(1, R.K) * U * r["dw_mag"] + (2.0 ** -26 * r["dw_mag"] if prec != "f32" else 0)
    check("dw %s %s (P = %d..%d of %d, c = %d..%d)" % (case.name, prec, int(Pk.min()), int(Pk.max()), g["cnt"], int(c.min()), int(c.max())),
          dw, r["dw"], bound)
