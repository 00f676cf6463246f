"""Float64 reference of the stem (csrc/stem.hip), one function per ABI entry point, and the case table of
tests/test_stem_stages_gpu.py.  Plain torch / numpy: no GPU is needed and nothing of the package's `ops` is used; the
functions run on whatever device their arguments live on (the two grid-cap cases of the pool and the reduction are
generated and referenced there).

Layouts are the kernels': conv_out / pooled / argmax / dpooled are NHWC (N*T, h, w, 64); the weights are (64, 245) with
k = (kt*7 + kh)*7 + kw; the clip is (N, T, H, W).  Every function takes exactly the arguments of its entry point.

    conv(x, w2), conv_abs(x, w2)                      sbl_stem_conv_fwd        (patches(x) @ w2^T: no library convolution)
    pool(conv_out, mean, invstd, gamma, beta)         sbl_stem_bn_relu_pool_fwd
    gather_g(conv_out, dpooled, argmax, ...)          stem_gather_apply: the max-pool adjoint times the ReLU mask
    reduce(conv_out, dpooled, argmax, ...)            sbl_stem_bwd_reduce
    wgrad(x, conv_out, dpooled, argmax, ..., sums)    sbl_stem_wgrad
    materialize(frames_u8, lut, y1, x1, flip, ...)    the fp32 clip a StemSrcU8 stands for
"""
import collections

import numpy as np
import torch

from sbl_for_multilingual_lip_reading_amd import detfill

U = 2.0 ** -24
EXACT_LIMIT = float(1 << 24)
KT, KH, KW, K = 5, 7, 7, 245
TILE_H, TILE_W = 8, 16


def t64(a, device=None):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    a = a.to(torch.float64)
    return a if device is None else a.to(device)


def _c(v):
    """A per-channel vector, broadcast over NHWC."""
    return t64(v).view(1, 1, 1, 64)


# --------------------------------------------------------------------------- the stages
def patches(x):
    """(N*T*Ho*Wo, 245) float64: column k = (kt*7 + kh)*7 + kw of pixel (n, t, oh, ow) is x[n, t + kt - 2, 2 oh + kh - 3,
    2 ow + kw - 3], zero outside the clip."""
    x = t64(x)
    N, T, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    xp = torch.nn.functional.pad(x, (3, 3, 3, 3, 2, 2))
    cols = []
    for kt in range(KT):
        for kh in range(KH):
            for kw in range(KW):
                cols.append(xp[:, kt:kt + T, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2].reshape(-1))
    return torch.stack(cols, 1)


def conv(x, w2, pat=None):
    """Conv3d(1, 64, (5,7,7), stride (1,2,2), pad (2,3,3)) -> (N*T, Ho, Wo, 64)."""
    N, T, H, W = x.shape
    p = patches(x) if pat is None else pat
    return (p @ t64(w2).t()).view(N * T, H // 2, W // 2, 64)


def conv_abs(x, w2, pat=None):
    """|x| * |w|: the magnitude the forward bounds are stated in."""
    N, T, H, W = x.shape
    p = patches(x) if pat is None else pat
    return (p.abs() @ t64(w2).abs().t()).view(N * T, H // 2, W // 2, 64)


def bn(conv_out, mean, invstd, gamma, beta):
    """(xhat, y before the ReLU)"""
    v = t64(conv_out)
    xh = (v - _c(mean).to(v.device)) * _c(invstd).to(v.device)
    return xh, xh * _c(gamma).to(v.device) + _c(beta).to(v.device)


def pool_taps(a, fill):
    """The nine taps t = kh*3 + kw of every 3x3 / stride 2 / pad 1 window of an NHWC map: a list of (NT, Hp, Wp, C)."""
    NT, Ho, Wo, C = a.shape
    Hp, Wp = Ho // 2, Wo // 2
    ap = torch.full((NT, Ho + 2, Wo + 2, C), fill, dtype=a.dtype, device=a.device)
    ap[:, 1:Ho + 1, 1:Wo + 1] = a
    return [ap[:, kh:kh + 2 * Hp:2, kw:kw + 2 * Wp:2] for kh in range(3) for kw in range(3)]


def pool(conv_out, mean, invstd, gamma, beta):
    """-> (pooled float64, argmax uint8, y).  argmax = the FIRST tap in (kh, kw) scan order that equals the window's
    maximum, as kh*3 + kw (stem_bn_relu_pool_kernel's rule).  No library argmax is involved: the code is the smallest
    t whose tap equals the maximum.  On integer y this is the maximum over the taps of the key y*16 + (8 - t)."""
    y = bn(conv_out, mean, invstd, gamma, beta)[1].clamp_min(0.0)
    taps = pool_taps(y, float("-inf"))
    m = taps[0]
    for t in range(1, 9):
        m = torch.maximum(m, taps[t])
    code = torch.full(m.shape, 9, dtype=torch.uint8, device=m.device)
    for t in range(8, -1, -1):
        code = torch.where(taps[t] == m, torch.full_like(code, t), code)
    return m, code, y


def pool_key(y_int):
    """The key form of the same rule for integer y (int64 NHWC, 0 <= y; the exact regime's y is a multiple of 1/2, so
    callers pass 2 y and halve the result): max over taps of y*16 + (8 - t) -> (pooled, code).  Padding taps carry a
    negative key."""
    taps = pool_taps(y_int * 16 + 8, -1)
    key = taps[0]
    for t in range(1, 9):
        key = torch.maximum(key, taps[t] - t)
    return key >> 4, (8 - (key & 15)).to(torch.uint8)


def gather_g(conv_out, dpooled, argmax, mean, invstd, gamma, beta):
    """g = the max-pool adjoint routed by the GIVEN argmax codes, times (y > 0) with y before the ReLU.  A code that
    points into the pool's padding (or is not 0..8) routes nowhere."""
    v = t64(conv_out)
    NT, Ho, Wo, C = v.shape
    Hp, Wp = Ho // 2, Wo // 2
    d = t64(dpooled).to(v.device)
    am = argmax.to(v.device)
    gp = torch.zeros((NT, Ho + 2, Wo + 2, C), dtype=torch.float64, device=v.device)
    for t in range(9):
        kh, kw = divmod(t, 3)
        gp[:, kh:kh + 2 * Hp:2, kw:kw + 2 * Wp:2] += torch.where(am == t, d, torch.zeros_like(d))
    y = bn(v, mean, invstd, gamma, beta)[1]
    return gp[:, 1:Ho + 1, 1:Wo + 1] * (y > 0)


def reduce(conv_out, dpooled, argmax, mean, invstd, gamma, beta):
    """sums[128] = (sum g, sum g * xhat) per channel."""
    g = gather_g(conv_out, dpooled, argmax, mean, invstd, gamma, beta)
    xh = bn(conv_out, mean, invstd, gamma, beta)[0]
    return torch.cat([g.sum((0, 1, 2)), (g * xh).sum((0, 1, 2))])


def dconv_of(conv_out, dpooled, argmax, mean, invstd, gamma, beta, sums):
    v = t64(conv_out)
    cnt = float(v.shape[0] * v.shape[1] * v.shape[2])
    s = t64(sums).to(v.device)
    g = gather_g(v, dpooled, argmax, mean, invstd, gamma, beta)
    xh = bn(v, mean, invstd, gamma, beta)[0]
    return _c(gamma).to(v.device) * _c(invstd).to(v.device) * (g - (s[:64] / cnt).view(1, 1, 1, 64) - xh * (s[64:] / cnt).view(1, 1, 1, 64))


def wgrad(x, conv_out, dpooled, argmax, mean, invstd, gamma, beta, sums, pat=None):
    """-> (dw (64, 245) float64, dgamma float32, dbeta float32)"""
    dc = dconv_of(conv_out, dpooled, argmax, mean, invstd, gamma, beta, sums)
    p = patches(x) if pat is None else pat
    s32 = t64(sums).to(torch.float32)
    return dc.reshape(-1, 64).t() @ p, s32[64:].clone(), s32[:64].clone()


def materialize(frames_u8, lut, y1, x1, flip, src_frame, Tout, Hc, Wc):
    """out[n, tt, ih, iw] = lut[in[n, src_frame[n, tt], y1[n] + ih, x1[n] + (flip[n] ? Wc-1-iw : iw)]]; a zero frame for
    src_frame < 0 or >= Tin, zero for any resolved coordinate outside the frame.  numpy in, float32 out."""
    N, Tin, Hin, Win = frames_u8.shape
    out = np.zeros((N, Tout, Hc, Wc), dtype=np.float32)
    ih, iw = np.arange(Hc), np.arange(Wc)
    for n in range(N):
        sy = int(y1[n]) + ih
        sx = int(x1[n]) + (Wc - 1 - iw if flip[n] else iw)
        ok = ((sy >= 0) & (sy < Hin))[:, None] & ((sx >= 0) & (sx < Win))[None, :]
        syc, sxc = np.clip(sy, 0, Hin - 1), np.clip(sx, 0, Win - 1)
        for tt in range(Tout):
            sf = int(src_frame[n, tt])
            if 0 <= sf < Tin:
                out[n, tt] = np.where(ok, lut[frames_u8[n, sf][syc[:, None], sxc[None, :]]], np.float32(0))
    return out


# --------------------------------------------------------------------------- the case table
Case = collections.namedtuple("Case", "name N T H W hi rounded pow2 edge")
# hi: x and w of the exact tier are integers in [-hi, hi].  Tiles are 8 x 16 output pixels.
CASES = [
    Case("1x1x8x8", 1, 1, 8, 8, 3, True, False,
         "1 tile, partial 4x4; four of five temporal taps in padding; pool 2x2, every window touches the padding"),
    Case("1x2x8x12", 1, 2, 8, 12, 3, True, False, "T = 2, Wo = 6"),
    Case("1x3x8x8", 1, 3, 8, 8, 3, True, False, "3 tiles: the bf2 forward's last pair has one live tile"),
    Case("2x5x20x36", 2, 5, 20, 36, 3, True, False,
         "40 tiles; Ho = 10 -> tiles 8 + 2, Wo = 18 -> tiles 16 + 2; every temporal tap live only at t = 2"),
    Case("1x4x16x32", 1, 4, 16, 32, 3, True, True, "exactly one full tile per frame; cnt = 512: the nonzero-sums wgrad setting"),
    Case("2x2x32x32", 2, 2, 32, 32, 3, True, True, "cnt = 1024, TY = 2"),
    # grid caps (512 f32 forward, 2 x 256 bf2 forward, 768 / 512 weight gradients): exact tier only, data in {-1, 0, 1}
    # ([-3, 3] would push the sum of squares of the 900-tile case past 2^24)
    Case("3x257x8x8", 3, 257, 8, 8, 1, False, False, "771 tiles: odd, above every conv / wgrad cap, ragged last round; T above any grid stride"),
    Case("5x20x40x72", 5, 20, 40, 72, 1, False, False, "900 tiles: TY = TX = 3, partial tiles both ways, above every cap"),
]
BY_NAME = {c.name: c for c in CASES}
# raw source: case -> (Tin, Hin, Win, all -1 last clip, seed).  2x5x20x36: a crop (Hc < Hin), both clips live.  3x257x8x8:
# frames that are the crop, two live clips and the all -1 clip, 771 tiles (the loaders' one-tile-ahead index prefetch runs
# past every grid cap).  Between them: live clips with flip 0 and with flip 1, source frames >= 1 at n >= 1, repeated
# frames, -1 tails - asserted by tests/test_stem_reference_cpu.py::test_raw_source_preconditions.
U8_CASES = {"2x5x20x36": (5, 28, 40, False, 7), "3x257x8x8": (150, 8, 8, True, 7)}
# NT, Ho, Wo.  (36, 44, 44): 69,696 pixels, above the 4096 x 16 that the reduction's grid formula covers - but its
# workgroups walk pixel ROWS, and 1584 rows leave every workgroup with one.  (130, 32, 52): 4160 rows on 4096 workgroups,
# so 64 of them take a second trip of the row loop, and Wo = 52 > 48 gives the column loop a second, partial trip.
REDUCE_CAPS = [(36, 44, 44), (130, 32, 52)]
POOL_CAP = (272, 44, 44)           # NT, Ho, Wo: 272 * 22 * 22 = 131,648 pooled pixels, above the 8192 x 16 of one round


def geom(c):
    Ho, Wo = c.H // 2, c.W // 2
    TY, TX = -(-Ho // TILE_H), -(-Wo // TILE_W)
    return dict(NT=c.N * c.T, Ho=Ho, Wo=Wo, Hp=Ho // 2, Wp=Wo // 2, TY=TY, TX=TX, ntiles=c.N * c.T * TY * TX, cnt=c.N * c.T * Ho * Wo)


def ints(name, shape, hi):
    """Integers in [-hi, hi] as float32, a function of (name, shape)."""
    return np.rint(detfill.uniform(name, shape) * np.float32(hi)).astype(np.float32)


def pick(name, n, values):
    u = (detfill.uniform(name, (n,)).astype(np.float64) + 1.0) * 0.5
    return np.asarray(values, dtype=np.float32)[np.minimum((u * len(values)).astype(np.int64), len(values) - 1)]


def exact_params(tag):
    """mean integer, invstd in {0.5, 1, 2}, gamma in {-1, 1, 2}, beta integer: every fp32 intermediate of
    (v - mean) * invstd * gamma + beta on integer v is exact, fused or not."""
    return dict(mean=ints("sr.mu." + tag, (64,), 1), invstd=pick("sr.is." + tag, 64, (0.5, 1.0, 2.0)),
                gamma=pick("sr.ga." + tag, 64, (-1.0, 1.0, 2.0)), beta=ints("sr.be." + tag, (64,), 1))


def synthetic_argmax(NT, Hp, Wp):
    """Every code 0..8 at every window class: code = (c + 3 pw + 5 ph + 7 img) mod 9 over the 64 channels.  Windows of
    the top row / left column therefore carry kh = 0 / kw = 0 codes, which point into the pool's padding and must route
    nowhere; with an even map no code of the LAST row or column points outside, but their kh = 2 / kw = 2 codes hit
    the odd last pixel row / column, whose second candidate window does not exist (the `ph0 + 1 < Hp` masks)."""
    img, ph, pw, c = np.ix_(np.arange(NT), np.arange(Hp), np.arange(Wp), np.arange(64))
    return ((c + 3 * pw + 5 * ph + 7 * img) % 9).astype(np.uint8)


def exact_inputs(c):
    """Host inputs of the exact tier of one case (numpy)."""
    g = geom(c)
    d = exact_params(c.name)
    d["x"] = ints("sr.x." + c.name, (c.N, c.T, c.H, c.W), c.hi)
    d["w"] = ints("sr.w." + c.name, (64, K), c.hi)
    d["conv_in"] = ints("sr.v." + c.name, (g["NT"], g["Ho"], g["Wo"], 64), 4)
    d["dpooled"] = ints("sr.dp." + c.name, (g["NT"], g["Hp"], g["Wp"], 64), 3)
    d["argmax_syn"] = synthetic_argmax(g["NT"], g["Hp"], g["Wp"])
    if c.pow2:
        d["sums_ab"] = (np.concatenate([ints("sr.a." + c.name, (64,), 1), ints("sr.b." + c.name, (64,), 1)]).astype(np.float64) * g["cnt"])
    return d


def device_ints(shape, hi, salt, device):
    """Integers in [-hi, hi] (int64) from the flat index, the same on every device: the grid-cap inputs that are too
    large to ship from the host."""
    n = int(np.prod(shape))
    i = torch.arange(n, dtype=torch.int64, device=device)
    h = (i * 2654435761 + salt * 40503) & 0xFFFFFFFF
    h = ((h ^ (h >> 15)) * 2246822519) & 0xFFFFFFFF
    h = h ^ (h >> 13)
    return ((h >> 3) % (2 * hi + 1) - hi).view(shape)


def reduce_cap_inputs(shape, device):
    """Synthetic integer conv_out in [-4, 4], dpooled in [-3, 3] and uniformly random argmax codes 0..8 at one of REDUCE_CAPS."""
    NT, Ho, Wo = shape
    d = exact_params("rcap")
    d["conv_in"] = device_ints((NT, Ho, Wo, 64), 4, 1, device).to(torch.float32)
    d["dpooled"] = device_ints((NT, Ho // 2, Wo // 2, 64), 3, 2, device).to(torch.float32)
    d["argmax"] = (device_ints((NT, Ho // 2, Wo // 2, 64), 4, 3, device) + 4).to(torch.uint8)
    return d


def pool_cap_inputs(device):
    NT, Ho, Wo = POOL_CAP
    d = exact_params("pcap")
    d["conv_in"] = device_ints((NT, Ho, Wo, 64), 4, 5, device).to(torch.float32)
    return d


def raw_inputs(c):
    """uint8 frames and clip integers for case c, built as tests/test_stem_u8_gpu.py's raw_case builds them: random bytes,
    crops at random origins, mixed flips, src_frame rows with repeats and a -1 tail and (zero_clip) the last clip all -1.
    The table is the integer one lut[b] = (b % 7) - 3, so the materialised clip is integers in [-3, 3]."""
    Tin, Hin, Win, zero_clip, seed = U8_CASES[c.name]
    N, Tout, Hc, Wc = c.N, c.T, c.H, c.W
    rng = np.random.RandomState(seed)
    frames = rng.randint(0, 256, size=(N, Tin, Hin, Win)).astype(np.uint8)
    y1 = rng.randint(0, Hin - Hc + 1, size=N).astype(np.int32)
    x1 = rng.randint(0, Win - Wc + 1, size=N).astype(np.int32)
    flip = ((np.arange(N) + seed) % 2).astype(np.int32)
    src = np.full((N, Tout), -1, dtype=np.int32)
    for n in range(N - 1 if zero_clip else N):
        L = int(rng.randint(max(1, Tout // 2), min(Tin, Tout - 1) + 1))
        cur = list(range(L))
        for i in range(1, L):
            if rng.rand() < 0.25:
                cur[i] = cur[i - 1]
        src[n, :L] = cur
    lut = ((np.arange(256) % 7) - 3).astype(np.float32)
    return dict(frames=frames, lut=lut, y1=y1, x1=x1, flip=flip, src_frame=src, dims=(N, Tin, Hin, Win, Tout, Hc, Wc))


# rounded tier: the detfill salt of each small case, chosen (on the CPU, from the reference alone) so that no element of
# the case has |y| < 8 U (|xhat gamma| + |beta|): the fp32 (y > 0) decision then agrees with float64 everywhere
ROUNDED_SALT = {"1x1x8x8": 0, "1x2x8x12": 0, "1x3x8x8": 0, "2x5x20x36": 0, "1x4x16x32": 0, "2x2x32x32": 0}


def rounded_inputs(c):
    """Host inputs of the rounded tier: detfill data scaled as in test_hip_parity.test_stem_fwd_bwd; mean / invstd are the
    batch statistics (eps 1e-5) of the float64 convolution, rounded to fp32, and conv_in is that convolution in fp32."""
    g = geom(c)
    s = ROUNDED_SALT[c.name]
    d = dict(x=detfill.normal("sr.rx." + c.name, (c.N, c.T, c.H, c.W), s),
             w=(detfill.uniform("sr.rw." + c.name, (64, K), s) * np.float32(0.08)).astype(np.float32),
             gamma=(1 + np.float32(0.3) * detfill.uniform("sr.rg." + c.name, (64,), s)).astype(np.float32),
             beta=(np.float32(0.2) * detfill.uniform("sr.rb." + c.name, (64,), s)).astype(np.float32),
             dpooled=detfill.uniform("sr.rdp." + c.name, (g["NT"], g["Hp"], g["Wp"], 64), s))
    v = conv(t64(d["x"]), d["w"])
    mean = v.mean((0, 1, 2))
    var = (v * v).mean((0, 1, 2)) - mean * mean
    d["mean"] = mean.to(torch.float32).numpy()
    d["invstd"] = (1.0 / torch.sqrt(var + 1e-5)).to(torch.float32).numpy()
    d["conv_in"] = v.to(torch.float32).numpy()
    return d


def relu_margin_violations(conv_in, mean, invstd, gamma, beta):
    """Number of elements whose float64 y lies within 8 U (|xhat gamma| + |beta|) of zero."""
    xh, y = bn(conv_in, mean, invstd, gamma, beta)
    return int((y.abs() < 8 * U * ((xh * _c(gamma)).abs() + _c(beta).abs())).sum())


# --------------------------------------------------------------------------- preconditions of the exact tier
def quantum_ok(a, q):
    """Every element of a is a multiple of q."""
    return bool(((a / q) == torch.round(a / q)).all())


def bf16_exact(a):
    """Every element of a survives a round trip through bf16 (one plane of the split holds it)."""
    f = t64(a).to(torch.float32)
    return bool((f.to(torch.bfloat16).to(torch.float32) == f).all())


def forward_preconditions(ref_conv):
    """per channel sum |conv| < 2^24 and sum conv^2 < 2^24 (integers): every fp32 partial sum of the statistics is an
    integer the format holds.  -> the two maxima."""
    s1 = float(ref_conv.abs().sum((0, 1, 2)).max())
    s2 = float((ref_conv * ref_conv).sum((0, 1, 2)).max())
    return s1, s2


def reduce_preconditions(g, xh):
    """g integer, g * xhat a multiple of 1/2; sum |g| < 2^24 and 2 sum |g xhat| < 2^24 per channel (partial sums counted in
    units of the quantum)."""
    gx = g * xh
    assert quantum_ok(g, 1.0) and quantum_ok(gx, 0.5)
    return float(g.abs().sum((0, 1, 2)).max()), 2.0 * float(gx.abs().sum((0, 1, 2)).max())


def wgrad_preconditions(x, dc, pat):
    """max |dconv| <= 256, max |x| <= 256 and both bf16-exact; dconv a multiple of 1/4 and 4 sum_pixels |dconv| |patch|
    < 2^24 per (co, k).  -> that largest sum, in quanta."""
    assert float(dc.abs().max()) <= 256 and float(t64(x).abs().max()) <= 256
    assert bf16_exact(dc) and bf16_exact(x) and quantum_ok(dc, 0.25) and quantum_ok(t64(x), 1.0)
    return 4.0 * float((dc.reshape(-1, 64).abs().t() @ pat.abs()).max())


# --------------------------------------------------------------------------- chain lengths of the rounded bounds
def cdiv(a, b):
    return -(-a // b)


def stats_chain(ntiles, prec):
    """n of the statistics bound: the longest chain of fp32 additions into one partial before the double atomic.
    stem_conv_fwd_kernel: 16 accumulator rows per tile and thread (s1[j] += acc, the epilogue loop), one tile per trip of
    a grid of min(ntiles, 512); one __shfl_xor add; red[0] + red[1] + red[2] + red[3] (3).
    stem_conv_fwd_bf2_kernel: the same per tile, one tile per pair and wavefront group on a grid of min(npairs, 256); one
    shuffle add; the sum of eight partials starting from 0 (8)."""
    if prec == "f32":
        return 16 * cdiv(ntiles, min(ntiles, 512)) + 1 + 3
    npairs = (ntiles + 1) // 2
    return 16 * cdiv(npairs, min(npairs, 256)) + 1 + 8


def reduce_chain(NT, Ho, Wo):
    """n of the reduction bound (stem_bwd_reduce_kernel): a thread adds ceil(Wo / 16) pixels per row it walks (sg[k] +=
    g[k]), a workgroup walks ceil(rows / grid) rows of a grid of min(ceil(pixels / 16), 4096); then 16 partials are added
    from 0 (16) before the double atomic."""
    grid = min(cdiv(NT * Ho * Wo, 16), 4096)
    return cdiv(NT * Ho, grid) * cdiv(Wo, 16) + 16


def wgrad_meets(ntiles, prec):
    """c of the weight-gradient bound per tap k, a (245,) tensor: float atomics into one dw element.  stem_wgrad_kernel: one
    per workgroup of a grid of min(ntiles, 768).  stem_wgrad_tr_kernel: one per workgroup of min(ntiles, 512), two for the
    ninth tap tile - (kt, kh) pairs 32 .. 34, taps k >= 224 - whose k-steps two wavefronts share (flush(accx, 8, wave & 1))."""
    c = torch.full((K,), float(min(ntiles, 768) if prec == "f32" else min(ntiles, 512)), dtype=torch.float64)
    if prec != "f32":
        c[224:] *= 2
    return c


def contributing_pixels(shape):
    """P of the weight-gradient bound per tap k, a (245,) tensor: the pixels whose tap k lies inside the clip (a tap in the
    padding multiplies by an exact zero: its product and its addition do not round)."""
    return patches(torch.ones(shape, dtype=torch.float64)).sum(0)


# --------------------------------------------------------------------------- references, computed once per case
def bn_args(d):
    return d["mean"], d["invstd"], d["gamma"], d["beta"]


def wgrad_settings(c, d, own):
    """(tag, argmax, sums): sums = 0 with the synthetic and with the reference's own argmax; on the power-of-two cases
    also sums[c] = cnt a_c, sums[64 + c] = cnt b_c, whose means the kernels' (float)(sums / cnt) holds exactly."""
    zero = np.zeros(128, dtype=np.float64)
    s = [("zero_syn", torch.from_numpy(d["argmax_syn"]), zero), ("zero_own", own, zero)]
    if c.pow2:
        s.append(("ab_own", own, d["sums_ab"]))
    return s


def _backward_reference(c, d, r, pat, x):
    bnp = bn_args(d)
    r["pooled"], r["code"], _ = pool(d["conv_in"], *bnp)
    xh = bn(d["conv_in"], *bnp)[0]
    for tag, am in (("own", r["code"]), ("syn", torch.from_numpy(d["argmax_syn"]))):
        g = gather_g(d["conv_in"], d["dpooled"], am, *bnp)
        r["red_pre_" + tag] = reduce_preconditions(g, xh)
        r["sums_" + tag] = reduce(d["conv_in"], d["dpooled"], am, *bnp)
    r["settings"] = wgrad_settings(c, d, r["code"])
    for tag, am, sums in r["settings"]:
        dc = dconv_of(d["conv_in"], d["dpooled"], am, *bnp, sums)
        r["wg_pre_" + tag] = wgrad_preconditions(x, dc, pat)
        r["dw_" + tag] = dc.reshape(-1, 64).t() @ pat


_EXACT, _RAW, _ROUNDED = {}, {}, {}


def exact_reference(name):
    """Inputs ("in"), float64 results and precondition figures of the exact tier of one case."""
    if name not in _EXACT:
        c = BY_NAME[name]
        d = exact_inputs(c)
        r = {"in": d}
        pat = patches(d["x"])
        r["conv"] = conv(d["x"], d["w"], pat)
        r["fwd_pre"] = forward_preconditions(r["conv"])
        _backward_reference(c, d, r, pat, d["x"])
        _EXACT[name] = r
    return _EXACT[name]


def raw_reference(name):
    """The same with the clip read through a StemSrcU8: materialize(...) first, then the reference."""
    if name not in _RAW:
        c = BY_NAME[name]
        d = dict(exact_reference(name)["in"])
        raw = raw_inputs(c)
        N, Tin, Hin, Win, Tout, Hc, Wc = raw["dims"]
        x = materialize(raw["frames"], raw["lut"], raw["y1"], raw["x1"], raw["flip"], raw["src_frame"], Tout, Hc, Wc)
        r = {"in": d, "raw": raw, "x": x}
        pat = patches(x)
        r["conv"] = conv(x, d["w"], pat)
        r["fwd_pre"] = forward_preconditions(r["conv"])
        _backward_reference(c, d, r, pat, x)
        _RAW[name] = r
    return _RAW[name]


def rounded_reference(name):
    """Inputs, float64 results and the bound magnitudes of the rounded tier of one small case."""
    if name not in _ROUNDED:
        c = BY_NAME[name]
        d = rounded_inputs(c)
        bnp = bn_args(d)
        r = {"in": d}
        pat = patches(d["x"])
        r["conv"], r["conv_abs"] = conv(d["x"], d["w"], pat), conv_abs(d["x"], d["w"], pat)
        r["pooled"], r["code"], r["y"] = pool(d["conv_in"], *bnp)
        xh, ypre = bn(d["conv_in"], *bnp)
        r["pool_mag"] = (xh * _c(d["gamma"])).abs() + _c(d["beta"]).abs()         # per conv pixel: |(v - mu) is gamma| + |beta|
        r["violations"] = relu_margin_violations(d["conv_in"], *bnp)
        g = gather_g(d["conv_in"], d["dpooled"], r["code"], *bnp)
        r["sums"] = reduce(d["conv_in"], d["dpooled"], r["code"], *bnp)
        r["sums_mag"] = torch.cat([g.abs().sum((0, 1, 2)), (g * xh).abs().sum((0, 1, 2))])
        cnt = float(geom(c)["cnt"])
        dc = dconv_of(d["conv_in"], d["dpooled"], r["code"], *bnp, r["sums"])
        r["dw"] = dc.reshape(-1, 64).t() @ pat
        gi = (_c(d["gamma"]) * _c(d["invstd"])).abs()
        mg, mgx = (r["sums"][:64] / cnt).view(1, 1, 1, 64), (r["sums"][64:] / cnt).view(1, 1, 1, 64)
        form = 8 * U * gi * (g.abs() + mg.abs() + xh.abs() * mgx.abs())            # forming dconv in fp32
        r["dw_form"] = form.reshape(-1, 64).t() @ pat.abs()
        r["dw_mag"] = dc.reshape(-1, 64).abs().t() @ pat.abs()
        r["dw_P"] = contributing_pixels((c.N, c.T, c.H, c.W))
        _ROUNDED[name] = r
    return _ROUNDED[name]
