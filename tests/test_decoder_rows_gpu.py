"""The decoder kernels that index rows through a SegDesc (the ragged stage layout and the compact "ends" layout of
csrc/sbl_common.h), one by one, against the plain numpy references of tests/decoder_rows_reference.py at the edges of the
segment tables and of the launch geometry: embedding + positional encoding (three forward entries, two gradients), the
cross-direction fusion and its adjoint, gather-last, the stage tail, arg-max / select, and the add + LayerNorm launches
that come in pairs, on the compact rows, or fused with the fusion.

Every test drives the C ABI directly (ops.call) with tensors it allocates itself; every output buffer is pre-filled with NaN
(token buffers with a sentinel), so an element the kernel does not write fails the comparison.  None of these kernels
depends on the matmul precision, so the module pins "f32".

Comparisons are of three kinds (U = 2^-24):
  * exact(): the result is one rounded fp32 operation of the inputs (an add, a product, 2 * x + y), a copy, or a sum of
    small integers: it must EQUAL the reference bit for bit;
  * check() against float64 with a bound counted from the kernel's path (each test's docstring has the count); the
    LayerNorm bounds are the error model of tests/ln_reference.py, derived in test_norm_elementwise_gpu.py;
  * token buffers: equal to the reference's first maximal index, everything but column step + 1 untouched.
check() prints the worst error / bound ratio of every comparison; the worst ratio measured on an MI355X is recorded in
each docstring ("measured").

The shapes (D = 512): Edge (1,), Small (1, 2, 3) and Full 1..16 (all 16 descriptor slots) with B = 3; Stage 1..16 with B = 32
(4352 rows: the one-thread-per-float kernels go through their grid-stride loop twice); Wide (16,) * 8 with B = 129 (16512
rows: the float4 kernels do).  shape() asserts those facts with the host code's arithmetic.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import decoder_rows_reference as R
from conftest import maxdiff
from ln_reference import LN_EPS, keep_scale, ln_bwd_ref, ln_fwd_ref, ln_geometry
from sbl_for_multilingual_lip_reading_amd import detfill

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
D = 512
V = 58
SEED = 0x1234ABCD5
SENTINEL = -7

SHAPES = {"edge": (R.EDGE, 3), "small": (R.SMALL, 3), "full": (R.FULL, 3), "stage": (R.FULL, R.STAGE_B), "wide": (R.WIDE, R.WIDE_B)}
# name -> (rows, trips of a one-thread-per-float kernel, trips of a float4 kernel, compact ends rows)
SHAPE_FACTS = {"edge": (3, 1, 1, 3), "small": (18, 1, 1, 15), "full": (408, 1, 1, 93), "stage": (4352, 2, 1, 992), "wide": (16512, 5, 2, 2064)}


@pytest.fixture(scope="module", autouse=True)
def ops():
    from sbl_for_multilingual_lip_reading_amd import _lib, ops as _ops
    _lib.load()
    assert torch.cuda.is_available()
    prev = _ops.get_matmul_precision()
    _ops.set_matmul_precision("f32")
    yield _ops
    _ops.set_matmul_precision(prev)


# --------------------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=None)
def _u_cached(name, shape):
    return detfill.uniform(name, shape)


def u(name, shape):
    """detfill uniform in [-1, 1), float32; computed once per (name, shape) and never written to."""
    return _u_cached(name, tuple(int(s) for s in shape))


def ints(name, shape, k):
    return np.rint(u(name, shape) * np.float32(k)).astype(np.float32)


def dev(a, dtype=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.copy()).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def f64(a):
    return np.asarray(a, dtype=np.float64)


def P(t):
    return None if t is None else t.data_ptr()


def S():
    return torch.cuda.current_stream().cuda_stream


def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def carr(seg_L):
    return (ctypes.c_int * len(seg_L))(*seg_L), len(seg_L)


def seed_dev():
    return torch.tensor([SEED], dtype=torch.int64, device=DEV)


def check(what, got, ref, bound):
    """|got - ref| <= bound elementwise (bound == 0: exact).  Prints and returns the worst error / bound ratio."""
    got, ref = f64(host(got) if hasattr(got, "detach") else got), f64(ref)
    bound = np.broadcast_to(f64(bound), ref.shape)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), what + ": non-finite output"
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    worst = float(ratio.max()) if ratio.size else 0.0
    print("%-52s worst err/bound %.3f  (max err %.3e)" % (what, worst, float(err.max()) if err.size else 0.0))
    assert worst <= 1.0, "%s: err/bound %.3f at %s" % (what, worst, np.unravel_index(int(ratio.argmax()), ratio.shape))
    return worst


def exact(what, got, ref):
    got = host(got) if hasattr(got, "detach") else np.asarray(got)
    ref = np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = int(np.count_nonzero(got != ref))
    assert bad == 0, "%s: %d of %d elements differ (max %.3e)" % (what, bad, ref.size, maxdiff(got, ref))


def shape(name):
    """(seg_L, B, rows) of a named shape, its geometry facts asserted with the host code's arithmetic."""
    seg_L, B = SHAPES[name]
    rows = R.n_rows(B, seg_L)
    assert (rows, R.ew_passes(rows * D), R.ew_passes(rows * D // 4), len(R.ends_full_rows(B, seg_L))) == SHAPE_FACTS[name]
    assert 1 <= len(seg_L) <= 16
    return seg_L, B, rows


def keep_mask(ops, n, p, seed, offset):
    """The keep mask of sbl_dropout over n elements at (seed, offset), recovered by running it over ones."""
    ones = torch.ones(n, device=DEV)
    out = nan(n)
    ops.call("sbl_dropout", P(ones), P(out), n, p, P(seed), offset, S())
    o = host(out)
    assert np.all((o == 0) | (o == keep_scale(p)))
    return o != 0


def tokens(name, B, ldt, Vc=V):
    """int64 (B, ldt) ids in [0, Vc)."""
    return np.minimum(((f64(u(name, (B, ldt))) + 1) * 0.5 * Vc).astype(np.int64), Vc - 1)


# --------------------------------------------------------------------------- embedding + positional encoding, forward
@pytest.mark.parametrize("name", ["edge", "small", "full", "wide"])
def test_embed_pe_fwd(ops, name):
    """sbl_embed_pe_seg_fwd and sbl_embed_pe_drop2_fwd: out[row (s, b, l)] = emb[tok[b, l]] + pe[l] is ONE fp32 add, so it
    must equal numpy's fp32 sum bit for bit; the token rows are 3 wider than the longest prefix (ldt) and the two
    directions read different buffers.  With dropout 0.1 the mask of direction d is sbl_dropout's at (seed, offset_d)
    over the stage's rows * 512 elements (recovered by running sbl_dropout over ones), and the output must EQUAL
    (emb + pe) * scale where it keeps (one more fp32 product) and 0 elsewhere.  Wide takes the float4 grid-stride loop
    into its second trip."""
    seg_L, B, rows = shape(name)
    arr, ns = carr(seg_L)
    ldt = max(seg_L) + 3
    emb, pe = u("dr.emb", (V, D)), u("dr.pe", (max(seg_L) + 1, D))
    tok = [tokens("dr.tok%d" % d, B, ldt) for d in (0, 1)]
    assert B * ldt < 4 or not np.array_equal(tok[0], tok[1])
    ref = [R.embed_pe32(emb, pe, *R.embed_index(tok[d], B, seg_L, V)) for d in (0, 1)]
    embd, ped, tokd = dev(emb), dev(pe), [dev(t) for t in tok]
    for d in (0, 1):
        out = nan(rows, D)
        ops.call("sbl_embed_pe_seg_fwd", P(tokd[d]), ldt, P(embd), P(ped), P(out), B, arr, ns, D, V, S())
        exact("embed_pe_seg_fwd[%s] dir %d" % (name, d), out, ref[d])
    seed = seed_dev()
    for p in (0.0, 0.1):
        outs = [nan(rows, D), nan(rows, D)]
        ops.call("sbl_embed_pe_drop2_fwd", P(tokd[0]), P(tokd[1]), ldt, P(embd), P(ped), P(outs[0]), P(outs[1]), B, arr, ns, D, V, p,
                 P(seed) if p else None, 40, 41, S())
        masks = []
        for d in (0, 1):
            want = ref[d]
            if p:
                masks.append(keep_mask(ops, rows * D, p, seed, 40 + d).reshape(rows, D))
                want = np.where(masks[d], ref[d] * keep_scale(p), np.float32(0))
            exact("embed_pe_drop2_fwd[%s] p=%g dir %d" % (name, p, d), outs[d], want)
        if p:
            assert 0.5 * p < np.mean(masks[0] != masks[1]) < 3 * p


@pytest.mark.parametrize("B,L,pos0", [(3, 1, 0), (3, 5, 0), (3, 5, 2), (1032, 16, 3)])
def test_embed_scale_pe_fwd(ops, B, L, pos0):
    """sbl_embed_scale_pe_fwd: out[b * L + l] = emb[tok[b, pos0 + l]] * sqrt(512) + pe[pos0 + l].  The compiler may emit a
    rounded product followed by an add, or one fused multiply-add; both are computed exactly on the host (fma32) and each
    element must equal one of them (the printout counts, among the elements where the two differ, how many took which).
    (1032, 16) is 16512 rows: the float4 loop's second trip; pos0 = 3 shifts both the token column and the PE row.
    measured: all of the elements where the forms differ (2,171,293 of 8,454,144 in the largest case) took the fused form."""
    rows = B * L
    assert R.ew_passes(rows * D // 4) == (2 if rows == 16512 else 1)
    scale = np.float32(np.sqrt(512.0))
    ldt = pos0 + L + 3
    emb, pe = u("dr.emb", (V, D)), u("dr.pe2", (pos0 + L, D))
    tok = tokens("dr.stok", B, ldt)
    two, one = R.embed_scale_pe32(emb, pe, *R.embed_index_flat(tok, B, L, V, pos0), scale)
    out = nan(rows, D)
    embd, ped, tokd = dev(emb), dev(pe), dev(tok)
    ops.call("sbl_embed_scale_pe_fwd", P(tokd), ldt, P(embd), P(ped), P(out), B, L, D, V, float(scale), pos0, S())
    got = host(out)
    differ = two != one
    print("embed_scale_pe_fwd[%d x %d pos0=%d]: %d elements where the forms differ: %d fused, %d product-then-add"
          % (B, L, pos0, differ.sum(), (differ & (got == one)).sum(), (differ & (got == two)).sum()))
    bad = int(np.count_nonzero((got != two) & (got != one)))
    assert bad == 0, "embed_scale_pe_fwd: %d of %d elements are neither form" % (bad, got.size)


def test_embed_fwd_clamps_ids(ops):
    """Ids -3 and V + 5 read vocabulary rows 0 and V - 1 in all three forward entries (the clamp is in the kernels)."""
    seg_L, B, rows = shape("small")
    arr, ns = carr(seg_L)
    ldt = max(seg_L) + 3
    emb, pe = u("dr.emb", (V, D)), u("dr.pe", (max(seg_L) + 1, D))
    tok = tokens("dr.tok0", B, ldt)
    tok[0, :] = -3
    tok[1, :] = V + 5
    t, pos = R.embed_index(tok, B, seg_L, V)
    ref = R.embed_pe32(emb, pe, t, pos)
    seg, b, l, _ = R.stage_rows(B, seg_L)
    assert np.array_equal(ref[b == 0], emb[0] + pe[l[b == 0]]) and np.array_equal(ref[b == 1], emb[V - 1] + pe[l[b == 1]])
    embd, ped, tokd = dev(emb), dev(pe), dev(tok)
    out = nan(rows, D)
    ops.call("sbl_embed_pe_seg_fwd", P(tokd), ldt, P(embd), P(ped), P(out), B, arr, ns, D, V, S())
    exact("embed_pe_seg_fwd clamp", out, ref)
    outs = [nan(rows, D), nan(rows, D)]
    ops.call("sbl_embed_pe_drop2_fwd", P(tokd), P(tokd), ldt, P(embd), P(ped), P(outs[0]), P(outs[1]), B, arr, ns, D, V, 0.0, None, 0, 0, S())
    exact("embed_pe_drop2_fwd clamp 0", outs[0], ref)
    exact("embed_pe_drop2_fwd clamp 1", outs[1], ref)
    L = 3
    t, pos = R.embed_index_flat(tok, B, L, V)
    assert set(t[:L]) == {0} and set(t[L:2 * L]) == {V - 1}
    out = nan(B * L, D)
    ops.call("sbl_embed_scale_pe_fwd", P(tokd), ldt, P(embd), P(ped), P(out), B, L, D, V, 2.0, 0, S())
    exact("embed_scale_pe_fwd clamp", out, np.float32(2) * emb[t] + pe[pos])          # a power-of-two scale: both forms agree


# --------------------------------------------------------------------------- embedding, backward
def token_pattern(pattern, B, ldt):
    if pattern == "same":            # every row adds onto vocabulary row 7: maximal contention of the float atomics
        return np.full((B, ldt), 7, np.int64)
    return (np.arange(B)[:, None] * ldt + np.arange(ldt)[None, :]) % V          # distinct as far as V allows


def embed_bwd_checks(tag, run, t, rows, scale, pow2):
    """Shared by the two gradient entries.  run(dy, preset) -> demb (device)."""
    dy, pre = ints("dr.edy", (rows, D), 3), ints("dr.epre", (V, D), 9)
    ref, _, cnt = R.embed_grad64(dy, t, V, pow2)
    assert np.abs(ref).max() + 9 < 2 ** 20          # every partial sum is an integer multiple of pow2 far inside 24 bits
    exact(tag + " integer dy", run(dy, pre, pow2), (f64(pre) + ref).astype(np.float32))
    dy, pre = u("dr.edy", (rows, D)), u("dr.epre", (V, D))
    ref, mag, cnt = R.embed_grad64(dy, t, V, scale)
    depth = cnt + (0 if scale == 1.0 else 1)
    depth = np.where(cnt > 0, depth, 0)[:, None]
    return check(tag + " random dy", run(dy, pre, scale), f64(pre) + ref, depth * U / (1 - depth * U) * (np.abs(f64(pre)) + mag))


@pytest.mark.parametrize("pattern", ["same", "distinct"])
@pytest.mark.parametrize("name", ["small", "full", "stage"])
def test_embed_seg_bwd(ops, name, pattern):
    """sbl_embed_seg_bwd: demb[tok[b, l]] += dy[row (s, b, l)], one float atomic per element onto the caller's preset.
    Integer dy in -3..3 onto an integer preset: every partial sum is exact in any order, so demb must EQUAL preset + the
    integer scatter sum.  Random dy: the n rows that hit one vocabulary row are n sequential fp32 additions in some
    order, a term passes through at most n roundings: n * U / (1 - n * U) * (|preset| + sum|terms|); a vocabulary row
    nothing hits has bound 0 and must come back bit-identical.  Stage (2,228,224 elements) takes the loop into its second
    trip; 'same' puts all rows onto one vocabulary row (depth 4352 there).
    measured: worst err/bound 0.61."""
    seg_L, B, rows = shape(name)
    arr, ns = carr(seg_L)
    ldt = max(seg_L) + 3
    tok = token_pattern(pattern, B, ldt)
    tokd = dev(tok)
    t, _ = R.embed_index(tok, B, seg_L, V)
    if pattern == "same":
        assert np.bincount(t, minlength=V)[7] == rows
    elif rows <= V:
        assert len(set(t[:B * seg_L[0]].tolist())) == B * seg_L[0]

    def run(dy, pre, scale):
        demb, dyd = dev(pre), dev(dy)
        ops.call("sbl_embed_seg_bwd", P(tokd), ldt, P(dyd), P(demb), B, arr, ns, D, V, S())
        return demb
    embed_bwd_checks("embed_seg_bwd[%s %s]" % (name, pattern), run, t, rows, 1.0, 1.0)


@pytest.mark.parametrize("pattern", ["same", "distinct"])
@pytest.mark.parametrize("B,L", [(3, 5), (272, 16)])
def test_embed_scale_bwd(ops, B, L, pattern):
    """sbl_embed_scale_bwd: demb[tok[b, l]] += dy[b * L + l] * scale.  Integer dy with scale = 1/4: every term and partial
    sum is a multiple of 1/4 far inside 24 bits, so demb must EQUAL the integer-valued preset + the exact sum.  Random dy
    with scale = sqrt(512): the product adds one rounding per term: depth n + 1.  (272, 16) = 4352 rows: second trip.
    measured: worst err/bound 0.95."""
    rows = B * L
    assert R.ew_passes(rows * D) == (2 if rows == 4352 else 1)
    ldt = L + 3
    tok = token_pattern(pattern, B, ldt)
    tokd = dev(tok)
    t, _ = R.embed_index_flat(tok, B, L, V)

    def run(dy, pre, scale):
        demb, dyd = dev(pre), dev(dy)
        ops.call("sbl_embed_scale_bwd", P(tokd), ldt, P(dyd), P(demb), B, L, D, V, float(scale), S())
        return demb
    embed_bwd_checks("embed_scale_bwd[%dx%d %s]" % (B, L, pattern), run, t, rows, np.float32(np.sqrt(512.0)), 0.25)


# --------------------------------------------------------------------------- fusion, gather-last
@pytest.mark.parametrize("name", ["edge", "small", "full", "wide"])
def test_fusion_seg(ops, name):
    """sbl_fusion_seg_fwd: A' = A + flip(B), B' = 2 B + flip(A); sbl_fusion_seg_bwd: dA = dA' + flip(dB'), dB = flip(dA') +
    2 dB'.  The factor 2 is exact and each output is one rounded add (a contraction of 2 * y + x into a fused
    multiply-add gives the same bits), so all four outputs must EQUAL numpy's fp32 evaluation.  Adjoint identity between
    the two entries in float64 from the kernels' own outputs: <fwd(a, b), (wa, wb)> = <(a, b), bwd(wa, wb)> up to the one
    rounding of every output element, U * (sum|A' wa| + sum|B' wb| + sum|dA a| + sum|dB b|).  Wide: the float4 loop's
    second trip, where the flipped row of an element lies in the other trip's half for some rows.
    measured: worst err/bound 0.003 (adjoint identity)."""
    seg_L, B, rows = shape(name)
    arr, ns = carr(seg_L)
    flip = R.flip_rows(B, seg_L)
    a, b, wa, wb = (u("dr.f" + k, (rows, D)) for k in ("a", "b", "wa", "wb"))
    ad, bd, wad, wbd = dev(a), dev(b), dev(wa), dev(wb)
    a2, b2, da, db = nan(rows, D), nan(rows, D), nan(rows, D), nan(rows, D)
    ops.call("sbl_fusion_seg_fwd", P(ad), P(bd), P(a2), P(b2), B, arr, ns, D, S())
    ops.call("sbl_fusion_seg_bwd", P(wad), P(wbd), P(da), P(db), B, arr, ns, D, S())
    r0, r1 = R.fusion32(a, b, flip)
    exact("fusion_seg_fwd[%s] A'" % name, a2, r0)
    exact("fusion_seg_fwd[%s] B'" % name, b2, r1)
    g0, g1 = R.fusion_bwd32(wa, wb, flip)
    exact("fusion_seg_bwd[%s] dA" % name, da, g0)
    exact("fusion_seg_bwd[%s] dB" % name, db, g1)
    ha2, hb2, hda, hdb = f64(host(a2)), f64(host(b2)), f64(host(da)), f64(host(db))
    lhs = (ha2 * wa).sum() + (hb2 * wb).sum()
    rhs = (hda * a).sum() + (hdb * b).sum()
    bound = U * (np.abs(ha2 * wa).sum() + np.abs(hb2 * wb).sum() + np.abs(hda * a).sum() + np.abs(hdb * b).sum())
    check("fusion adjoint identity[%s]" % name, np.array([lhs]), np.array([rhs]), np.array([bound]))


@pytest.mark.parametrize("name", ["edge", "small", "full", "stage"])
def test_gather_last(ops, name):
    """sbl_gather_last_fwd: out[s * B + b] = x[last row of sequence (s, b)], a copy: exact.  sbl_gather_last_bwd over a
    NaN-filled dx: the nseg * B gradient rows land on those rows and EVERY other row is written zero."""
    seg_L, B, rows = shape(name)
    arr, ns = carr(seg_L)
    last = R.last_rows(B, seg_L)
    assert len(last) == ns * B
    x, dy = u("dr.gx", (rows, D)), u("dr.gdy", (ns * B, D))
    dy = np.where(dy == 0, np.float32(0.5), dy)
    xd, dyd = dev(x), dev(dy)
    out, dx = nan(ns * B, D), nan(rows, D)
    ops.call("sbl_gather_last_fwd", P(xd), P(out), B, arr, ns, D, S())
    exact("gather_last_fwd[%s]" % name, out, R.gather_last(x, last))
    ops.call("sbl_gather_last_bwd", P(dyd), P(dx), B, arr, ns, D, S())
    want = R.gather_last_bwd(dy, last, rows)
    assert np.count_nonzero(want.any(1)) == ns * B
    exact("gather_last_bwd[%s]" % name, dx, want)


# --------------------------------------------------------------------------- stage tail
TAIL_SEGS = {1: (1,), 2: (3, 1), 3: (1, 2, 3), 4: (2, 1, 4, 3)}
TAIL_B = 3


def tail_run(ops, seg_L, Vc, ya, yb, w, ldy, step, write_tok):
    arr, ns = carr(seg_L)
    nrows = ns * TAIL_B
    ldp = Vc + 3
    yad, ybd, wd = dev(ya), dev(yb), [dev(x) for x in w]
    last = [nan(nrows, D), nan(nrows, D)]
    pred = [nan(nrows, ldp), nan(nrows, ldp)]
    ys = [torch.full((TAIL_B, ldy), SENTINEL, dtype=torch.long, device=DEV) for _ in (0, 1)]
    ops.call("sbl_decoder_tail_fwd", P(yad), P(ybd), P(wd[0]), P(wd[1]), P(last[0]), P(last[1]), P(pred[0]), P(pred[1]), ldp,
             P(ys[0]), P(ys[1]), ldy, step, write_tok, TAIL_B, arr, ns, D, Vc, S())
    return [host(x) for x in last], [host(x) for x in pred], [host(x) for x in ys]


def tail_checks(tag, seg_L, Vc, ya, yb, w, last, pred, tie=None):
    """last exact, logits within the bound, pad columns untouched; returns the float64 logits of both directions."""
    ns = len(seg_L)
    first, lastr = R.first_rows(TAIL_B, seg_L), R.last_rows(TAIL_B, seg_L)
    l32, l64 = R.tail_last32(ya, yb, first, lastr), R.tail_last64(ya, yb, first, lastr)
    refs, worst = [], 0.0
    for d in (0, 1):
        exact(tag + " last%d" % d, last[d], l32[d])
        lg, mag = R.tail_logits64(l64[d], w[d])
        if tie:
            lg[:, tie[1]] = lg[:, tie[0]]          # identical weight rows: the same number, whatever order BLAS summed them in
        worst = max(worst, check(tag + " pred%d" % d, pred[d][:, :Vc], lg, 15 * U / (1 - 15 * U) * mag))
        assert np.isnan(pred[d][:, Vc:]).all(), tag + ": pad columns of pred written"
        refs.append((lg, 15 * U / (1 - 15 * U) * mag))
    return refs


@pytest.mark.parametrize("Vc", [1, 17, 58, 64])
@pytest.mark.parametrize("nseg", [1, 2, 3, 4])
def test_decoder_tail(ops, nseg, Vc):
    """sbl_decoder_tail_fwd with B = 3 and 1..4 segments: nseg * B = 3, 6, 9, 12 rows, so the last workgroup of four rows holds
    3, 2, 1 clamped rows or none (3 < 4: the only workgroup is partial); segment lists with a length-1 segment in every
    place (a direction's last row IS the other's first row), V = 1, 17 (one partly filled wavefront of classes), 58, 64,
    ldp = V + 3 with the pad columns still NaN afterwards.
    last_d = kf * own[L-1] + other[0] (kf = 1, 2): the product is exact, one rounded add: EQUAL to numpy's fp32.
    Logits against float64 from the unrounded last: the rounding already in `last` contributes U * sum|last_k w_k|; a lane's
    chain is one product and 7 fused multiply-adds (8 roundings on its first term), the transposing butterfly adds 6 levels:
    a term passes through at most 14 more, so (1 + 14) * U / (1 - 15 U) * sum_k |last_k| |w_k|.
    Tokens: ys_d[b, step + 1] = first maximal index of the LAST segment's row b (the reference's margins are asserted to
    exceed twice the bound, so the kernel's own logits have the same arg-max), all other entries keep the sentinel;
    step + 1 = ldy - 1 for odd nseg; write_tok = 0 writes none.
    measured: worst err/bound 0.02 (logits)."""
    seg_L = TAIL_SEGS[nseg]
    nrows = nseg * TAIL_B
    assert nrows % 4 == {1: 3, 2: 2, 3: 1, 4: 0}[nseg] and R.cdiv(nrows, 4) == {1: 1, 2: 2, 3: 3, 4: 3}[nseg]
    rows = R.n_rows(TAIL_B, seg_L)
    ya, yb = u("dr.tya", (rows, D)), u("dr.tyb", (rows, D))
    w = [u("dr.tw%d" % d, (Vc, D)) * np.float32(0.1) for d in (0, 1)]
    step = 5
    ldy = step + 2 if nseg % 2 else step + 4
    tag = "tail[nseg=%d V=%d]" % (nseg, Vc)
    last, pred, ys = tail_run(ops, seg_L, Vc, ya, yb, w, ldy, step, 1)
    refs = tail_checks(tag, seg_L, Vc, ya, yb, w, last, pred)
    init = np.full((TAIL_B, ldy), SENTINEL, np.int64)
    for d in (0, 1):
        lg, bound = (x[(nseg - 1) * TAIL_B:] for x in refs[d])
        if Vc > 1:
            top = np.sort(lg, 1)
            assert np.all(top[:, -1] - top[:, -2] > 2 * bound.max(1)), tag + ": reference margin inside the bound"
        exact(tag + " ys%d" % d, ys[d], R.tail_tokens(init, refs[d][0], TAIL_B, nseg, step))
        exact(tag + " ys%d own logits" % d, ys[d][:, step + 1], R.first_argmax(pred[d][(nseg - 1) * TAIL_B:, :Vc]))
    last2, pred2, ys2 = tail_run(ops, seg_L, Vc, ya, yb, w, ldy, step, 0)
    for d in (0, 1):
        exact(tag + " write_tok=0 ys%d" % d, ys2[d], init)
        exact(tag + " write_tok=0 last%d" % d, last2[d], last[d])
        exact(tag + " write_tok=0 pred%d" % d, pred2[d][:, :Vc], pred[d][:, :Vc])


@pytest.mark.parametrize("Vc", [58, 64])
@pytest.mark.parametrize("tie", [(15, 16), (10, 40)])
def test_decoder_tail_ties(ops, tie, Vc):
    """Planted exact ties for the maximum inside the tail's own arg-max: classes 15 / 16 (the last class of wavefront 0 and
    the first of wavefront 1) and 10 / 40 (far apart) get IDENTICAL weight rows (0.05 in every column) and the inputs a
    common offset of 0.5, so the two logits are the same sum of the same products in the same order - bit-equal, asserted -
    and exceed every other class by more than 10 (asserted on the reference).  The token must be the lower index.
    measured: worst err/bound 0.07 (logits, same bound as test_decoder_tail)."""
    seg_L = TAIL_SEGS[3]
    rows = R.n_rows(TAIL_B, seg_L)
    ya, yb = u("dr.tya", (rows, D)) + np.float32(0.5), u("dr.tyb", (rows, D)) + np.float32(0.5)
    w = [(u("dr.tw%d" % d, (Vc, D)) * np.float32(0.1)).copy() for d in (0, 1)]
    for d in (0, 1):
        w[d][tie[0]] = w[d][tie[1]] = np.float32(0.05)
    step, ldy = 0, 3
    tag = "tail ties[%d/%d V=%d]" % (tie[0], tie[1], Vc)
    last, pred, ys = tail_run(ops, seg_L, Vc, ya, yb, w, ldy, step, 1)
    refs = tail_checks(tag, seg_L, Vc, ya, yb, w, last, pred, tie)
    for d in (0, 1):
        lg = refs[d][0]
        others = np.delete(lg, list(tie), 1)
        assert np.all(lg[:, tie[0]] == lg[:, tie[1]]) and np.all(lg[:, tie[0]] - others.max(1) > 10)
        exact(tag + " bit-equal logits %d" % d, pred[d][:, tie[0]], pred[d][:, tie[1]])
        want = np.full((TAIL_B, ldy), SENTINEL, np.int64)
        want[:, step + 1] = tie[0]
        exact(tag + " ys%d" % d, ys[d], want)
        exact(tag + " ys%d vs reference" % d, ys[d], R.tail_tokens(np.full((TAIL_B, ldy), SENTINEL, np.int64), lg, TAIL_B, len(seg_L), step))


# --------------------------------------------------------------------------- arg-max / select
def argmax_cases(Vc):
    """(name, tied classes or None) that fit Vc classes; a tie is planted at 2.0, above every other logit."""
    cases = [("none", None), ("-inf row", "inf")]
    if Vc > 1:
        cases.append(("first / last", (0, Vc - 1)))
    if Vc > 6:
        cases.append(("neighbouring lanes", (5, 6)))
    if Vc > 35:
        cases.append(("lanes 3 / 35", (3, 35)))
    if Vc > 64:
        cases.append(("same lane, c / c + 64", (0, 64)))
    if Vc > 198:
        cases.append(("same lane, three trips", (70, 134, 198)))
        cases.append(("same lane 3 / 67 against lane 4", (67, 3, 4)))
    return cases


@pytest.mark.parametrize("Vc", [1, 58, 64, 65, 200])
@pytest.mark.parametrize("B", [1, 4, 5])
def test_argmax_select(ops, B, Vc):
    """sbl_argmax_select: ys[b, step + 1] = coin ? first maximal index of pred[b, :V] : gold[b, step].  One wavefront per
    row, four rows per workgroup (B = 1, 4, 5: a partial, a full, a full and a partial workgroup); lane c takes classes c,
    c + 64, ... (V = 1, 58, 64, 65, 200: one lane, a partly filled trip, exactly one trip, one class in the second trip,
    four trips).  ldp = V + 5 with +inf in the pad columns (a kernel that read them would pick them), ldg and ldy wider
    than the data.  Planted exact ties, value 2.0 above all other logits: first / last class, neighbouring lanes, lanes 3 /
    35, the same lane in two and three trips (c, c + 64, c + 128), a same-lane pair against its neighbour; a row of all -inf
    gives 0.  Each case runs at its own step with the coin from the device array (1, then 0: the gold token), then with
    gold = NULL / always arg-max and pred = NULL / always gold.  Only column step + 1 may change."""
    ldp, ldy, ldg = Vc + 5, 12, 14
    gold = tokens("dr.gold", B, ldg, max(Vc, 2))
    goldd = dev(gold)
    for step, (name, tie) in enumerate(argmax_cases(Vc)):
        pred = np.full((B, ldp), np.inf, np.float32)
        pred[:, :Vc] = u("dr.am%d" % step, (B, Vc))
        if tie == "inf":
            pred[:, :Vc] = -np.inf
        elif tie:
            pred[:, list(tie)] = np.float32(2)
        predd = dev(pred)
        init = np.full((B, ldy), SENTINEL, np.int64)
        tag = "argmax_select[B=%d V=%d %s]" % (B, Vc, name)
        for own in (1, 0):
            coins = np.full((ldy,), 1 - own, np.int32)
            coins[step] = own
            ys, coinsd = dev(init), dev(coins)
            ops.call("sbl_argmax_select", P(predd), ldp, P(goldd), ldg, P(ys), ldy, step, 1 - own, P(coinsd), B, Vc, S())
            want = R.argmax_select(pred[:, :Vc], gold, init, step, own)
            if own and tie:
                assert np.all(want[:, step + 1] == (0 if tie == "inf" else min(tie)))
            exact(tag + " coin %d" % own, ys, want)
        ys = dev(init)
        ops.call("sbl_argmax_select", P(predd), ldp, None, 0, P(ys), ldy, step, 1, None, B, Vc, S())
        exact(tag + " gold NULL", ys, R.argmax_select(pred[:, :Vc], gold, init, step, 1))
        ys = dev(init)
        ops.call("sbl_argmax_select", None, ldp, P(goldd), ldg, P(ys), ldy, step, 0, None, B, Vc, S())
        exact(tag + " pred NULL", ys, R.argmax_select(pred[:, :Vc], gold, init, step, 0))


# --------------------------------------------------------------------------- add + LayerNorm: pairs, ends, fused fusion
def ln_dir_inputs(M, d):
    """Direction d's operands: different x, residual, gamma and beta per direction."""
    x = u("dr.lnx%d" % d, (M, D)) * np.float32(2)
    res = u("dr.lnr%d" % d, (M, D))
    gamma = np.float32(1) + np.float32(0.2) * u("dr.lng%d" % d, (D,))
    beta = np.float32(0.1) * u("dr.lnb%d" % d, (D,))
    return x, res, gamma, beta


def ln2_call(ops, entry, ins, with_res, M, tail_args):
    """Run a two-direction forward entry; returns per-direction (y, mean, rstd) device tensors."""
    xs, rs, gs, bs = ([dev(ins[d][k]) for d in (0, 1)] for k in range(4))
    y, mean, rstd = [nan(M, D), nan(M, D)], [nan(M), nan(M)], [nan(M), nan(M)]
    ops.call(entry, P(xs[0]), P(xs[1]), P(rs[0]) if with_res else None, P(rs[1]) if with_res else None, P(gs[0]), P(gs[1]), P(bs[0]), P(bs[1]),
             P(y[0]), P(y[1]), P(mean[0]), P(mean[1]), P(rstd[0]), P(rstd[1]), *tail_args)
    return y, mean, rstd


def ln_fwd_checks(tag, f, y, mean, rstd):
    return (check(tag + "y", y, f["y"], f["e_y"]), check(tag + "mean", mean, f["mean"], f["e_mean"]),
            check(tag + "rstd", rstd, f["rstd"], f["e_rstd"]))


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("with_res", [0, 1])
@pytest.mark.parametrize("M", [1, 5, 4352])
def test_add_layernorm2_fwd(ops, M, with_res, p):
    """sbl_add_layernorm2_fwd: both directions in one launch, each with its own x, residual, gamma, beta and dropout offset,
    against ln_fwd_ref's float64 LayerNorm(x * mask * scale + res) and error model (tests/ln_reference.py; derivation in
    test_norm_elementwise_gpu.py::test_add_layernorm_fwd_bwd).  M = 1 (one wavefront of the only workgroup), 5 (a second
    workgroup with one row), 4352 (the stage-batched step); residuals present and both NULL; dropout 0.1 with direction d's
    mask recovered from sbl_dropout at (seed, offset_d).
    measured: worst err/bound 0.16 (y), 0.04 (mean), 0.10 (rstd)."""
    assert R.cdiv(M, 4) == {1: 1, 5: 2, 4352: 1088}[M]
    ins = [ln_dir_inputs(M, d) for d in (0, 1)]
    seed = seed_dev()
    y, mean, rstd = ln2_call(ops, "sbl_add_layernorm2_fwd", ins, with_res, M, (M, D, LN_EPS, p, P(seed) if p else None, 70, 71, S()))
    masks = [keep_mask(ops, M * D, p, seed, 70 + d).reshape(M, D) if p else None for d in (0, 1)]
    if p:
        assert not np.array_equal(masks[0], masks[1])
    for d in (0, 1):
        x, res, gamma, beta = ins[d]
        f = ln_fwd_ref(x, res if with_res else None, gamma, beta, masks[d], p)
        ln_fwd_checks("ln2[%d res=%d p=%g] dir %d " % (M, with_res, p, d), f, y[d], mean[d], rstd[d])


def ends_masks(ops, seg_L, B, rows, p, seed, offset):
    """(full-layout mask at the ends rows, compact-index mask) of a compact launch; the two must differ exactly when the
    ends rows are not 0 .. M-1 (Edge: every sequence is one row, the layouts coincide)."""
    er = R.ends_full_rows(B, seg_L)
    full = keep_mask(ops, rows * D, p, seed, offset).reshape(rows, D)
    right, wrong = full[er], full[:len(er)]
    assert np.array_equal(right, wrong) == np.array_equal(er, np.arange(len(er)))
    if not np.array_equal(er, np.arange(len(er))):
        moved = er != np.arange(len(er))
        assert np.mean(right[moved] != wrong[moved]) > p * (1 - p)          # two independent masks differ on 2 p (1 - p)
    return right


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("name", ["edge", "small", "full", "stage"])
def test_add_layernorm2_ends_fwd(ops, name, p):
    """sbl_add_layernorm2_ends_fwd: sbl_add_layernorm2_fwd on the compact rows, where the dropout decision of compact row r
    is the one the FULL-layout launch draws for the full row it stands for.  The full-layout mask is recovered from
    sbl_dropout over ones of B * sum(seg_L) * 512 elements and indexed by the ends rows; the test also asserts that this
    mask differs from the compact-index mask (the first M rows of the same draw) wherever a compact row is not its own full
    row - on Small, Full and Stage; on Edge the two layouts are the same rows - so a kernel that indexed the mask by the
    compact row could not pass.  Same float64 reference and error model as test_add_layernorm2_fwd.
    measured: worst err/bound 0.16 (y), 0.03 (mean), 0.10 (rstd)."""
    seg_L, B, rows = shape(name)
    arr, ns = carr(seg_L)
    M = SHAPE_FACTS[name][3]
    ins = [ln_dir_inputs(M, d) for d in (0, 1)]
    seed = seed_dev()
    y, mean, rstd = ln2_call(ops, "sbl_add_layernorm2_ends_fwd", ins, 1, M, (B, arr, ns, D, LN_EPS, p, P(seed) if p else None, 70, 71, S()))
    for d in (0, 1):
        x, res, gamma, beta = ins[d]
        mask = ends_masks(ops, seg_L, B, rows, p, seed, 70 + d) if p else None
        f = ln_fwd_ref(x, res, gamma, beta, mask, p)
        ln_fwd_checks("ln2_ends[%s p=%g] dir %d " % (name, p, d), f, y[d], mean[d], rstd[d])


def ends_bwd_run(ops, seg_L, B, M, x, res, gamma, mean32, rstd32, dy, pre_g, pre_b, p, seed, offset):
    arr, ns = carr(seg_L)
    dyd, xd, rd, gd, md, sd = dev(dy), dev(x), dev(res), dev(gamma), dev(mean32), dev(rstd32)
    dz, dxd = nan(M, D), (nan(M, D) if p else None)
    dgamma, dbeta = dev(pre_g), dev(pre_b)
    ops.call("sbl_add_layernorm_ends_bwd", P(dyd), P(xd), P(rd), P(gd), P(md), P(sd), P(dz), P(dxd), P(dgamma), P(dbeta), B, arr, ns, D,
             p, P(seed) if p else None, offset, S())
    return dz, dxd, dgamma, dbeta


def ends_forward_stats(ops, seg_L, B, M, ins, p, seed):
    arr, ns = carr(seg_L)
    _, mean, rstd = ln2_call(ops, "sbl_add_layernorm2_ends_fwd", ins, 1, M, (B, arr, ns, D, LN_EPS, p, P(seed) if p else None, 70, 71, S()))
    return [host(m) for m in mean], [host(r) for r in rstd]


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("name", ["edge", "small", "full", "stage"])
def test_add_layernorm_ends_bwd(ops, name, p):
    """sbl_add_layernorm_ends_bwd on the compact rows, from the mean / rstd sbl_add_layernorm2_ends_fwd wrote (held to float64
    in the test above): dz against ln_bwd_ref's float64 gradient and error model with the FULL-layout mask; dx_drop must
    EQUAL dz * mask * scale in fp32 (one product) with that mask; dy is integer valued, so dbeta must EQUAL the integer
    preset + the integer column sums; dgamma as in test_add_layernorm_fwd_bwd with the geometry of the compact M: a term
    passes rows_per_block / 8 per-wave additions, 8 in the block's combine and at most grid float atomics onto the preset:
    depth = 1 + rpb / 8 + 8 + grid.  Both directions (their own operands and offsets).
    measured: worst err/bound 0.24 (dz), 0.17 (dgamma)."""
    seg_L, B, rows = shape(name)
    M = SHAPE_FACTS[name][3]
    rpb, grid = ln_geometry(M)
    assert (rpb, grid) == {"edge": (16, 1), "small": (16, 1), "full": (32, 3), "stage": (32, 31)}[name]
    ins = [ln_dir_inputs(M, d) for d in (0, 1)]
    seed = seed_dev()
    mean, rstd = ends_forward_stats(ops, seg_L, B, M, ins, p, seed)
    dy = ints("dr.lndy", (M, D), 3)
    pre_g, pre_b = u("dr.preg", (D,)), ints("dr.preb", (D,), 9)
    for d in (0, 1):
        x, res, gamma, beta = ins[d]
        mask = ends_masks(ops, seg_L, B, rows, p, seed, 70 + d) if p else None
        dz, dxd, dgamma, dbeta = ends_bwd_run(ops, seg_L, B, M, x, res, gamma, mean[d], rstd[d], dy, pre_g, pre_b, p, seed, 70 + d)
        f = ln_fwd_ref(x, res, gamma, beta, mask, p)
        rdz, e_dz, t, e_t = ln_bwd_ref(dy, f["v"], f["e_v"], gamma, mean[d], rstd[d])
        tag = "ln_ends_bwd[%s p=%g] dir %d " % (name, p, d)
        check(tag + "dz", dz, rdz, e_dz)
        if p:
            exact(tag + "dx_drop", dxd, np.where(mask, host(dz) * keep_scale(p), np.float32(0)))
        exact(tag + "dbeta", dbeta, (f64(pre_b) + f64(dy).sum(0)).astype(np.float32))
        depth = 1 + rpb // 8 + 8 + grid
        check(tag + "dgamma", dgamma, f64(pre_g) + t.sum(0), depth * U * (np.abs(f64(pre_g)) + np.abs(t).sum(0)) + e_t.sum(0))


def test_add_layernorm_ends_bwd_one_hot_rows(ops):
    """Stage's 992 compact rows are 31 blocks of 32: dy is zero except one row r at the block boundaries (0, last row of
    block 0, first row of block 1, M - 2, M - 1; asserted from the recomputed rows-per-block), dgamma / dbeta start at zero,
    dropout 0.1 (so the row's full-layout mask enters xhat): dbeta must equal that row of dy exactly, dgamma its dy * xhat to
    the term's own error, and dz must be exactly zero on every other row.
    measured: worst err/bound 0.82 (dgamma), 0.20 (dz)."""
    name, p, d = "stage", 0.1, 0
    seg_L, B, rows = shape(name)
    M = SHAPE_FACTS[name][3]
    rpb, grid = ln_geometry(M)
    assert grid >= 2 and (grid - 1) * rpb < M
    ins = [ln_dir_inputs(M, k) for k in (0, 1)]
    seed = seed_dev()
    mean, rstd = ends_forward_stats(ops, seg_L, B, M, ins, p, seed)
    x, res, gamma, beta = ins[d]
    mask = ends_masks(ops, seg_L, B, rows, p, seed, 70 + d)
    f = ln_fwd_ref(x, res, gamma, beta, mask, p)
    row, zero = u("dr.onehot", (D,)), np.zeros((D,), np.float32)
    for r in sorted({0, rpb - 1, rpb, M - 2, M - 1}):
        assert (r // rpb == 0) if r < rpb else (r // rpb == 1 if r == rpb else r // rpb == grid - 1)
        dy = np.zeros((M, D), np.float32)
        dy[r] = row
        dz, dxd, dgamma, dbeta = ends_bwd_run(ops, seg_L, B, M, x, res, gamma, mean[d], rstd[d], dy, zero, zero, p, seed, 70 + d)
        rdz, e_dz, t, e_t = ln_bwd_ref(dy, f["v"], f["e_v"], gamma, mean[d], rstd[d])
        assert np.count_nonzero(e_dz[np.arange(M) != r]) == 0
        check("ln_ends one-hot r=%d dz" % r, dz, rdz, e_dz)
        exact("ln_ends one-hot r=%d dx_drop" % r, dxd, np.where(mask, host(dz) * keep_scale(p), np.float32(0)))
        exact("ln_ends one-hot r=%d dbeta" % r, dbeta, row)
        check("ln_ends one-hot r=%d dgamma" % r, dgamma, t[r], e_t[r])


FUSION_SHAPES = {"small": (R.SMALL, 3), "full": (R.FULL, 3), "odd": ((2, 5), 3)}


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("with_res", [0, 1])
@pytest.mark.parametrize("name", ["small", "full", "odd"])
def test_add_layernorm2_fusion_fwd(ops, name, with_res, p):
    """sbl_add_layernorm2_fusion_fwd in float64: A = LayerNorm(dropout(x0) + res0), B = the same of direction 1 (ln_fwd_ref,
    masks recovered per direction), then xn0 = A + flip(B), xn1 = 2 B + flip(A).  The LayerNorm rows carry the model's e_y;
    the fusion adds one rounding of the sum (2 * B is exact): xn0[l] within e_y(A[l]) + e_y(B[L-1-l]) + U |xn0|, xn1[l] within
    2 e_y(B[l]) + e_y(A[L-1-l]) + U |xn1|; mean / rstd per direction as in test_add_layernorm2_fwd.  Rows: 18 (Small), 408
    (Full), 21 (segments (2, 5): 21 % 4 = 1, one wavefront in the last workgroup); with and without residual; dropout 0.25.
    measured: worst err/bound 0.14 (xn0), 0.14 (xn1), 0.03 (mean), 0.11 (rstd)."""
    seg_L, B = FUSION_SHAPES[name]
    rows = R.n_rows(B, seg_L)
    assert rows % 4 == {"small": 2, "full": 0, "odd": 1}[name]
    arr, ns = carr(seg_L)
    flip = R.flip_rows(B, seg_L)
    ins = [ln_dir_inputs(rows, d) for d in (0, 1)]
    seed = seed_dev()
    xn, mean, rstd = ln2_call(ops, "sbl_add_layernorm2_fusion_fwd", ins, with_res, rows,
                              (B, arr, ns, D, LN_EPS, p, P(seed) if p else None, 70, 71, S()))
    f = []
    for d in (0, 1):
        x, res, gamma, beta = ins[d]
        mask = keep_mask(ops, rows * D, p, seed, 70 + d).reshape(rows, D) if p else None
        f.append(ln_fwd_ref(x, res if with_res else None, gamma, beta, mask, p))
    A, Bf = f
    tag = "ln2_fusion[%s res=%d p=%g] " % (name, with_res, p)
    r0, r1 = R.fusion64(A["y"], Bf["y"], flip)
    check(tag + "xn0", xn[0], r0, A["e_y"] + Bf["e_y"][flip] + U * np.abs(r0))
    check(tag + "xn1", xn[1], r1, 2 * Bf["e_y"] + A["e_y"][flip] + U * np.abs(r1))
    for d in (0, 1):
        check(tag + "mean%d" % d, mean[d], f[d]["mean"], f[d]["e_mean"])
        check(tag + "rstd%d" % d, rstd[d], f[d]["rstd"], f[d]["e_rstd"])
