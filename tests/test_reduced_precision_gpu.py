"""The two reduced arithmetics of the tile engine, "bf16x3" and "bf16", held kernel by kernel to what they are defined to
compute (tests/bf16_model.py: bf16 planes of the operands, the mode's plane products, float64 on the CPU) at the tolerances
of their f32 / bf16x6 twins in test_hip_parity.py - against that reference a kernel owes fp32 accumulation error only, so a
dropped K tail, a garbage pixel in a BatchNorm sum or a wrong image of a multi-image tile fails here although it passes the
percent-level whole-step bounds these modes had so far.  Every check prints observed / tolerance; each test prints its worst.

Routing facts this module relies on and checks:
  - sbl_conv_patch_tile sizes its tile from an LDS budget per plane, so in these modes the 6x6, 7x7, 4x4, 4x5 (both modes)
    and 3x3 (bf16) maps run sbl_conv_patch_kernel with 5 to 28 whole images per tile; the f32 / bf16x6 suite never goes
    beyond two.
  - decoder-sized dense products go to sbl_skinny_gemm_kernel, which multiplies in exact fp32 in EVERY mode (skinny_gemm.h).
    The GEMM checks ask the library which kernel the launch took (sbl_profile_last_kernel) and hold a skinny launch to the
    unrounded product, every tile-engine launch to the named mode; the epilogue and split-K checks run a second time at a K
    the skinny kernel does not take, so that the tile engine's epilogues are reached in these modes too.
  - the stem weight gradient forms its second operand (the BatchNorm / pool adjoint) inside the kernel, so it has no
    operand-rounded reference; it stays with test_stem_reduced_precision_modes in test_hip_parity.py.
"""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_model as BM
from conftest import maxdiff
from sbl_for_multilingual_lip_reading_amd import detfill

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KID_SKINNY = 1      # sbl_profile_last_kernel: 1 skinny GEMM, 2 / 3 tiled 64x64 / 128x128 (include/sbl_hip.h)


@pytest.fixture(scope="module", params=["bf16x3", "bf16"])
def rp(request):
    from sbl_for_multilingual_lip_reading_amd import _lib, ops as _ops
    _lib.load()
    assert torch.cuda.is_available()
    _ops.set_matmul_precision(request.param)
    yield _ops, request.param
    _ops.set_matmul_precision("f32")


@pytest.fixture(autouse=True)
def _mode_is_set(rp):
    """The precision is process-wide; make sure no other module's fixture left another one behind."""
    ops, mode = rp
    ops.set_matmul_precision(mode)
    yield
    assert ops.get_matmul_precision() == mode


def U(name, shape, s=1.0):
    return torch.from_numpy(detfill.uniform(name, shape) * np.float32(s))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


class Checks:
    def __init__(self, label):
        self.label, self.rows = label, []

    def lt(self, what, observed, tol):
        observed, tol = float(observed), float(tol)
        self.rows.append((observed / tol if tol > 0 else float("inf"), what, observed, tol))
        print("  %s | %s: %.3e / %.3e = %.3f" % (self.label, what, observed, tol, self.rows[-1][0]))
        assert observed < tol, "%s | %s: observed %.3e, tolerance %.3e" % (self.label, what, observed, tol)

    def differs(self, what, observed, tol, gap, model_err):
        """Proof that the named mode ran: the output is further than the tolerance from the UNROUNDED result.  Decisive
        only where the model itself is (gap, computed on the CPU, at least 3 x the tolerance)."""
        if gap >= 3 * tol:
            print("  %s | %s: %.3e from the unrounded result, tolerance %.3e (model gap %.3e)" % (self.label, what, observed, tol, gap))
            assert observed > tol, "%s | %s: within %.3e of the unrounded result - a higher-precision kernel ran" % (self.label, what, tol)
            return True
        # (bf16x3 at these tolerances.)  Still asserted: the output is closer to the named mode's model than to the unrounded
        # result, which a launch that ran bf16x6 or f32 instead would not be
        print("  %s | %s: model gap %.3e < 3 x tolerance %.3e; %.3e from the model, %.3e from the unrounded result"
              % (self.label, what, gap, tol, model_err, observed))
        assert observed > model_err, "%s | %s: closer to the unrounded result than to the %s" % (self.label, what, "model")
        return False


@contextlib.contextmanager
def checks(label):
    c = Checks(label)
    try:
        yield c
    finally:
        if c.rows:
            w = max(c.rows)
            print("WORST %s | %s: %.3e / %.3e = %.3f" % (label, w[1], w[2], w[3], w[0]))


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _last_kernel():
    from sbl_for_multilingual_lip_reading_amd import _lib
    return _lib.load().sbl_profile_last_kernel()


def _gemm_mode(mode):
    """The arithmetic the launch just enqueued is held to: the skinny kernel is exact fp32 in every mode."""
    return "f32" if _last_kernel() == KID_SKINNY else mode


# --------------------------------------------------------------------------- dense GEMM
@pytest.mark.parametrize("ta,tb", [(0, 1), (0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(928, 512, 512), (32, 58, 512), (100, 70, 36), (512, 2048, 512), (37, 1536, 64),
                                   (2048, 512, 2048), (1, 64, 7)])
def test_gemm(rp, ta, tb, M, N, K):
    ops, mode = rp
    A = U("gA%d%d" % (M, K), (K, M) if ta else (M, K))
    B = U("gB%d%d" % (N, K), (N, K) if tb else (K, N))
    Ad, Bd = A.to(DEV), B.to(DEV)
    C = torch.empty(M, N, device=DEV)
    ops.gemm(ta, tb, M, N, K, Ad, A.size(1), Bd, B.size(1), C, N)
    eff = _gemm_mode(mode)
    ref = BM.bilinear(torch.matmul, A.t() if ta else A, B.t() if tb else B, eff)
    with checks("gemm %s(%s) %dx%dx%d ta%d tb%d" % (mode, eff, M, N, K, ta, tb)) as c:
        c.lt("C", maxdiff(C, ref), 2e-6 * max(K, 16) ** 0.5 * 4)      # twin: test_hip_parity.test_gemm


@pytest.mark.parametrize("ta,tb", [(0, 1), (1, 0)])
def test_gemm_big_tiles_odd_slab_count(rp, ta, tb):
    """128x128 tiles, K = 63 slabs of 16 + a ragged tail of 4, NaN-prefilled output: the split-bf16 bodies of the larger
    tiles (PREC = 3 / 1 instantiations) run the missing slab on zeros.  Also the module's GEMM proof that the named mode ran."""
    ops, mode = rp
    M, N, K = 4160, 4096, 16 * 63 + 4
    g = torch.Generator().manual_seed(5)
    A = torch.rand((K, M) if ta else (M, K), generator=g) * 2 - 1
    B = torch.rand((N, K) if tb else (K, N), generator=g) * 2 - 1
    C = torch.full((M, N), float("nan"), device=DEV)
    ops.gemm(ta, tb, M, N, K, A.to(DEV), A.size(1), B.to(DEV), B.size(1), C, N)
    assert _last_kernel() != KID_SKINNY
    Ao, Bo = (A.t() if ta else A), (B.t() if tb else B)
    ref = BM.bilinear(torch.matmul, Ao, Bo, mode)
    exact = Ao.double() @ Bo.double()
    tol = 2e-6 * K ** 0.5 * 4                                          # twin: test_gemm_big_tiles_odd_slab_count
    with checks("gemm big tiles %s ta%d tb%d" % (mode, ta, tb)) as c:
        c.lt("C", maxdiff(C, ref), tol)
        decisive = c.differs("C vs unrounded", maxdiff(C, exact), tol, float((ref - exact).abs().max()), maxdiff(C, ref))
        assert decisive or mode != "bf16"


@pytest.mark.parametrize("K,K2", [(96, 4096), (100, 4100)])
def test_gemm_epilogues_and_strides(rp, K, K2):
    """test_hip_parity.test_gemm_epilogues_and_strides in full (K = 96 / 4096: the skinny kernel takes both products), and once
    more at K = 100 / 4100 (K % 8 != 0: the tile engine's epilogues and its in-launch split-K in the reduced modes)."""
    ops, mode = rp
    M, N = 70, 130
    A, W, b = U("eA%d" % K, (M, K + 8)), U("eW%d" % K, (N, K)), U("eb", (N,))
    Ad, Wd, bd = A.to(DEV), W.to(DEV), b.to(DEV)
    x = Ad[:, :K]                                     # row stride K + 8: strided operand view
    with checks("gemm epilogues %s K=%d/%d" % (mode, K, K2)) as c:
        # tolerances: those of the twin, check by check
        C = torch.full((M, N + 4), 7.0, device=DEV)
        ops.gemm(0, 1, M, N, K, x, K + 8, Wd, K, C, N + 4, bias=bd)          # ldc > N
        eff = _gemm_mode(mode)
        assert eff == mode or K % 8 == 0              # K % 8 != 0 is not a skinny shape: the tile engine ran
        prod = BM.bilinear(torch.matmul, A[:, :K], W.t(), eff)
        ref = prod + b.double()
        c.lt("bias, ldc > N", maxdiff(C[:, :N], ref), 1e-5)
        assert float(C[:, N:].min()) == 7.0 and float(C[:, N:].max()) == 7.0
        C2 = torch.empty(M, N, device=DEV)
        ops.gemm(0, 1, M, N, K, x, K + 8, Wd, K, C2, N, bias=bd, relu=1)
        c.lt("bias + ReLU", maxdiff(C2, ref.clamp_min(0)), 1e-5)
        mask = U("em", (M, N))
        C3 = torch.empty(M, N, device=DEV)
        ops.gemm(0, 1, M, N, K, x, K + 8, Wd, K, C3, N, mask=mask.to(DEV), ldm=N)
        c.lt("mask", maxdiff(C3, prod * (mask > 0)), 1e-5)
        C4 = C2.clone()
        ops.gemm(0, 1, M, N, K, x, K + 8, Wd, K, C4, N, accumulate=1)
        c.lt("accumulate", maxdiff(C4, C2.cpu().double() + prod), 2e-5)
        c.lt("accumulate (from the model)", maxdiff(C4, ref.clamp_min(0) + prod), 2e-5)
        # split-K path (plain epilogue, few tiles, K >= 256), overwrite and accumulate
        M, N, K = 64, 64, K2
        A, W = U("sA%d" % K, (M, K)), U("sW%d" % K, (N, K))
        C5 = torch.full((M, N), 3.0, device=DEV)
        ops.gemm(0, 1, M, N, K, A.to(DEV), K, W.to(DEV), K, C5, N)
        eff = _gemm_mode(mode)
        assert eff == mode or K % 8 == 0
        ref = BM.bilinear(torch.matmul, A, W.t(), eff)
        c.lt("split-K overwrite", maxdiff(C5, ref), 1e-4)
        ops.gemm(0, 1, M, N, K, A.to(DEV), K, W.to(DEV), K, C5, N, accumulate=1)
        c.lt("split-K accumulate", maxdiff(C5, 2 * ref), 2e-4)
        cs = torch.empty(N, device=DEV)
        ops.call("sbl_colsum_f32", C5.data_ptr(), N, cs.data_ptr(), M, N, 0, ops._s())
        c.lt("colsum", maxdiff(cs, (2 * ref).sum(0)), 1e-3)
        assert float(ops._workspace()[:4096].abs().max()) == 0.0      # split-K tile counters re-armed


@pytest.mark.parametrize("M,N,K,relu", [(32, 512, 512, 0), (96, 1536, 512, 0), (416, 2048, 512, 1), (640, 512, 2048, 0),
                                        (992, 512, 512, 0), (1440, 1536, 512, 0), (2208, 2048, 512, 1), (2208, 512, 2048, 0),
                                        (70, 58, 512, 0)])
def test_gemm2_equals_two_products(rp, M, N, K, relu):
    """All gemm2 shapes of the twin; (416 / 640 / 992, ...) are the <= 320-tile launches that take the 512-thread wave-group
    K split (NH = 2 bodies of PREC 3 / 1)."""
    ops, mode = rp
    A = [U("g2a%d%d%d" % (M, K, d), (M, K)) for d in (0, 1)]
    B = [U("g2b%d%d%d" % (N, K, d), (N, K), 0.05) for d in (0, 1)]
    bias = [U("g2c%d%d" % (N, d), (N,)) for d in (0, 1)]
    C = [torch.full((M, N), float("nan"), device=DEV) for _ in (0, 1)]
    Ad, Bd, bd = [t.to(DEV) for t in A], [t.to(DEV) for t in B], [t.to(DEV) for t in bias]
    ops.gemm2(M, N, K, Ad[0], Ad[1], K, Bd[0], Bd[1], K, C[0], C[1], N, bd[0], bd[1], relu=relu)
    eff = _gemm_mode(mode)
    assert float(ops._workspace()[:4096].abs().max()) == 0.0      # split-K tile counters re-armed
    with checks("gemm2 %s(%s) %dx%dx%d" % (mode, eff, M, N, K)) as c:
        for d in (0, 1):
            ref = BM.bilinear(torch.matmul, A[d], B[d].t(), eff) + bias[d].double()
            if relu:
                ref = ref.clamp_min(0)
            c.lt("C%d" % d, maxdiff(C[d], ref), 4e-7 * K ** 0.5 * 4)      # twin: test_gemm2_equals_two_products


# --------------------------------------------------------------------------- merged decoder weight gradients
def _wgrad_refs(A, B, mode):
    dw = None
    for a, b in zip(A, B):
        t = BM.bilinear(lambda p, q: p.t() @ q, a, b, mode)
        dw = t if dw is None else dw + t
    colsum = sum(a.double().sum(0) for a in A)      # plain fp32 column sums of dY: no rounding of the operand
    return dw, colsum


@pytest.mark.parametrize("M,N,seg_rows", [(512, 512, (96, 37, 160, 5)), (2048, 512, (48, 131, 64)), (60, 132, (200, 9, 77))])
def test_wgrad_seg(rp, M, N, seg_rows):
    """sbl_wgrad_seg_f32 through ops._wgrad_seg: C += sum_s A_s^T B_s over segments of unequal row counts (rows that are
    not multiples of 16: the unaligned 64x64 loaders; 2048x512 with aligned rows would take the 128x128 tiles - see the
    grouped test for those), accumulating into a non-zero C, with the bias gradient's column sums.  No twin in
    test_hip_parity.py (the merged weight gradients are only reached through whole steps there; their f32 / bf16x6
    instantiations are tested in test_gemm_routes_gpu.py): the GEMM tolerance
    4e-7 * sqrt(K) * 4 over K = all rows, split-K float atomics included; column sums as test_gemm_epilogues' colsum."""
    ops, mode = rp
    A = [U("ws.a%d%d%d" % (s, r, M), (r, M)) for s, r in enumerate(seg_rows)]
    B = [U("ws.b%d%d%d" % (s, r, N), (r, N)) for s, r in enumerate(seg_rows)]
    C0, cs0 = U("ws.c%d%d" % (M, N), (M, N)), U("ws.cs%d" % M, (M,))
    C, cs = C0.to(DEV), cs0.to(DEV)
    Ad, Bd = [t.to(DEV) for t in A], [t.to(DEV) for t in B]
    ops._wgrad_seg(C, N, cs, Ad, M, Bd, N, M, N, list(seg_rows))
    assert _last_kernel() != KID_SKINNY
    dw, colsum = _wgrad_refs(A, B, mode)
    K = sum(seg_rows)
    with checks("wgrad_seg %s %dx%d rows %s" % (mode, M, N, seg_rows)) as c:
        c.lt("C += dW", maxdiff(C, C0.double() + dw), 4e-7 * max(K, 16) ** 0.5 * 4)
        c.lt("colsum", maxdiff(cs, cs0.double() + colsum), 1e-3)


def test_wgrad_seg_aligned_128_tiles(rp):
    """... and with rows that are multiples of 16 on a weight with >= 48 128x128 tiles (SegMC<128, true>)."""
    ops, mode = rp
    M, N, seg_rows = 2048, 512, (48, 160, 64, 16)
    A = [U("wsa.a%d" % s, (r, M)) for s, r in enumerate(seg_rows)]
    B = [U("wsa.b%d" % s, (r, N)) for s, r in enumerate(seg_rows)]
    C, cs = torch.zeros(M, N, device=DEV), torch.zeros(M, device=DEV)
    ops._wgrad_seg(C, N, cs, [t.to(DEV) for t in A], M, [t.to(DEV) for t in B], N, M, N, list(seg_rows))
    dw, colsum = _wgrad_refs(A, B, mode)
    with checks("wgrad_seg aligned %s" % mode) as c:
        c.lt("dW", maxdiff(C, dw), 4e-7 * sum(seg_rows) ** 0.5 * 4)
        c.lt("colsum", maxdiff(cs, colsum), 1e-3)


@pytest.mark.parametrize("seg_rows", [(48, 160, 64), (208,)])
def test_wgrad_group(rp, seg_rows):
    """sbl_wgrad_group_f32 through ops.wgrad_group: problems of different M / N (partial 128x128 tiles included) in one
    launch, segmented and one-segment loaders, column sums on some problems; deterministic - two runs are bit-equal.  Same
    tolerances as test_wgrad_seg."""
    ops, mode = rp
    dims = [(512, 512), (2048, 512), (60, 132), (512, 2048)]
    probs = []
    for p, (M, N) in enumerate(dims):
        A = [U("wgp.a%d%d%d" % (p, s, r), (r, M)) for s, r in enumerate(seg_rows)]
        B = [U("wgp.b%d%d%d" % (p, s, r), (r, N)) for s, r in enumerate(seg_rows)]
        probs.append((M, N, A, B, U("wgp.c%d" % p, (M, N)), U("wgp.cs%d" % p, (M,)) if p != 2 else None))

    def per_weight(*a):
        raise AssertionError("the grouped kernel did not take the problems")

    def run():
        out, problems = [], []
        for M, N, A, B, C0, cs0 in probs:
            C, cs = C0.to(DEV), None if cs0 is None else cs0.to(DEV)
            out.append((C, cs))
            problems.append((C, N, cs, [t.to(DEV) for t in A], M, [t.to(DEV) for t in B], N, M, N))
        ops.wgrad_group(problems, tuple(seg_rows), torch.cuda.current_stream(), per_weight)
        torch.cuda.synchronize()
        return out
    first, second = run(), run()
    K = sum(seg_rows)
    with checks("wgrad_group %s rows %s" % (mode, seg_rows)) as c:
        for p, (M, N, A, B, C0, cs0) in enumerate(probs):
            dw, colsum = _wgrad_refs(A, B, mode)
            c.lt("problem %d (%dx%d) C += dW" % (p, M, N), maxdiff(first[p][0], C0.double() + dw), 4e-7 * max(K, 16) ** 0.5 * 4)
            assert torch.equal(first[p][0], second[p][0]), "problem %d: two runs differ" % p
            if cs0 is not None:
                c.lt("problem %d colsum" % p, maxdiff(first[p][1], cs0.double() + colsum), 1e-3)


# --------------------------------------------------------------------------- trunk convolutions
TWIN_CONV_CASES = [
    (3, 22, 22, 64, 64, 3, 1), (5, 22, 22, 64, 128, 3, 2), (5, 22, 22, 64, 128, 1, 2), (4, 11, 11, 128, 128, 3, 1),
    (6, 6, 6, 256, 512, 3, 2), (7, 3, 3, 512, 512, 3, 1), (2, 7, 5, 64, 64, 3, 2), (40, 22, 22, 64, 64, 3, 1),
    (20, 22, 22, 128, 128, 3, 1), (3, 28, 28, 64, 64, 3, 1), (2, 20, 24, 64, 128, 3, 1), (300, 22, 22, 64, 64, 3, 1),
    (5, 11, 11, 128, 128, 3, 1), (601, 11, 11, 128, 128, 3, 1), (3, 10, 12, 128, 64, 3, 1),
    (150, 3, 3, 512, 512, 3, 1), (130, 6, 6, 256, 256, 3, 1), (70, 6, 6, 256, 256, 3, 1), (33, 4, 5, 256, 128, 3, 1),
    (9, 5, 4, 128, 256, 3, 1)]
# geometries only these modes send to the patch-resident kernel: G = 7 images per tile at 6x6 (5 < G; 130 = 18 * 7 + 4),
# 28 at 3x3 (bf16 only), 5 at 7x7, 16 at 4x4, 12 at 4x5
MULTI_IMAGE_CASES = [(n, 6, 6, 256, 256, 3, 1) for n in (5, 7)] + [(n, 3, 3, 512, 512, 3, 1) for n in (27, 28, 29)] + [
    (12, 7, 7, 256, 256, 3, 1), (33, 4, 4, 512, 512, 3, 1)]


def _conv_inputs(NIMG, H, W, Cin, Cout, k, stride):
    pad = 1 if k == 3 else 0
    x = U("cx%d%d%d" % (NIMG, H, Cin), (NIMG, Cin, H, W))
    w = U("cw%d%d%d" % (Cout, Cin, k), (Cout, Cin, k, k), 0.1)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    dy = U("cdy%d%d" % (NIMG, Cout), (NIMG, Cout, Ho, Wo))
    return pad, x, w, dy


def _pack(ops, w):
    Cout, Cin, k, _ = w.shape
    wd = w.to(DEV)
    w_ohwi, w_dg = torch.empty(Cout, k, k, Cin, device=DEV), torch.empty(Cin, k, k, Cout, device=DEV)
    ops.call("sbl_conv_weight_pack", wd.data_ptr(), w_ohwi.data_ptr(), w_dg.data_ptr(), Cout, Cin, k, k, None, 0, ops._s())
    return w_ohwi, w_dg


@contextlib.contextmanager
def knob(ops, which, value, default):
    ops.call("sbl_set_tuning", which, value)
    try:
        yield
    finally:
        ops.call("sbl_set_tuning", which, default)


@pytest.mark.parametrize("NIMG,H,W,Cin,Cout,k,stride", TWIN_CONV_CASES + MULTI_IMAGE_CASES)
def test_conv2d_fwd_dgrad_wgrad(rp, NIMG, H, W, Cin, Cout, k, stride):
    """Forward with BN statistics, input gradient and weight gradient against the model; the 3x3 / stride-1 cases under
    knob 5 = 2 (patch-resident kernel where sbl_conv_patch_tile takes the map) and knob 5 = 0 (gather / position-major
    kernels).  The statistics are checked against the model output's own sums: on tiles with a partial image group this is
    where images that are not there would show.  Twin of every check: test_hip_parity.test_conv2d_fwd_dgrad_wgrad."""
    ops, mode = rp
    pad, x, w, dy = _conv_inputs(NIMG, H, W, Cin, Cout, k, stride)
    y = BM.bilinear(lambda a, b: F.conv2d(a, b, None, stride, pad), x, w, mode)
    dx = BM.bilinear(lambda g, b: torch.nn.grad.conv2d_input(x.shape, b, g, stride, pad), dy, w, mode)
    dw = BM.bilinear(lambda a, g: torch.nn.grad.conv2d_weight(a, w.shape, g, stride, pad), x, dy, mode)
    Ho, Wo = y.shape[2:]
    xd, dyd = _nhwc(x).to(DEV), _nhwc(dy).to(DEV)
    w_ohwi, w_dg = _pack(ops, w)
    ws = ops._workspace()
    yn = _nhwc(y).reshape(-1, Cout)
    with checks("conv %s %s" % (mode, (NIMG, H, W, Cin, Cout, k, stride))) as c:
        for kv in ((2, 0) if (k == 3 and stride == 1) else (2,)):
            with knob(ops, 5, kv, 2):
                yd = torch.full((NIMG, Ho, Wo, Cout), float("nan"), device=DEV)
                stats = torch.empty(2 * Cout, device=DEV, dtype=torch.float64)
                ops.call("sbl_conv2d_fwd", xd.data_ptr(), w_ohwi.data_ptr(), yd.data_ptr(), stats.data_ptr(), 0, NIMG, H, W, Cin, Cout,
                         k, k, stride, pad, ws.data_ptr(), ops.WS_BYTES, ops._s())
                dxd = torch.full(tuple(xd.shape), float("nan"), device=DEV)
                ops.call("sbl_conv2d_dgrad", dyd.data_ptr(), w_dg.data_ptr(), dxd.data_ptr(), NIMG, H, W, Cin, Cout, k, k, stride,
                         pad, ws.data_ptr(), ops.WS_BYTES, ops._s())
                torch.cuda.synchronize()
            t = "knob5=%d " % kv
            c.lt(t + "y", maxdiff(yd, _nhwc(y)), 4e-7 * (Cin * k * k) ** 0.5 * 4)
            c.lt(t + "stats sum", relerr(stats[:Cout], yn.sum(0)), 1e-5)
            c.lt(t + "stats sumsq", relerr(stats[Cout:], (yn * yn).sum(0)), 1e-5)
            assert float(ws[:4096].abs().max()) == 0.0      # tile counters are left re-armed (zero)
            c.lt(t + "dx", maxdiff(dxd, _nhwc(dx)), 4e-7 * (Cout * k * k) ** 0.5 * 4)
        dwd = torch.empty(Cout, k, k, Cin, device=DEV)
        ops.call("sbl_conv2d_wgrad", xd.data_ptr(), dyd.data_ptr(), dwd.data_ptr(), NIMG, H, W, Cin, Cout, k, k, stride, pad,
                 0, ops._s())
        dwo = torch.empty(Cout, Cin, k, k, device=DEV)
        ops.call("sbl_conv_wgrad_unpack", dwd.data_ptr(), dwo.data_ptr(), Cout, Cin, k, k, 0, ops._s())
        c.lt("dw", relerr(dwo, dw), 2e-5)
        ops.call("sbl_conv_wgrad_unpack", dwd.data_ptr(), dwo.data_ptr(), Cout, Cin, k, k, 1, ops._s())     # += form
        c.lt("dw +=", relerr(dwo, 2 * dw), 2e-5)


def test_conv_named_mode_ran(rp):
    """Proof for the convolutions: unit-scale weights (the twin's 0.1 scale puts bf16x3's rounding inside the tolerance),
    layer 3's 6x6 map with a partial last image group."""
    ops, mode = rp
    NIMG, H, W, C = 130, 6, 6, 256
    x, w = U("pm.x", (NIMG, C, H, W)), U("pm.w", (C, C, 3, 3))
    y = BM.bilinear(lambda a, b: F.conv2d(a, b, None, 1, 1), x, w, mode)
    exact = F.conv2d(x.double(), w.double(), None, 1, 1)
    xd = _nhwc(x).to(DEV)
    w_ohwi, _ = _pack(ops, w)
    yd = torch.empty(NIMG, H, W, C, device=DEV)
    ops.call("sbl_conv2d_fwd", xd.data_ptr(), w_ohwi.data_ptr(), yd.data_ptr(), None, 0, NIMG, H, W, C, C, 3, 3, 1, 1, None, 0, ops._s())
    tol = 4e-7 * (9 * C) ** 0.5 * 4 * 10      # unit weights: ten times the twin's operand scale
    with checks("conv proof %s" % mode) as c:
        c.lt("y", maxdiff(yd, _nhwc(y)), tol)
        decisive = c.differs("y vs unrounded", maxdiff(yd, _nhwc(exact)), tol, float((y - exact).abs().max()), maxdiff(yd, _nhwc(y)))
        assert decisive or mode != "bf16"


# --------------------------------------------------------------------------- fused input-gradient epilogues
def _bn_operands(tag, shape, C):
    pre = U("fe.pre" + tag, shape)
    mean, inv = U("fe.mu" + tag, (C,), 0.1), U("fe.is" + tag, (C,), 0.2) + 1.0
    return pre, mean, inv


def _bn_sums(g, pre, mean, inv):
    xhat = (pre.double() - mean.double()) * inv.double()
    return torch.cat([g.sum((0, 1, 2)), (g * xhat).sum((0, 1, 2))])


@pytest.mark.parametrize("NIMG,H,W,C", [(130, 6, 6, 256), (150, 3, 3, 512), (12, 7, 7, 256), (40, 22, 22, 64)])
def test_fused_dgrad_epilogues(rp, NIMG, H, W, C):
    """sbl_conv2d_dgrad_bnstats (dx bit-equal to sbl_conv2d_dgrad in the same mode) and the three stride-1 forms of
    sbl_conv2d_dgrad_fused - addend alone, addend + one BatchNorm, addend + two - with dx against the model and the sums
    against float64 sums built from the model dx.  Twin: test_dgrad_epilogue_reduces_the_next_batchnorm_backward (dx at the
    input-gradient tolerance of test_conv2d_fwd_dgrad_wgrad, sums at 2e-5 of the largest sum)."""
    ops, mode = rp
    shape = (NIMG, H, W, C)
    dy, w = U("fe.dy%d%d" % (H, C), (NIMG, C, H, W)), U("fe.w%d%d" % (H, C), (C, C, 3, 3), 0.1)
    pre, mean, inv = _bn_operands("%d" % H, shape, C)
    pre2, mean2, inv2 = _bn_operands("b%d" % H, shape, C)
    act = ((pre - mean) * inv).clamp_min(0).contiguous()      # fp32 on the CPU: both sides see the same (act > 0)
    addend = U("fe.add%d" % H, shape)
    dxm = _nhwc(BM.bilinear(lambda g, b: torch.nn.grad.conv2d_input((NIMG, C, H, W), b, g, 1, 1), dy, w, mode))
    dyd = _nhwc(dy).to(DEV)
    _, w_dg = _pack(ops, w)
    ws = ops._workspace()
    d = {k: v.to(DEV) for k, v in dict(pre=pre, mean=mean, inv=inv, pre2=pre2, mean2=mean2, inv2=inv2, act=act, add=addend).items()}
    tol = 4e-7 * (9 * C) ** 0.5 * 4
    pos = (act > 0)

    def fused(addend_, bn, bn2):
        dx = torch.full(shape, float("nan"), device=DEV)
        sums = torch.full(((4 if bn2 else 2) * C,), float("nan"), device=DEV, dtype=torch.float64) if bn else None
        ops.call("sbl_conv2d_dgrad_fused", dyd.data_ptr(), w_dg.data_ptr(), dx.data_ptr(), NIMG, H, W, C, C, 3, 3, 1, 1, ws.data_ptr(),
                 ops.WS_BYTES, d["add"].data_ptr() if addend_ else None, *([d["act"].data_ptr(), d["pre"].data_ptr(), d["mean"].data_ptr(),
                                                                           d["inv"].data_ptr()] if bn else [None] * 4),
                 *([d["pre2"].data_ptr(), d["mean2"].data_ptr(), d["inv2"].data_ptr()] if bn2 else [None] * 3),
                 None if sums is None else sums.data_ptr(), 0, ops._s())
        torch.cuda.synchronize()
        return dx, sums
    with checks("fused dgrad %s %s" % (mode, shape)) as c:
        dx0, dx1 = torch.empty(shape, device=DEV), torch.empty(shape, device=DEV)
        ops.call("sbl_conv2d_dgrad", dyd.data_ptr(), w_dg.data_ptr(), dx0.data_ptr(), NIMG, H, W, C, C, 3, 3, 1, 1, ws.data_ptr(), ops.WS_BYTES, ops._s())
        sums = torch.full((2 * C,), float("nan"), device=DEV, dtype=torch.float64)
        ops.call("sbl_conv2d_dgrad_bnstats", dyd.data_ptr(), w_dg.data_ptr(), dx1.data_ptr(), NIMG, H, W, C, C, 3, 3, 1, 1, ws.data_ptr(),
                 ops.WS_BYTES, d["act"].data_ptr(), d["pre"].data_ptr(), d["mean"].data_ptr(), d["inv"].data_ptr(), sums.data_ptr(), 0, ops._s())
        assert torch.equal(dx0, dx1)
        c.lt("bnstats dx", maxdiff(dx1, dxm), tol)
        exact = _bn_sums(dxm * pos, pre, mean, inv)
        c.lt("bnstats sums", float((sums.cpu() - exact).abs().max()), 2e-5 * float(exact.abs().max()))
        dx, _ = fused(True, False, False)
        c.lt("addend dx", maxdiff(dx, dxm + addend.double()), tol)
        g = (dxm + addend.double()) * pos
        dx, sums = fused(True, True, False)
        c.lt("addend + BN dx", maxdiff(dx, dxm + addend.double()), tol)
        exact = _bn_sums(g, pre, mean, inv)
        c.lt("addend + BN sums", float((sums.cpu() - exact).abs().max()), 2e-5 * float(exact.abs().max()))
        dx, sums = fused(True, True, True)
        c.lt("addend + 2 BN dx", maxdiff(dx, dxm + addend.double()), tol)
        exact = torch.cat([_bn_sums(g, pre, mean, inv), _bn_sums(g, pre2, mean2, inv2)])
        c.lt("addend + 2 BN sums", float((sums.cpu() - exact).abs().max()), 2e-5 * float(exact.abs().max()))
        assert float(ws[:4096].abs().max()) == 0.0


def test_compact_downsample_gradient_feeds_the_stride2_fused_form(rp):
    """sbl_conv1x1s2_dgrad_compact (64 -> 128 at 22x22: the compact even/even-pixel gradient of the downsample branch) and
    sbl_conv2d_dgrad_fused at stride 2 adding it on parity class (0, 0), with the previous block's BatchNorm sums."""
    ops, mode = rp
    NIMG, H, W, Cin, Cout = 9, 22, 22, 64, 128
    dy1, w1 = U("cp.dy1", (NIMG, Cout, 11, 11)), U("cp.w1", (Cout, Cin, 3, 3), 0.1)
    dyd_, wd_ = U("cp.dyd", (NIMG, Cout, 11, 11)), U("cp.wd", (Cout, Cin, 1, 1), 0.1)
    pre, mean, inv = _bn_operands("cp", (NIMG, H, W, Cin), Cin)
    act = ((pre - mean) * inv).clamp_min(0).contiguous()
    ws = ops._workspace()
    _, w1_dg = _pack(ops, w1)
    _, wd_dg = _pack(ops, wd_)
    dxc = torch.full((NIMG, 11, 11, Cin), float("nan"), device=DEV)
    dydd = _nhwc(dyd_).to(DEV)
    ops.call("sbl_conv1x1s2_dgrad_compact", dydd.data_ptr(), wd_dg.data_ptr(), dxc.data_ptr(), NIMG, H, W, Cin, Cout, ws.data_ptr(), ops.WS_BYTES, ops._s())
    dxc_m = BM.bilinear(torch.matmul, _nhwc(dyd_).reshape(-1, Cout), wd_.reshape(Cout, Cin), mode).reshape(NIMG, 11, 11, Cin)
    dx1_m = _nhwc(BM.bilinear(lambda g, b: torch.nn.grad.conv2d_input((NIMG, Cin, H, W), b, g, 2, 1), dy1, w1, mode))
    dx = torch.full((NIMG, H, W, Cin), float("nan"), device=DEV)
    sums = torch.full((2 * Cin,), float("nan"), device=DEV, dtype=torch.float64)
    dy1d, actd, pred, meand, invd = _nhwc(dy1).to(DEV), act.to(DEV), pre.to(DEV), mean.to(DEV), inv.to(DEV)
    ops.call("sbl_conv2d_dgrad_fused", dy1d.data_ptr(), w1_dg.data_ptr(), dx.data_ptr(), NIMG, H, W, Cin, Cout, 3, 3, 2, 1, ws.data_ptr(),
             ops.WS_BYTES, dxc.data_ptr(), actd.data_ptr(), pred.data_ptr(), meand.data_ptr(), invd.data_ptr(), None, None, None,
             sums.data_ptr(), 0, ops._s())
    ref = dx1_m.clone()
    ref[:, ::2, ::2] += dxc.cpu().double()      # the kernel's own compact gradient, added exactly: isolates the fused launch
    g = ref * (act > 0)
    exact = _bn_sums(g, pre, mean, inv)
    with checks("compact + stride-2 fused %s" % mode) as c:
        c.lt("compact dx", maxdiff(dxc, dxc_m), 4e-7 * Cout ** 0.5 * 4)          # twin: the (5, 22, 22, 64, 128, 1, 2) input gradient
        c.lt("fused dx", maxdiff(dx, ref), 4e-7 * (9 * Cout) ** 0.5 * 4)         # twin: the (5, 22, 22, 64, 128, 3, 2) input gradient
        c.lt("fused sums", float((sums.cpu() - exact).abs().max()), 2e-5 * float(exact.abs().max()))


# --------------------------------------------------------------------------- patch-resident weight gradient
@pytest.mark.parametrize("NIMG,H,W,Cin,Cout,knob9", [
    (9, 22, 22, 64, 64, 100), (7, 11, 11, 128, 128, 100), (10, 6, 6, 256, 128, 30), (5, 28, 28, 64, 128, 100), (4, 14, 14, 128, 64, 100),
    (260, 11, 11, 64, 64, 100), (2, 9, 13, 64, 64, 100),
    # 7x7 and 4x4 (config 5's layers 3 and 4): other images-per-tile counts than the 6x6 case
    (12, 7, 7, 256, 128, 30), (33, 4, 4, 512, 256, 16)])
def test_conv_patch_weight_gradient(rp, NIMG, H, W, Cin, Cout, knob9):
    """The cases of test_hip_parity.test_conv_patch_weight_gradient_agrees_with_gather_kernels under knob 9 = their value and
    knob 9 = 0, each against the model at that test's relerr < 2e-5."""
    ops, mode = rp
    x = U("pw.x%d%d" % (H, Cin), (NIMG, Cin, H, W))
    dy = U("pw.dy%d%d" % (NIMG, Cout), (NIMG, Cout, H, W))
    dw = BM.bilinear(lambda a, g: torch.nn.grad.conv2d_weight(a, (Cout, Cin, 3, 3), g, 1, 1), x, dy, mode)
    xd, dyd = _nhwc(x).to(DEV), _nhwc(dy).to(DEV)
    with checks("patch wgrad %s %s" % (mode, (NIMG, H, W, Cin, Cout))) as c:
        for kv in (knob9, 0):
            with knob(ops, 9, kv, 30):
                dwd = torch.full((Cout, 3, 3, Cin), float("nan"), device=DEV)
                ops.call("sbl_conv2d_wgrad", xd.data_ptr(), dyd.data_ptr(), dwd.data_ptr(), NIMG, H, W, Cin, Cout, 3, 3, 1, 1, 0, ops._s())
                torch.cuda.synchronize()
            c.lt("knob9=%d dw" % kv, relerr(dwd.permute(0, 3, 1, 2), dw), 2e-5)


# --------------------------------------------------------------------------- stem forward through the raw ABI
@pytest.mark.parametrize("N,T,H,W", [(2, 6, 32, 32), (1, 3, 88, 88), (2, 2, 24, 40), (1, 5, 112, 112)])
def test_stem_conv_fwd(rp, N, T, H, W):
    """sbl_stem_conv_fwd against F.conv3d over the planes: conv_out within the 2e-5 of test_hip_parity.test_stem_fwd_bwd, the
    (sum, sumsq) statistics at the convolutions' relerr < 1e-5; and the stem's proof that the named mode ran."""
    ops, mode = rp
    x = torch.from_numpy(detfill.normal("stem.x%d%d" % (H, W), (N, T, H, W)))
    w = U("stem.w", (64, 1, 5, 7, 7), 0.08)
    conv3 = lambda a, b: F.conv3d(a, b, None, (1, 2, 2), (2, 3, 3))      # noqa: E731
    ref = BM.bilinear(conv3, x.unsqueeze(1), w, mode)                   # (N, 64, T, Ho, Wo)
    exact = conv3(x.unsqueeze(1).double(), w.double())
    Ho, Wo = H // 2, W // 2
    to_nhwc = lambda t: t.permute(0, 2, 3, 4, 1).reshape(N * T, Ho, Wo, 64)      # noqa: E731
    conv = torch.full((N * T, Ho, Wo, 64), float("nan"), device=DEV)
    stats = torch.full((128,), float("nan"), device=DEV, dtype=torch.float64)
    xd, wd = x.to(DEV), w.reshape(64, 245).contiguous().to(DEV)
    ops.call("sbl_stem_conv_fwd", xd.data_ptr(), wd.data_ptr(), conv.data_ptr(), stats.data_ptr(), N, T, H, W, ops._s())
    rn = to_nhwc(ref).reshape(-1, 64)
    with checks("stem fwd %s %s" % (mode, (N, T, H, W))) as c:
        c.lt("conv_out", maxdiff(conv, to_nhwc(ref)), 2e-5)
        c.lt("stats sum", relerr(stats[:64], rn.sum(0)), 1e-5)
        c.lt("stats sumsq", relerr(stats[64:], (rn * rn).sum(0)), 1e-5)
        decisive = c.differs("conv_out vs unrounded", maxdiff(conv, to_nhwc(exact)), 2e-5, float((ref - exact).abs().max()),
                             maxdiff(conv, to_nhwc(ref)))
        assert decisive or mode != "bf16"
