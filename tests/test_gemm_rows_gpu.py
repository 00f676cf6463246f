"""sbl_gemm2_rows_f32 through the C ABI: the 16x16-tile kernel on every shape class it takes, and the calls it hands on.

Every launch is checked as tests/test_gemm_routes_gpu.py checks the dense family (its helpers are used here):
  * route: sbl_profile_last_route() is what tests/gemm_rows.py predicts - family 9, tile 4 with the kernel's (V, U), or
    tile 0 for a forwarded call - and sbl_profile_last_kernel() is 1 (skinny) or, forwarded, the family
    gemm_routes.route_gemm2() predicts;
  * frame: both outputs live in NaN-prefilled M x N windows of sentinel buffers with ldc = N + 4 and a guard row above and
    below; the sentinels must survive and no NaN may remain.  Operand padding (lda = K + 4, ldb = K + 8) is NaN;
  * value: EXACT on integer data under all four precisions (the kernel is exact fp32 in every mode), and on uniform data
    against float64 within the bound of the 32x32 skinny leaf at that K,
        |C - ref| <= (K + c) * U * (|A||B| + |bias|),  c = gemm_routes.extra_roundings(skinny dual leaf of K)
    (NW = 4 or 8 for the LDS meet, + 1 for a bias).  It is this kernel's bound too: it cuts K into the same NW chains of
    fused multiply-adds, which meet in the same NW additions.  For K % (16 * NW) == 0 the chains are the 32x32 kernel's
    own, term by term, and the output must EQUAL sbl_gemm2_f32's bit for bit (test_rows16_equals_gemm2_bitwise);
The two directions get separate data.  One float64 reference per (K, data kind) is computed for the largest shape (128 x
512) and sliced for the smaller ones."""
import functools

import numpy as np
import pytest
import torch

import gemm_rows as G
import gemm_routes as R
from test_gemm_routes_gpu import DEV, NAN, PRECS, ROUNDED_PRECS, Frame, P, S, U, check, f64, fill, kid, operand

pytestmark = pytest.mark.gpu

MS, NS, KS = (1, 16, 17, 33, 128), (16, 40, 512), (16, 48, 512, 2048)
EPIS = ("", "b", "r", "br")
PA, PB = 4, 8


@pytest.fixture(scope="module", autouse=True)
def ops():
    from sbl_for_multilingual_lip_reading_amd import _lib, ops as _ops
    _lib.load()
    assert torch.cuda.is_available()
    prev = _ops.get_matmul_precision()
    yield _ops
    _ops.set_matmul_precision(prev)


def last_route():
    from sbl_for_multilingual_lip_reading_amd import _lib
    return G.decode_route(_lib.load().sbl_profile_last_route())


@functools.lru_cache(maxsize=None)
def master(K, kind):
    """Host operands of both directions at 128 x 512 x K with their float64 products and magnitudes (read-only)."""
    d = {"A": [], "B": [], "bias": [], "ref": [], "mag": []}
    for t in (0, 1):
        tag = "%d.%d.%s" % (t, K, kind)
        A, B = fill(kind, "rows.A" + tag, (max(MS), K)), fill(kind, "rows.B" + tag, (max(NS), K))
        d["A"].append(A)
        d["B"].append(B)
        d["bias"].append(fill(kind, "rows.b" + tag, (max(NS),)))
        d["ref"].append(f64(A) @ f64(B).T)
        d["mag"].append(np.abs(f64(A)) @ np.abs(f64(B)).T)
    return d


@functools.lru_cache(maxsize=2)
def problem(M, N, K, kind):
    m = master(K, kind)
    d = {"A": [], "B": [], "bias": [], "ref": [], "mag": [], "absb": [], "keep": []}
    for t in (0, 1):
        ab, av = operand(m["A"][t][:M], K + PA, 0)
        bb, bv = operand(m["B"][t][:N], K + PB, 0)
        d["keep"] += [ab, bb]
        d["A"].append(av)
        d["B"].append(bv)
        d["bias"].append(torch.from_numpy(m["bias"][t][:N].copy()).to(DEV))
        d["ref"].append(torch.from_numpy(np.ascontiguousarray(m["ref"][t][:M, :N])).to(DEV))
        d["mag"].append(torch.from_numpy(np.ascontiguousarray(m["mag"][t][:M, :N])).to(DEV))
        d["absb"].append(d["bias"][t].double().abs())
    return d


def run_rows(ops, M, N, K, kind, precs):
    d = problem(M, N, K, kind)
    assert G.takes16(M, N, K, K + PA, K + PB, True)
    leaf32 = R.SK("dual", *R.skinny_nwu(K))      # the leaf whose bound the issue of this kernel holds it to
    worst = 0.0
    for prec in precs:
        ops.set_matmul_precision(prec)
        for epi in EPIS:
            what = "rows16 %dx%dx%d %s %s %s" % (M, N, K, epi or "plain", kind, prec)
            bias = d["bias"] if "b" in epi else [None, None]
            fr = [Frame(M, N, NAN) for _ in (0, 1)]
            ops.call("sbl_gemm2_rows_f32", M, N, K, P(d["A"][0]), P(d["A"][1]), K + PA, P(d["B"][0]), P(d["B"][1]), K + PB,
                     fr[0].ptr(), fr[1].ptr(), fr[0].ld, P(bias[0]), P(bias[1]), int("r" in epi), None, 0, S())
            assert kid() == R.KERNEL_ID["skinny"], what
            assert last_route() == (G.ROUTE_FAMILY, G.TILE_16) + G.vu16(K), "%s: noted route %s" % (what, last_route())
            c = R.extra_roundings(leaf32, "b" in epi, False, prec)
            for t in (0, 1):
                fr[t].check_frame(what)
                ref, mag = d["ref"][t], d["mag"][t]
                if "b" in epi:
                    ref, mag = ref + d["bias"][t].double(), mag + d["absb"][t]
                if "r" in epi:
                    ref = ref.clamp(min=0.0)                  # 1-Lipschitz: the bound carries over
                bound = None if kind == "int" else (K + c) * U * mag + R.dropped(leaf32, prec) * d["mag"][t]
                worst = max(worst, check("%s [%d]" % (what, t), fr[t].out(), ref, bound))
    return worst


SHAPES = [(M, N, K) for K in KS for N in NS for M in MS]


@pytest.mark.parametrize("M,N,K", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_rows16_exact(ops, M, N, K):
    """Integer operands and bias, all four precisions, plain / bias / ReLU / both: the outputs of both directions EQUAL the
    integer result; M = 1 (one row of one tile), 16, 17 (one row into the second tile), 33, 128; N = 40 with a ragged last
    column tile, N = 512 with the XCD tile order on; K = 16 and 48 leave ranges 1-3 / 3 of K empty."""
    run_rows(ops, M, N, K, "int", PRECS)


@pytest.mark.parametrize("M,N,K", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_rows16_rounded(ops, M, N, K):
    """Uniform data under f32 and bf16x6 against float64 within the skinny leaf's bound at that K.
    measured (worst err / bound over all cases): 0.19 under f32 and bf16x6 alike (128x40x16, plain: the shortest K)."""
    run_rows(ops, M, N, K, "uni", ROUNDED_PRECS)


BITWISE = [(M, N, K) for K in (64, 512, 2048) for M, N in ((17, 40), (33, 512), (128, 512))]


@pytest.mark.parametrize("M,N,K", BITWISE, ids=["%dx%dx%d" % s for s in BITWISE])
def test_rows16_equals_gemm2_bitwise(ops, M, N, K):
    """Where K % (16 * V) == 0 - every product of the decoder - the 16x16 kernel adds the same terms in the same order as
    the 32x32 skinny kernel sbl_gemm2_f32 takes for the shape: both outputs, uniform data, bias + ReLU and plain, are
    bit-identical, so moving a launch between the two changes nothing downstream."""
    assert G.same_sums(K) and G.takes16(M, N, K, K + PA, K + PB, True)
    assert R.route_gemm2(M, N, K, K + PA, K + PB, True, True, True, None).family == "skinny"
    d = problem(M, N, K, "uni")
    ops.set_matmul_precision("f32")
    for epi in ("", "br"):
        bias = d["bias"] if epi else [None, None]
        out = {}
        for name in ("sbl_gemm2_f32", "sbl_gemm2_rows_f32"):
            fr = [Frame(M, N, NAN) for _ in (0, 1)]
            ops.call(name, M, N, K, P(d["A"][0]), P(d["A"][1]), K + PA, P(d["B"][0]), P(d["B"][1]), K + PB, fr[0].ptr(), fr[1].ptr(),
                     fr[0].ld, P(bias[0]), P(bias[1]), int(bool(epi)), None, 0, S())
            assert kid() == R.KERNEL_ID["skinny"]
            out[name] = fr
        assert last_route()[:2] == (G.ROUTE_FAMILY, G.TILE_16)
        for t in (0, 1):
            x, y = out["sbl_gemm2_f32"][t].buf, out["sbl_gemm2_rows_f32"][t].buf
            assert bool(torch.isfinite(y).all())
            assert torch.equal(x, y), "%dx%dx%d %s [%d]: %d elements differ" % (M, N, K, epi or "plain", t, int((x != y).sum()))


# (M, N, K, off): shapes the entry point hands to sbl_gemm2_f32
FORWARDED = [
    (256, 512, 64, 0),        # 2 * 8 * 16 = 256 workgroups on 32x32 tiles: not row-starved
    (33, 40, 520, 0),         # K % 16 == 8
    (33, 40, 48, 1),          # every operand one float past a 16-byte boundary
]


def note16(ops):
    """One launch of the 16x16 kernel (16 x 16 x 16), so that the route note of the call before is not 'forwarded'."""
    d = problem(16, 16, 16, "int")
    fr = [Frame(16, 16, NAN) for _ in (0, 1)]
    ops.call("sbl_gemm2_rows_f32", 16, 16, 16, P(d["A"][0]), P(d["A"][1]), 16 + PA, P(d["B"][0]), P(d["B"][1]), 16 + PB,
             fr[0].ptr(), fr[1].ptr(), fr[0].ld, None, None, 0, None, 0, S())
    assert last_route() == (G.ROUTE_FAMILY, G.TILE_16) + G.vu16(16)


@pytest.mark.parametrize("M,N,K,off", FORWARDED, ids=["%dx%dx%d_o%d" % f for f in FORWARDED])
def test_forwarded_is_gemm2(ops, M, N, K, off):
    """A call that does not qualify returns what sbl_gemm2_f32 returns, bit for bit (whole frames compared), runs the
    kernel family route_gemm2() predicts for it and is noted as forwarded - under f32 and bf16x6, right after a launch of the
    16x16 kernel (a stale route note would show)."""
    assert not G.takes16(M, N, K, K + PA, K + PB, off == 0)
    leaf = R.route_gemm2(M, N, K, K + PA, K + PB, off == 0, True, True, R.WS_FULL)
    ws = torch.zeros(R.WS_FULL // 4, dtype=torch.float32, device=DEV)
    keep, A, B, bias = [], [], [], []
    for t in (0, 1):
        tag = "%d.%dx%dx%d" % (t, M, N, K)
        ab, av = operand(fill("uni", "fwd.A" + tag, (M, K)), K + PA, off)
        bb, bv = operand(fill("uni", "fwd.B" + tag, (N, K)), K + PB, off)
        keep += [ab, bb]
        A.append(av)
        B.append(bv)
        bias.append(torch.from_numpy(fill("uni", "fwd.b" + tag, (N,))).to(DEV))
    for prec in ROUNDED_PRECS:
        ops.set_matmul_precision(prec)
        out = {}
        for name in ("sbl_gemm2_f32", "sbl_gemm2_rows_f32"):
            if name == "sbl_gemm2_rows_f32":
                note16(ops)
            fr = [Frame(M, N, NAN) for _ in (0, 1)]
            ops.call(name, M, N, K, P(A[0]), P(A[1]), K + PA, P(B[0]), P(B[1]), K + PB, fr[0].ptr(), fr[1].ptr(), fr[0].ld,
                     P(bias[0]), P(bias[1]), 1, ws.data_ptr(), R.WS_FULL, S())
            assert kid() == R.KERNEL_ID[leaf.family], (name, prec, kid(), leaf)
            out[name] = fr
        assert last_route() == (G.ROUTE_FAMILY, G.TILE_FORWARDED, 0, 0)
        for t in (0, 1):
            out["sbl_gemm2_rows_f32"][t].check_frame("forwarded %dx%dx%d [%d]" % (M, N, K, t))
            assert bool(torch.isfinite(out["sbl_gemm2_rows_f32"][t].out()).all())
            assert torch.equal(out["sbl_gemm2_f32"][t].buf, out["sbl_gemm2_rows_f32"][t].buf), "direction %d differs under %s" % (t, prec)
