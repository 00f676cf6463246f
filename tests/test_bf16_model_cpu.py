"""Pins tests/bf16_model.py - the CPU statement of the split-bf16 modes that test_reduced_precision_gpu.py holds the
kernels to - to the kernels' own definition (csrc/bf16_split.h), and shows that a comparison against it can fail."""
import os
import re

import numpy as np
import pytest
import torch

import bf16_model as BM
from sbl_for_multilingual_lip_reading_amd import detfill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT_H = os.path.join(ROOT, "sbl_for_multilingual_lip_reading_amd", "csrc", "bf16_split.h")

# M x N x K of the GEMM checks' table: a conv-sized K with a ragged tail, 63 slabs + 4, a long split-K product
SHAPES = [(100, 70, 36), (64, 64, 1012), (37, 96, 4096)]


def gemm_tol(K):
    return 4e-7 * max(K, 16) ** 0.5 * 4      # the tolerance of the f32 / bf16x6 GEMM and convolution parity tests


def U(name, shape):
    return torch.from_numpy(detfill.uniform(name, shape))


def test_plane_zero_is_the_round_to_nearest_even_cast():
    # exact ties of the 8-bit significand (1 + 2^-8 sits halfway between 1 and 1 + 2^-7): to even, both signs
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -20,
                      -0.3, 0.0, 3.0e-5, -1.0], dtype=torch.float32)
    p0 = BM.planes(x, 1)[0]
    assert torch.equal(p0, x.bfloat16().float())
    assert p0[:5].tolist() == [1.0, 1.0 + 2.0 ** -6, -1.0, -(1.0 + 2.0 ** -6), 1.0 + 2.0 ** -7]
    y = U("bm.p0", (4096,))
    assert bool((y < 0).any()) and torch.equal(BM.planes(y, 3)[0], y.bfloat16().float())
    # every plane is a bf16 value: its low 16 bits are zero
    for p in BM.planes(y, 3):
        assert int((p.view(torch.int32) & 0xFFFF).abs().max()) == 0


@pytest.mark.parametrize("kind", ["uniform", "normal"])
def test_three_planes_sum_back_bit_for_bit(kind):
    x = torch.from_numpy(getattr(detfill, kind)("bm.sum." + kind, (100000,)))
    p = BM.planes(x, 3)
    assert torch.equal((p[0] + p[1]) + p[2], x)                       # in fp32, the kernels' own order
    assert torch.equal((p[0].double() + p[1].double() + p[2].double()).float(), x)
    two = BM.planes(x, 2)
    assert torch.equal(two[0], p[0]) and torch.equal(two[1], p[1])
    assert float((x - two[0] - two[1]).abs().max()) <= 2.0 ** -16 * float(x.abs().max())


def test_term_counts():
    assert [len(BM.terms(m)) for m in ("bf16", "bf16x3", "bf16x6")] == [1, 3, 6]
    for m, n in BM.PLANES.items():
        t = BM.terms(m)
        assert len(set(t)) == len(t) and all(0 <= i < n and 0 <= j < n and i + j <= n - 1 for i, j in t)
        assert sorted(t) == sorted((j, i) for i, j in t)              # symmetric: operand order does not matter


def _ternary(expr, t):
    """Value of a C conditional chain `t == a ? x : t == b ? y : z` (the form of BfTerms' pa / pb) at t."""
    expr = expr.strip()
    if "?" not in expr:
        return int(expr)
    cond, rest = expr.split("?", 1)
    then, other = rest.split(":", 1)
    m = re.fullmatch(r"\s*t\s*==\s*(\d+)\s*", cond)
    assert m, cond
    return _ternary(then, t) if t == int(m.group(1)) else _ternary(other, t)


@pytest.mark.parametrize("nt,mode", [(3, "bf16x3"), (6, "bf16x6")])
def test_terms_agree_with_the_kernels_tables(nt, mode):
    src = open(SPLIT_H).read()
    body = re.search(r"struct BfTerms<%d>\s*\{(.*?)\n\};" % nt, src, re.S).group(1)
    npl, n = (int(v) for v in re.search(r"NPL\s*=\s*(\d+)\s*,\s*N\s*=\s*(\d+)", body).groups())
    pa = re.search(r"pa\(int t\)\s*\{\s*return\s+(.*?);\s*\}", body).group(1)
    pb = re.search(r"pb\(int t\)\s*\{\s*return\s+(.*?);\s*\}", body).group(1)
    pairs = [(_ternary(pa, t), _ternary(pb, t)) for t in range(n)]
    assert npl == BM.PLANES[mode] and n == nt == len(BM.terms(mode))
    assert sorted(pairs) == sorted(BM.terms(mode))


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_fp32_accumulation_stays_within_the_gemm_tolerance_and_a_dropped_tail_does_not(M, N, K):
    A, B = U("bm.A%d" % K, (M, K)), U("bm.B%d" % K, (K, N))
    exact = A.double() @ B.double()
    for mode in ("bf16", "bf16x3", "bf16x6"):
        model = BM.bilinear(torch.matmul, A, B, mode)
        emu = float((BM.fp32_emulation(A, B, mode).double() - model).abs().max())
        gap = float((model - exact).abs().max())
        dropped = float((BM.bilinear(torch.matmul, A[:, :K - 4], B[:K - 4], mode) - model).abs().max())
        print("%dx%dx%d %-6s fp32 emulation vs model %.2e / tol %.2e   model vs exact %.2e   last 4 of K dropped %.2e"
              % (M, N, K, mode, emu, gemm_tol(K), gap, dropped))
        assert emu < gemm_tol(K)
        assert dropped > 1000 * gemm_tol(K)          # a dropped K tail leaves the tolerance by orders of magnitude
        if mode != "bf16x6":
            assert gap > gemm_tol(K)                 # ... and a higher-precision mode than the named one is outside it too
    assert float((BM.bilinear(torch.matmul, A, B, "f32") - exact).abs().max()) == 0.0


def test_bilinear_takes_convolutions_and_their_gradients():
    import torch.nn.functional as F
    x, w = U("bm.cx", (2, 8, 5, 5)), U("bm.cw", (4, 8, 3, 3))
    y = BM.bilinear(lambda a, b: F.conv2d(a, b, None, 1, 1), x, w, "bf16x6")
    assert y.dtype == torch.float64 and float((y - F.conv2d(x.double(), w.double(), None, 1, 1)).abs().max()) < 1e-6
    dy = U("bm.cdy", tuple(y.shape))
    xr = x.double().requires_grad_(True)
    gx, = torch.autograd.grad(F.conv2d(xr, w.double(), None, 1, 1), xr, dy.double())
    dx = BM.bilinear(lambda g, b: torch.nn.grad.conv2d_input(x.shape, b, g, 1, 1), dy, w, "bf16x6")
    assert float((dx - gx).abs().max()) < 1e-6
    one = BM.bilinear(lambda a, b: F.conv2d(a, b, None, 1, 1), x, w, "bf16")
    assert torch.equal(one, F.conv2d(x.bfloat16().double(), w.bfloat16().double(), None, 1, 1))
    assert np.isfinite(float(one.sum()))
