"""What a split-bf16 mode of the tile engine is DEFINED to compute, restated on the CPU in float64.

csrc/bf16_split.h splits every fp32 operand element by round-to-nearest-even casts, p0 = bf16(x), p1 = bf16(x - p0),
p2 = bf16(x - p0 - p1), and the kernels sum the plane products a_i * b_j with i + j <= planes - 1 in fp32 (products of two
bf16 values are exact in fp32).  torch.Tensor.bfloat16() rounds the same way, so a mode's result is an exact function of the
operands up to fp32 accumulation order, and a kernel compared with bilinear() owes only that accumulation error - the
tolerances of the f32 / bf16x6 parity tests apply unchanged to "bf16x3" and "bf16".
"""
import torch

PLANES = {"bf16": 1, "bf16x3": 2, "bf16x6": 3}


def planes(x, n):
    """The first n bf16 planes of a CPU float tensor, as fp32 tensors (every subtraction below is exact in fp32)."""
    r = x.detach().to(torch.float32)
    assert r.device.type == "cpu"
    out = []
    for _ in range(n):
        p = r.bfloat16().to(torch.float32)
        out.append(p)
        r = r - p
    return out


def terms(mode):
    """The plane pairs (i of operand a, j of operand b) a mode multiplies: all with i + j <= planes - 1."""
    n = PLANES[mode]
    return [(i, j) for i in range(n) for j in range(n) if i + j <= n - 1]


def bilinear(fn, a, b, mode):
    """sum over the mode's terms of fn(a_i, b_j) in float64; fn is bilinear in its two tensor arguments (a matmul, a
    convolution, a convolution's input or weight gradient).  mode "f32" is the unrounded float64 result."""
    if mode == "f32":
        return fn(a.detach().double(), b.detach().double())
    n = PLANES[mode]
    pa, pb = planes(a, n), planes(b, n)
    out = None
    for i, j in terms(mode):
        t = fn(pa[i].double(), pb[j].double())
        out = t if out is None else out + t
    return out


def fp32_emulation(a, b, mode, slab=16):
    """The product a @ b the way a kernel forms it: per 16-deep K slab, every term's plane product added into one fp32
    accumulator (torch's fp32 matmul stands in for the MFMA's own 16-term sum)."""
    n = PLANES[mode]
    pa, pb = planes(a, n), planes(b, n)
    acc = torch.zeros(a.size(0), b.size(1), dtype=torch.float32)
    for k0 in range(0, a.size(1), slab):
        for i, j in terms(mode):
            acc = acc + pa[i][:, k0:k0 + slab] @ pb[j][k0:k0 + slab]
    return acc
