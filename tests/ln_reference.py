"""Float64 reference and fp32 error model of the add + LayerNorm kernels (csrc/norm.hip, D = 512), shared by
tests/test_norm_elementwise_gpu.py and tests/test_decoder_rows_gpu.py.  Plain numpy; the derivation of every term is in
the docstring of test_norm_elementwise_gpu.py::test_add_layernorm_fwd_bwd."""
import numpy as np

U = 2.0 ** -24
LN_EPS = 1e-5


def f64(a):
    return np.asarray(a, dtype=np.float64)


def cdiv(a, b):
    return (a + b - 1) // b


def ln_geometry(M):
    """sbl_add_layernorm_bwd's host arithmetic: (rows per block, grid)."""
    blocks = max(1, min(cdiv(M, 32), 256))
    rpb = cdiv(cdiv(M, blocks), 16) * 16
    return rpb, cdiv(M, rpb)


def keep_scale(p):
    return np.float32(1) / (np.float32(1) - np.float32(p))


def ln_fwd_ref(x, res, gamma, beta, mask, p):
    """float64 LayerNorm(x * mask * scale + res) with the error model of the forward kernel (see test_add_layernorm_fwd_bwd):
    returns y, mean, rstd and their bounds, plus v, e_v (abs error of the kernel's v) for the backward's model."""
    xs = f64(x) * (mask * float(keep_scale(p))) if mask is not None else f64(x)
    v = xs + f64(res) if res is not None else xs
    e_v = U * ((np.abs(xs) if mask is not None else 0.0) + (np.abs(v) if res is not None else 0.0)) + np.zeros_like(v)
    mu = v.mean(1, keepdims=True)
    e_mu = e_v.mean(1, keepdims=True) + 9 * U * np.abs(v).mean(1, keepdims=True) + U * np.abs(mu)
    dc = v - mu
    e_d = e_v + e_mu + U * np.abs(dc)
    var = (dc * dc).mean(1, keepdims=True)
    rs = 1.0 / np.sqrt(var + float(np.float32(LN_EPS)))
    rel_rs = np.sqrt((e_d * e_d).mean(1, keepdims=True)) * rs + 9 * U
    g, b = f64(gamma), f64(beta)
    a = dc * rs * g
    y = a + b
    e_y = np.abs(g) * rs * e_d + np.abs(a) * (rel_rs + 2 * U) + U * (np.abs(a) + np.abs(b))
    return dict(y=y, e_y=e_y, mean=mu[:, 0], e_mean=e_mu[:, 0], rstd=rs[:, 0], e_rstd=(rel_rs * rs)[:, 0], v=v, e_v=e_v)


def ln_bwd_ref(dy, v, e_v, gamma, mean32, rstd32):
    """float64 dz and per-row terms of dgamma from the fp32 mean / rstd the kernel is given, with the backward's error model."""
    mu, rs, g, d = f64(mean32)[:, None], f64(rstd32)[:, None], f64(gamma), f64(dy)
    xh = (v - mu) * rs
    e_xh = rs * e_v + 2 * U * np.abs(xh)                                 # v - mu, * rstd
    gd = g * d
    s1 = gd.mean(1, keepdims=True)
    s2 = (gd * xh).mean(1, keepdims=True)
    e_s1 = 10 * U * np.abs(gd).mean(1, keepdims=True)                    # gamma * dy, then the 512-wide reduction
    e_s2 = (np.abs(gd) * e_xh).mean(1, keepdims=True) + 11 * U * np.abs(gd * xh).mean(1, keepdims=True)
    inner = gd - s1 - xh * s2
    dz = rs * inner
    e_dz = rs * (U * np.abs(gd) + e_s1 + np.abs(s2) * e_xh + np.abs(xh) * e_s2 + U * np.abs(xh * s2)
                 + 2 * U * (np.abs(gd) + np.abs(s1) + np.abs(xh * s2))) + U * np.abs(dz)
    t = d * xh                                                           # dgamma terms
    e_t = np.abs(d) * e_xh + U * np.abs(t)
    return dz, e_dz, t, e_t
