"""The memory-bound kernels around the tile engine, one by one, against float64 at the edges of their launch geometry:
the BatchNorm family, add+LayerNorm (with its fused dropout), the label-smoothed cross entropy, Adam, and the small
elementwise kernels (row scale, positional-encoding add, average pool, dropout).

Every test drives the C ABI directly (ops.call) with tensors it allocates itself, and compares with a numpy float64
evaluation of the same formula on the same fp32 inputs (mean / invstd / rstd included where the kernel takes them as
inputs).  None of these kernels depends on the matmul precision, so the module pins "f32".

Tolerances are of two kinds only, both computed in the test from the float64 reference (U = 2^-24, the fp32 unit
roundoff; the derivation is in each test's docstring):
  * elementwise outputs: k * U * sum|terms of that element's formula|, k = the fp32 roundings on the kernel's path, plus
    9 * U * (reduced magnitude) for a value that went through a 512-wide reduction;
  * reductions of random data: depth * U * sum|t_i|, depth = the longest chain of fp32 additions one term goes through,
    from the launch geometry the test recomputes with the host code's own arithmetic.
What catches a dropped or doubled row is not those bounds but the exact checks: small-integer gradients (every fp32
partial sum is exact, so the result must EQUAL the integer column sum) and one-hot rows at the block boundaries.

`check()` prints the worst error / bound ratio of every comparison; the worst ratio measured on an MI355X is recorded
in each docstring ("measured").
"""
import functools

import numpy as np
import pytest
import torch

from conftest import maxdiff
from ln_reference import LN_EPS, keep_scale, ln_bwd_ref, ln_fwd_ref, ln_geometry
from sbl_for_multilingual_lip_reading_amd import detfill

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
EW_CAP = 8192 * 256          # work items one pass of ew_grid() covers


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


def cdiv(a, b):
    return (a + b - 1) // b


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
    print("%-44s worst err/bound %.3f  (max err %.3e)" % (what, worst, float(err.max()) if err.size else 0.0))
    assert worst <= 1.0, "%s: err/bound %.3f at %s" % (what, worst, np.unravel_index(int(ratio.argmax()), ratio.shape))
    return worst


def exact(what, got, ref):
    got = host(got) if hasattr(got, "detach") else np.asarray(got)
    ref = np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = int(np.count_nonzero(got != ref))
    assert bad == 0, "%s: %d of %d elements differ (max %.3e)" % (what, bad, ref.size, maxdiff(got, ref))


# --------------------------------------------------------------------------- BatchNorm
BN_SHAPES = [(1, 4), (37, 64), (54, 512), (131109, 64)]       # the last one: 131072 * 16 float4 = one grid pass, + 37 rows


@functools.lru_cache(maxsize=None)
def bn_data(rows, C):
    """Host inputs of one (rows, C) BatchNorm problem.  dy is small-integer valued; y (the ReLU's output as the backward
    sees it) is a multiple of 0.5 in [-1, 1], so it holds exact zeros and negatives for `!(y > 0)`."""
    d = {"x": u("bn.x", (rows, C)) * np.float32(2), "res": u("bn.res", (rows, C)),
         "dy": np.rint(u("bn.dy", (rows, C)) * np.float32(3)).astype(np.float32),
         "y": (np.rint(u("bn.y", (rows, C)) * np.float32(2)) / np.float32(2)).astype(np.float32),
         "mean": u("bn.mean", (C,)) * np.float32(0.3), "invstd": np.float32(0.5) + np.abs(u("bn.invstd", (C,))),
         "gamma": np.float32(1) + np.float32(0.2) * u("bn.gamma", (C,)), "beta": np.float32(0.1) * u("bn.beta", (C,))}
    assert (d["y"] == 0).any() or rows * C < 16
    return d


@functools.lru_cache(maxsize=4)
def bn_dev(rows, C):
    return {k: dev(v) for k, v in bn_data(rows, C).items()}


def bn_fwd_ref(x, res, mean, invstd, gamma, beta, relu):
    """float64 y and the elementwise bound: k * U * (|xhat * gamma| + |beta| + |res|)."""
    a = (f64(x) - f64(mean)) * f64(invstd) * f64(gamma)
    y = a + f64(beta)
    mag = np.abs(a) + np.abs(f64(beta))
    k = 4                                       # x - mean, * invstd, * gamma, + beta
    if res is not None:
        y = y + f64(res)
        mag = mag + np.abs(f64(res))
        k = 5                                   # + res
    if relu:
        y = np.maximum(y, 0.0)                  # 1-Lipschitz: the bound carries over
    return y, k * U * mag


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("with_res", [0, 1])
@pytest.mark.parametrize("rows,C", BN_SHAPES)
def test_bn_apply_fwd(ops, rows, C, with_res, relu):
    """y = [relu](gamma * (x - mean) * invstd + beta [+ res]) against float64.  Roundings on the kernel's path: the
    subtraction, two multiplications, the beta add and the residual add, so k = 4 (5 with res) times U times
    |xhat*gamma| + |beta| + |res|.  (131109, 64) takes every thread of the capped grid into a second trip.
    measured: worst err/bound 0.69."""
    h, d = bn_data(rows, C), bn_dev(rows, C)
    y = torch.full((rows, C), float("nan"), device=DEV)
    ops.call("sbl_bn_apply_fwd", P(d["x"]), P(d["res"]) if with_res else None, P(d["mean"]), P(d["invstd"]), P(d["gamma"]),
             P(d["beta"]), P(y), rows, C, relu, S())
    ref, bound = bn_fwd_ref(h["x"], h["res"] if with_res else None, h["mean"], h["invstd"], h["gamma"], h["beta"], relu)
    check("bn_apply_fwd y", y, ref, bound)


def bn_stats_ref(stats, count, rm, rv, momentum, eps):
    """bn_finalize's arithmetic in double: (mean, invstd, new running_mean, new running_var, raw variance)."""
    C = stats.size // 2
    mean = stats[:C] / float(count)
    raw = stats[C:] / float(count) - mean * mean
    var = np.maximum(raw, 0.0)
    invstd = 1.0 / np.sqrt(var + float(np.float32(eps)))
    mom = float(np.float32(momentum))
    unbiased = var * float(count) / float(count - 1) if count > 1 else var
    nrm = None if rm is None else (1.0 - mom) * f64(rm) + mom * mean
    nrv = None if rv is None else (1.0 - mom) * f64(rv) + mom * unbiased
    return mean, invstd, nrm, nrv, raw


def bn_make_stats(C, count):
    """float64 (sum, sumsq) of a made-up batch: mean 0.3u, variance 0.5 + |u|; channel 1 has mean 1000 and a sum of
    squares a hair below count * mean^2, so that sumsq / count - mean^2 comes out slightly negative."""
    m = f64(u("bns.m", (C,))) * 0.3
    var = 0.5 + np.abs(f64(u("bns.var", (C,))))
    m[1] = 1000.0
    stats = np.concatenate([count * m, count * (var + m * m)])
    stats[C + 1] = count * 1000.0 ** 2 * (1.0 - 1e-15)
    return stats


def rounded_once(what, got, ref):
    """A float32 that is the double `ref` rounded once: within half an ulp of it (the 1e-6 slack admits the last-bit
    difference between this double evaluation and the device's, which may contract a*b - c into one fma)."""
    return check(what, got, ref, U * np.abs(ref) * (1 + 1e-6) + 1e-45)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("with_res", [0, 1])
@pytest.mark.parametrize("rows,C", BN_SHAPES)
def test_bn_apply_fwd_stats(ops, rows, C, with_res, relu):
    """The training form: statistics supplied by the test in float64.  save_mean / save_invstd / running_mean / running_var
    must be the double-precision formula (momentum = the fp32 value promoted; unbiased variance, which at count = 1 - the
    (1, 4) case - falls back to the biased one) rounded once to fp32; num_batches_tracked goes up by exactly 1.  Channel 1
    carries a slightly negative sumsq/count - mean^2, so its invstd must be 1/sqrt(eps).  y is then held to
    test_bn_apply_fwd's bound with the kernel's own save_mean / save_invstd as the fp32 statistics (they were just
    checked), which also checks that every thread kept ITS channel quad through the grid-stride wrap.
    measured: worst err/bound 0.98 (statistics: the bound is half an ulp at the top of a binade), 0.72 (y)."""
    h, d = bn_data(rows, C), bn_dev(rows, C)
    count = rows
    stats = bn_make_stats(C, count)
    x = h["x"].copy()
    x[:, 1] += np.float32(1000)
    rm, rv = u("bns.rm", (C,)) * np.float32(0.1), np.float32(1) + np.float32(0.25) * np.abs(u("bns.rv", (C,)))
    momentum, eps = 0.1, 1e-5
    xd, sd, rmd, rvd = dev(x), dev(stats), dev(rm), dev(rv)
    nbt = torch.tensor([41], dtype=torch.int64, device=DEV)
    y = torch.full((rows, C), float("nan"), device=DEV)
    sm, si = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    ops.call("sbl_bn_apply_fwd_stats", P(xd), P(d["res"]) if with_res else None, P(sd), count, P(rmd), P(rvd), momentum, eps,
             P(d["gamma"]), P(d["beta"]), P(y), P(sm), P(si), P(nbt), rows, C, relu, S())
    mean, invstd, nrm, nrv, raw = bn_stats_ref(stats, count, rm, rv, momentum, eps)
    assert raw[1] < 0 and invstd[1] == 1.0 / np.sqrt(float(np.float32(eps)))
    rounded_once("bn_apply_fwd_stats save_mean", sm, mean)
    rounded_once("bn_apply_fwd_stats save_invstd", si, invstd)
    rounded_once("bn_apply_fwd_stats running_mean", rmd, nrm)
    rounded_once("bn_apply_fwd_stats running_var", rvd, nrv)
    assert int(nbt.item()) == 42
    ref, bound = bn_fwd_ref(x, h["res"] if with_res else None, host(sm), host(si), h["gamma"], h["beta"], relu)
    check("bn_apply_fwd_stats y", y, ref, bound)


def test_bn_apply_fwd_stats_accepts_null_running_statistics(ops):
    """running_mean = running_var = NULL (and no counter): save_mean / save_invstd / y as before, nothing else written."""
    rows, C = 37, 64
    h, d = bn_data(rows, C), bn_dev(rows, C)
    stats = bn_make_stats(C, rows)
    x = h["x"].copy()
    x[:, 1] += np.float32(1000)
    y = torch.full((rows, C), float("nan"), device=DEV)
    sm, si = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    xd, sd = dev(x), dev(stats)
    ops.call("sbl_bn_apply_fwd_stats", P(xd), None, P(sd), rows, None, None, 0.1, 1e-5, P(d["gamma"]), P(d["beta"]),
             P(y), P(sm), P(si), None, rows, C, 1, S())
    mean, invstd, _, _, _ = bn_stats_ref(stats, rows, None, None, 0.1, 1e-5)
    rounded_once("bn_apply_fwd_stats(null running) save_mean", sm, mean)
    rounded_once("bn_apply_fwd_stats(null running) save_invstd", si, invstd)
    ref, bound = bn_fwd_ref(x, None, host(sm), host(si), h["gamma"], h["beta"], 1)
    check("bn_apply_fwd_stats(null running) y", y, ref, bound)


@pytest.mark.parametrize("C", [64, 100])
@pytest.mark.parametrize("count", [1, 5000])
def test_bn_finalize_and_eval_stats(ops, C, count):
    """sbl_bn_finalize: the same double formulas rounded once (C = 100 is no multiple of its 64-lane block; null running
    statistics accepted).  sbl_bn_eval_stats is fp32: mean is a copy, invstd = 1 / sqrtf(rv + eps) has three roundings on
    one positive term, so 3 * U * |invstd|.
    measured: worst err/bound 0.99 (finalize), 0.42 (eval invstd)."""
    stats = bn_make_stats(C, count)
    rm, rv = u("bns.rm", (C,)) * np.float32(0.1), np.float32(1) + np.float32(0.25) * np.abs(u("bns.rv", (C,)))
    mean, invstd, nrm, nrv, raw = bn_stats_ref(stats, count, rm, rv, 0.1, 1e-5)
    assert raw[1] < 0
    sd = dev(stats)
    for running in (True, False):
        rmd, rvd = (dev(rm), dev(rv)) if running else (None, None)
        nbt = torch.tensor([7], dtype=torch.int64, device=DEV)
        sm, si = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
        ops.call("sbl_bn_finalize", P(sd), count, P(rmd), P(rvd), 0.1, 1e-5, P(sm), P(si), C, P(nbt), S())
        rounded_once("bn_finalize save_mean", sm, mean)
        rounded_once("bn_finalize save_invstd", si, invstd)
        if running:
            rounded_once("bn_finalize running_mean", rmd, nrm)
            rounded_once("bn_finalize running_var", rvd, nrv)
        assert int(nbt.item()) == 8
    em, ei = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    rmd, rvd = dev(rm), dev(rv)
    ops.call("sbl_bn_eval_stats", P(rmd), P(rvd), 1e-5, P(em), P(ei), C, S())
    exact("bn_eval_stats mean", em, rm)
    ref = 1.0 / np.sqrt(f64(rv) + float(np.float32(1e-5)))
    check("bn_eval_stats invstd", ei, ref, 3 * U * ref)


def bn_reduce_geometry(rows, C, ws):
    """sbl_bn_bwd_reduce's host arithmetic: (row groups per block, rows per block, grid)."""
    rg = 256 // (C // 4)
    blocks = min(cdiv(rows, 4 * rg), 512)
    if ws:
        blocks = min(blocks, 131072 // (2 * C))
    blocks = max(blocks, 1)
    rpb = cdiv(rows, blocks)
    return rg, rpb, cdiv(rows, rpb)


def bn_reduce_call(ops, d, sums, rows, C, relu, ws, dy=None):
    if ws == "lib":         # the calling stream's GEMM workspace, as ops.bn_bwd_reduce passes it
        wsp, wsb = ops._workspace().data_ptr(), ops.WS_BYTES
    elif ws == "short":     # counters only: no room for one partial row, so the call must fall back to atomics
        wsp, wsb = ops._workspace().data_ptr(), 16384
    else:
        wsp, wsb = None, 0
    ops.call("sbl_bn_bwd_reduce", P(d["dy"] if dy is None else dy), P(d["y"]) if relu else None, P(d["x"]), P(d["mean"]),
             P(d["invstd"]), P(sums), rows, C, relu, wsp, wsb, S())


BN_REDUCE_SHAPES = [(1, 4), (1000, 4), (1, 64), (63, 64), (600, 64), (32769 + 37, 64), (7, 512), (1025 + 3, 512), (4097 + 5, 512)]


@pytest.mark.parametrize("ws", ["lib", None, "short"])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("rows,C", BN_REDUCE_SHAPES)
def test_bn_bwd_reduce(ops, rows, C, relu, ws):
    """sums = (sum g, sum g * xhat) per channel, g = dy * [y > 0].  Regimes (asserted on the recomputed geometry): one
    block with only the tail loop, the 4-row unrolled loop plus tail, the 512-block cap, the workspace cap of 128 blocks
    at C = 512, the atomics path (no workspace, and a workspace too short for the partials), and the last block's
    combine with G = 256 / (C/2) = 128, 8 and 1 groups.
    dy is integer valued in -3..3: every fp32 partial and the double combine are exact, so sums[0:C] must EQUAL the
    integer column sums.  sums[C:2C]: a term g * (x - mean) * invstd carries 3 roundings, then passes through at most
    ceil(rows_per_block / rg) sequential per-lane additions and the rg additions of the block's LDS combine in fp32 (the
    rest is double), so depth = 3 + ceil(rpb / rg) + rg, bound depth * U * sum|t_i| per channel.
    With the workspace a second call must give bit-identical sums (the ticket re-arms, the order is fixed) and leave the
    counter region zero.
    measured: worst err/bound 0.20 (sums[C:2C])."""
    rg, rpb, grid = bn_reduce_geometry(rows, C, ws is not None)
    if (rows, C) == (1, 64):
        assert grid == 1 and rpb <= rg                      # tail loop only
    if (rows, C) == (63, 64):
        assert grid == 1 and rpb < 4 * rg                   # under 4 rows per lane: still no unrolled trip
    if (rows, C) == (600, 64):
        assert grid > 1 and rpb > 3 * rg                    # unrolled trips plus tail
    if (rows, C) == (32769 + 37, 64):
        assert cdiv(rows, 4 * rg) > 512 and grid <= 512
    if (rows, C) == (1025 + 3, 512):
        assert cdiv(rows, 4 * rg) > 128 and (grid <= 128 if ws else grid > 128)
    if (rows, C) == (4097 + 5, 512):
        assert cdiv(rows, 4 * rg) > 512 and (grid <= 128 if ws else 128 < grid <= 512)
    h, d = bn_data(rows, C), bn_dev(rows, C)
    sums = torch.full((2 * C,), float("nan"), dtype=torch.float64, device=DEV)
    bn_reduce_call(ops, d, sums, rows, C, relu, ws)
    g = f64(h["dy"]) * (h["y"] > 0) if relu else f64(h["dy"])
    t = g * (f64(h["x"]) - f64(h["mean"])) * f64(h["invstd"])
    exact("bn_bwd_reduce sums[0:C]", sums[:C], g.sum(0))
    depth = 3 + cdiv(rpb, rg) + rg
    check("bn_bwd_reduce sums[C:2C]", sums[C:], t.sum(0), depth * U * np.abs(t).sum(0))
    if ws == "lib":
        again = torch.full((2 * C,), float("nan"), dtype=torch.float64, device=DEV)
        bn_reduce_call(ops, d, again, rows, C, relu, ws)
        assert torch.equal(sums, again)
    if ws is not None:
        assert int(ops._workspace()[:4096].view(torch.int32).abs().max().item()) == 0


@pytest.mark.parametrize("rows,C,ws", [(600, 64, "lib"), (1025 + 3, 512, "lib"), (1025 + 3, 512, None), (32769 + 37, 64, "lib")])
def test_bn_bwd_reduce_one_hot_rows(ops, rows, C, ws):
    """dy is zero except one row r, r at the geometry's boundaries: 0, the last row of block 0, the first row of block 1,
    rows - 2, rows - 1 (asserted from the recomputed rows-per-block).  sums[0:C] must equal that row's g exactly;
    sums[C:2C] its g * xhat to the 3 roundings of the term (every other term is an exact zero).
    measured: worst err/bound 0.72."""
    rg, rpb, grid = bn_reduce_geometry(rows, C, ws is not None)
    assert grid >= 2 and (grid - 1) * rpb < rows <= grid * rpb
    h, d = bn_data(rows, C), bn_dev(rows, C)
    row = u("bn.onehot", (C,))
    for r in (0, rpb - 1, rpb, rows - 2, rows - 1):
        assert 0 <= r < rows
        assert (r // rpb == 0) if r < rpb else (r // rpb == 1 if r == rpb else r // rpb == grid - 1)
        dy = torch.zeros((rows, C), device=DEV)
        dy[r] = dev(row)
        sums = torch.full((2 * C,), float("nan"), dtype=torch.float64, device=DEV)
        bn_reduce_call(ops, d, sums, rows, C, 1, ws, dy=dy)
        g = f64(row) * (h["y"][r] > 0)
        t = g * (f64(h["x"][r]) - f64(h["mean"])) * f64(h["invstd"])
        exact("bn_bwd_reduce one-hot r=%d sums[0:C]" % r, sums[:C], g)
        check("bn_bwd_reduce one-hot r=%d sums[C:2C]" % r, sums[C:], t, 3 * U * np.abs(t))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("rows,C", BN_SHAPES)
def test_bn_bwd_apply(ops, rows, C, relu, accumulate):
    """dx = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat)) from the double sums the test supplies (the true sums of
    its integer-valued dy).  Roundings: the two means narrowed to fp32 (1 each), xhat (2) times the mean (1), two
    subtractions (2), gamma * invstd and the final product (2): at most 4 on a term, 2 on the running sum, 2 outside, so
    k = 8 times U * |gamma * invstd| * (|g| + |mean g| + |xhat * mean gx|).  dres must equal the masked dy exactly (it is
    skipped when NULL, the accumulate = 1 cases).  dbeta: integer sums, so accumulate = 0 (over NaN garbage) and
    accumulate = 1 (onto an integer preset) are both exact; dgamma: two roundings, 2 * U * (|preset| + |sum|).
    measured: worst err/bound 0.52 (dx), 0.90 (dgamma)."""
    h, d = bn_data(rows, C), bn_dev(rows, C)
    g = f64(h["dy"]) * (h["y"] > 0) if relu else f64(h["dy"])
    xhat = (f64(h["x"]) - f64(h["mean"])) * f64(h["invstd"])
    sums = np.concatenate([g.sum(0), (g * xhat).sum(0)])
    if accumulate:
        pre_b = np.rint(u("bn.preb", (C,)) * np.float32(9)).astype(np.float32)
        pre_g = u("bn.preg", (C,))
    else:
        pre_b = pre_g = np.full((C,), np.nan, dtype=np.float32)
    dgamma, dbeta, sd = dev(pre_g), dev(pre_b), dev(sums)
    dx = torch.full((rows, C), float("nan"), device=DEV)
    dres = None if accumulate else torch.full((rows, C), float("nan"), device=DEV)
    ops.call("sbl_bn_bwd_apply", P(d["dy"]), P(d["y"]) if relu else None, P(d["x"]), P(d["mean"]), P(d["invstd"]), P(d["gamma"]),
             P(sd), P(dx), P(dres), P(dgamma), P(dbeta), rows, C, relu, accumulate, S())
    mg, mx = sums[:C] / rows, sums[C:] / rows
    gi = f64(h["gamma"]) * f64(h["invstd"])
    ref = gi * (g - mg - xhat * mx)
    check("bn_bwd_apply dx", dx, ref, 8 * U * np.abs(gi) * (np.abs(g) + np.abs(mg) + np.abs(xhat * mx)))
    if dres is not None:
        exact("bn_bwd_apply dres", dres, g.astype(np.float32))
    base_b, base_g = (f64(pre_b), f64(pre_g)) if accumulate else (0.0, 0.0)
    exact("bn_bwd_apply dbeta", dbeta, (base_b + sums[:C]).astype(np.float32))
    check("bn_bwd_apply dgamma", dgamma, base_g + sums[C:], 2 * U * (np.abs(base_g) + np.abs(sums[C:])))


# --------------------------------------------------------------------------- add + LayerNorm (D = 512)
D = 512
LN_SEED = 0x1234ABCD5
LN_M = [1, 2, 17, 33, 4352, 8211]


def ln_inputs(M, kind):
    x = u("ln.x." + kind, (M, D)) * np.float32(2)
    res = u("ln.res." + kind, (M, D))
    if kind == "offcentre":      # row means near 50, standard deviation near 0.05: x + res has sigma^2 = (a^2 + b^2) / 3
        x = (np.float32(50) + np.float32(0.06) * u("ln.x." + kind, (M, D))).astype(np.float32)
        res = (np.float32(0.06) * res).astype(np.float32)
    gamma = np.float32(1) + np.float32(0.2) * u("ln.gamma", (D,))
    beta = np.float32(0.1) * u("ln.beta", (D,))
    dy = np.rint(u("ln.dy." + kind, (M, D)) * np.float32(3)).astype(np.float32)
    return x, res, gamma, beta, dy


def ln_mask(ops, M, p, seed, offset):
    """The keep mask of sbl_dropout at (seed, offset), recovered by running it over ones."""
    ones = torch.ones(M * D, device=DEV)
    out = torch.empty_like(ones)
    ops.call("sbl_dropout", P(ones), P(out), M * D, p, P(seed), offset, S())
    o = host(out).reshape(M, D)
    assert np.all((o == 0) | (o == keep_scale(p)))
    return o != 0


def ln_run(ops, x, res, gamma, beta, dy, p, offset, pre_g, pre_b):
    """Forward then backward through the C ABI; returns device outputs and the recovered mask (None without dropout)."""
    M = x.shape[0]
    seed = torch.tensor([LN_SEED], dtype=torch.int64, device=DEV)
    xd, rd, gd, bd, dyd = dev(x), (dev(res) if res is not None else None), dev(gamma), dev(beta), dev(dy)
    y = torch.full((M, D), float("nan"), device=DEV)
    mean, rstd = torch.full((M,), float("nan"), device=DEV), torch.full((M,), float("nan"), device=DEV)
    ops.call("sbl_add_layernorm_fwd", P(xd), P(rd), P(gd), P(bd), P(y), P(mean), P(rstd), M, D, LN_EPS, p, P(seed), offset, S())
    dz = torch.full((M, D), float("nan"), device=DEV)
    dxd = torch.full((M, D), float("nan"), device=DEV) if p > 0 else None
    dgamma, dbeta = dev(pre_g), dev(pre_b)
    ops.call("sbl_add_layernorm_bwd", P(dyd), P(xd), P(rd), P(gd), P(mean), P(rstd), P(dz), P(dxd), P(dgamma), P(dbeta), M, D,
             p, P(seed), offset, S())
    mask = ln_mask(ops, M, p, seed, offset) if p > 0 else None
    return dict(y=y, mean=mean, rstd=rstd, dz=dz, dx_drop=dxd, dgamma=dgamma, dbeta=dbeta, mask=mask)


def ln_check(ops, M, kind, with_res, p=0.0, offset=0, tag=""):
    x, res, gamma, beta, dy = ln_inputs(M, kind)
    res = res if with_res else None
    pre_g = u("ln.preg", (D,))
    pre_b = np.rint(u("ln.preb", (D,)) * np.float32(9)).astype(np.float32)
    o = ln_run(ops, x, res, gamma, beta, dy, p, offset, pre_g, pre_b)
    f = ln_fwd_ref(x, res, gamma, beta, o["mask"], p)
    tag = "ln[%d %s res=%d p=%g off=%d]%s " % (M, kind, with_res, p, offset, tag)
    check(tag + "y", o["y"], f["y"], f["e_y"])
    check(tag + "mean", o["mean"], f["mean"], f["e_mean"])
    check(tag + "rstd", o["rstd"], f["rstd"], f["e_rstd"])
    mean32, rstd32 = host(o["mean"]), host(o["rstd"])
    dz, e_dz, t, e_t = ln_bwd_ref(dy, f["v"], f["e_v"], gamma, mean32, rstd32)
    check(tag + "dz", o["dz"], dz, e_dz)
    if p > 0:
        dz32 = host(o["dz"])
        exact(tag + "dx_drop", o["dx_drop"], np.where(o["mask"], dz32 * keep_scale(p), np.float32(0)))
    exact(tag + "dbeta", o["dbeta"], (f64(pre_b) + f64(dy).sum(0)).astype(np.float32))
    rpb, grid = ln_geometry(M)
    depth = 1 + rpb // 8 + 8 + grid
    check(tag + "dgamma", o["dgamma"], f64(pre_g) + t.sum(0), depth * U * (np.abs(f64(pre_g)) + np.abs(t).sum(0)) + e_t.sum(0))
    return o["mask"]


@pytest.mark.parametrize("with_res", [0, 1])
@pytest.mark.parametrize("M", LN_M)
def test_add_layernorm_fwd_bwd(ops, M, with_res):
    """sbl_add_layernorm_fwd / _bwd at one row, a half-filled wave pair, one block with a clamped row (17), two blocks with
    a single row in the second (33), the stage-batched decoder's 4352 rows and the first odd size past the 256-block cap
    (8211: 48 rows per block), with and without the residual; asserted on the recomputed geometry.
    Forward model (v = x [* mask * scale] [+ res]): e_v = U per operation; the mean adds 9 * U * mean|v| (512-wide
    reduction) and its own rounding; e_d = e_v + e_mean + U|v - mean|; the variance is a sum of squares, so its relative
    error is 2 * rms(e_d) / sigma plus (9 + 2) * U, rstd takes half of that plus the eps add and rsqrtf (<= 9 * U in all);
    y = (v - mean) * rstd * gamma + beta adds two products and one sum.
    Backward model from the fp32 mean / rstd the kernel reads: xhat has e_v * rstd + 2 roundings; the two row means carry
    10 and 11 * U of their magnitude (product roundings + the 512-wide reduction) plus xhat's error; dz = rstd * (gamma dy
    - s1 - xhat * s2) adds one rounding per product and two for the subtractions.
    dy is integer valued: dbeta must EQUAL preset + the integer column sums (preset integer valued, every fp32 partial
    and float atomic exact).  dgamma: a term passes rows_per_block / 8 per-wave additions, 8 in the block's LDS combine
    and at most grid float atomics onto the preset, and is itself one product of xhat: depth = 1 + rpb/8 + 8 + grid,
    bound depth * U * (|preset| + sum|t_i|) + sum of the terms' own errors.
    measured over this test, the off-centre and the dropout cases: worst err/bound 0.21 (y), 0.18 (mean), 0.11 (rstd),
    0.59 (dz), 0.26 (dgamma)."""
    rpb, grid = ln_geometry(M)
    assert {1: (16, 1), 2: (16, 1), 17: (32, 1), 33: (32, 2), 4352: (32, 136), 8211: (48, 172)}[M] == (rpb, grid)
    if M == 33:
        assert M - (grid - 1) * rpb == 1        # the second block holds one row
    ln_check(ops, M, "plain", with_res)


@pytest.mark.parametrize("M", [33, 4352])
def test_add_layernorm_off_centre_rows(ops, M):
    """Row means near 50 with a standard deviation near 0.05: a one-pass variance would lose everything here.  The same
    model; its bound grows with |mean| * rstd through e_mean (9 * U * mean|v| against a spread of 0.05).
    measured: see test_add_layernorm_fwd_bwd."""
    x, res, _, _, _ = ln_inputs(M, "offcentre")
    v = f64(x) + f64(res)
    assert np.all(np.abs(v.mean(1) - 50) < 0.01) and np.all(np.abs(v.std(1) - 0.05) < 0.01)
    ln_check(ops, M, "offcentre", 1)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("M", [33, 4352])
def test_add_layernorm_fused_dropout(ops, M, p):
    """The fused masks must be sbl_dropout's at the same (seed, offset): the mask is recovered by running sbl_dropout over
    ones, the forward must equal LayerNorm(x * mask * scale + res) in float64, dz its float64 gradient, and dx_drop must
    EQUAL dz * mask * scale in fp32 (one multiplication).  A second offset gives another mask and passes the same checks.
    measured: see test_add_layernorm_fwd_bwd."""
    m0 = ln_check(ops, M, "plain", 1, p, offset=3)
    m1 = ln_check(ops, M, "plain", 1, p, offset=4)
    for m in (m0, m1):
        n = m.size
        assert abs(m.mean() - (1 - p)) < 5 * np.sqrt(p * (1 - p) / n)
    assert 0.5 * min(p, 1 - p) < np.mean(m0 != m1) < 1 - 0.5 * min(p, 1 - p)


@pytest.mark.parametrize("M", [33, 4352, 8211])
def test_add_layernorm_bwd_one_hot_rows(ops, M):
    """dy is zero except one row r at the boundaries of the backward's blocks (0, last row of block 0, first row of block
    1, M - 2, M - 1; asserted from the recomputed rows-per-block), dgamma / dbeta start at zero: dbeta must equal that row
    of dy exactly, dgamma its dy * xhat to the term's own error, and dz must be exactly zero on every other row.
    measured: worst err/bound 0.62 (dgamma), 0.24 (dz)."""
    rpb, grid = ln_geometry(M)
    assert grid >= 2 and (grid - 1) * rpb < M
    x, res, gamma, beta, _ = ln_inputs(M, "plain")
    row = u("ln.onehot", (D,))
    zero = np.zeros((D,), np.float32)
    f = ln_fwd_ref(x, res, gamma, beta, None, 0.0)
    for r in sorted({0, rpb - 1, rpb, M - 2, M - 1}):
        assert (r // rpb == 0) if r < rpb else (r // rpb == 1 if r == rpb else r // rpb == grid - 1)
        dy = np.zeros((M, D), np.float32)
        dy[r] = row
        o = ln_run(ops, x, res, gamma, beta, dy, 0.0, 0, zero, zero)
        dz, e_dz, t, e_t = ln_bwd_ref(dy, f["v"], f["e_v"], gamma, host(o["mean"]), host(o["rstd"]))
        assert np.count_nonzero(e_dz[np.arange(M) != r]) == 0
        check("ln one-hot[%d] r=%d dz" % (M, r), o["dz"], dz, e_dz)
        exact("ln one-hot[%d] r=%d dbeta" % (M, r), o["dbeta"], row)
        check("ln one-hot[%d] r=%d dgamma" % (M, r), o["dgamma"], t[r], e_t[r])


# --------------------------------------------------------------------------- label-smoothed cross entropy
IGNORE = -1


def ce_inputs(R, C, scale, ignore):
    pred = (u("ce.pred", (R, C)) * np.float32(scale)).astype(np.float32)
    gold = np.minimum(((f64(u("ce.gold", (R,))) + 1) * 0.5 * C).astype(np.int64), C - 1)
    if C >= 2:        # ties for the maximum: the first index must win, so gold = first counts and gold = second does not
        pairs = [(0, min(5, C - 2), C - 1, 0), (2, min(5, C - 2), C - 1, 1), (4, 6 % (C - 1), C - 1 if C < 72 else 70, 1)]
        for r, a, b, pick in pairs:
            if r < R:
                pred[r, a] = pred[r, b] = np.float32(scale + 1)
                gold[r] = (a, b)[pick]
    if ignore == "half":
        gold[1::2] = IGNORE
    elif ignore == "all_but_one":
        gold[1:] = IGNORE
    return pred, gold


def ce_ref(pred, gold, eps32, gscale32):
    """float64 (loss rows, dpred) of loss.py's smoothed loss, with the kernels' error model (see the test's docstring)."""
    R, C = pred.shape
    eps, gs = float(eps32), float(gscale32)
    valid = gold != IGNORE
    p = f64(pred)
    mx = p.max(1, keepdims=True)
    dlt = p - mx
    e = np.exp(dlt)
    se = e.sum(1, keepdims=True)
    sm = e / se
    lse = np.log(se) + mx
    onehot = np.zeros((R, C), bool)
    onehot[np.arange(R)[valid], gold[valid]] = True
    q = np.where(onehot, 1.0 - eps, eps / C)
    rows = -(q * (p - lse)).sum(1)
    trips = cdiv(C, 64)
    rel_exp = (2 * np.abs(dlt) + 2) * U                  # pred - max, * log2(e), v_exp_f32 (1 ulp = 2 U)
    rel_se = (sm * rel_exp).sum(1, keepdims=True) + (trips + 6) * U
    e_lse = 3 * U * np.abs(np.log(se)) + rel_se + U * np.abs(lse)     # v_log_f32 (1 ulp) * ln 2, the sum's error, + max
    e_rows = (q * (e_lse + U * np.abs(p - lse)) + 2 * U * np.abs(q * (p - lse))).sum(1) \
        + (trips + 6) * U * np.abs(q * (p - lse)).sum(1)
    nvalid = int(valid.sum())
    qsum = (1.0 - eps) + (C - 1) * eps / C
    scale = gs / max(nvalid, 1)
    dpred = np.where(valid[:, None], scale * (qsum * sm - q), 0.0)
    e_dpred = np.where(valid[:, None], scale * (qsum * sm * (rel_exp + rel_se + 7 * U) + 4 * U * q) + 2 * U * scale * (qsum * sm + q), 0.0)
    return np.where(valid, rows, 0.0), np.where(valid, e_rows, 0.0), dpred, e_dpred, nvalid


@pytest.mark.parametrize("ignore", ["none", "half", "all_but_one"])
@pytest.mark.parametrize("C", [1, 58, 64, 65, 200])
@pytest.mark.parametrize("R", [1, 5, 64, 4099])
def test_smoothed_ce(ops, R, C, ignore):
    """sbl_smoothed_ce_fwd / _bwd for eps in {0, 0.1}, logits in +-3 and +-30, gscale in {1, 0.37}: one, exactly one and more
    than one lane trip per row (C = 58, 64, 65 / 200), rows that do not fill the last 4-row block, ignored rows (their
    dpred must be exactly zero), planted ties for the maximum (correct count by torch.argmax's first-index rule).
    The kernels use __expf / __logf, whose error the ROCm documentation on the build machine does not state; the model
    below takes the hardware transcendental instructions at 1 ulp (2 * U) and counts the roundings around them:
    exp(d), d = pred - max: U|d| for the subtraction, U|d| for the product with log2(e), 2 * U for v_exp_f32, so
    rel_exp = (2|d| + 2) * U; the row's sum of exponentials adds ceil(C/64) + 6 additions; log: 3 * U * |ln se|.
    dpred = scale * (qsum * softmax - q): rel_exp + rel_se + 7 roundings (division, qsum's four, two products) on the
    softmax term, 4 on q, and 2 more on the result.  The loss sum is one float atomic per valid row: nvalid * U * sum|loss
    rows| on top of the rows' own errors.  valid and correct counts are exact.
    measured: worst err/bound 0.80 (dpred), 0.26 (loss sum): the 1-ulp model of the two instructions holds."""
    for scale in (3.0, 30.0):
        pred, gold = ce_inputs(R, C, scale, ignore)
        pd, gd = dev(pred), dev(gold)
        valid = gold != IGNORE
        am = torch.argmax(torch.from_numpy(pred), dim=1).numpy()
        ncorrect = int(np.count_nonzero(valid & (am == gold)))
        if C >= 2 and ignore == "none" and R >= 5:
            assert am[0] == gold[0] and am[2] != gold[2] and am[4] != gold[4]
        for eps in (0.0, 0.1):
            eps32 = np.float32(eps)
            out3 = torch.full((3,), float("nan"), device=DEV)
            ops.call("sbl_smoothed_ce_fwd", P(pd), P(gd), P(out3), R, C, eps, IGNORE, S())
            for gscale in (1.0, 0.37):
                gs32 = np.float32(gscale)
                gsd = dev(np.array([gs32], np.float32))
                dpred = torch.full((R, C), float("nan"), device=DEV)
                ops.call("sbl_smoothed_ce_bwd", P(pd), P(gd), P(out3), P(gsd), P(dpred), R, C, eps, IGNORE, S())
                rows, e_rows, ref, e_ref, nvalid = ce_ref(pred, gold, eps32, gs32)
                tag = "ce[R=%d C=%d %s s=%g eps=%g gs=%g] " % (R, C, ignore, scale, eps, gscale)
                check(tag + "dpred", dpred, ref, e_ref)
                assert np.count_nonzero(host(dpred)[~valid]) == 0
            o = host(out3)
            assert o[1] == nvalid and o[2] == ncorrect, (o, nvalid, ncorrect)
            check(tag + "loss sum", o[:1], [rows.sum()], [e_rows.sum() + nvalid * U * np.abs(rows).sum()])


# --------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("n", [1, 257, EW_CAP + 333])
def test_adam_step(ops, n):
    """torch.optim.Adam's update (m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2; p -= lr / (1 - b1^t) * m / (sqrt(v) /
    sqrt(1 - b2^t) + eps)) in float64 from the same fp32 p, g, m, v, at step 1, 2 and 10000 and grad_scale 1 and 1/8;
    n = 2,097,152 + 333 takes the capped grid into a second trip.  Roundings: g * scale (1); m: 1 - b1, two products, one
    sum on top: 4 * U * (|b1 m| + |(1 - b1) g|); v: g's rounding twice, 1 - b2, three products, one sum: 7 * U * (b2 v + (1 -
    b2) g^2).  The denominator inherits half of v's relative error (<= 3.5 U) and adds sqrt, the bias factor, a product and a
    sum (4), the update the step size, a product and a division (3): |update| * 10.5 * U plus m's error through the same
    quotient, and the final subtraction U * (|p| + |update|).  A block of entries has g = m = v = 0: bound 0, so they must
    come back bit-identical (and finite).
    measured: worst err/bound 0.996 (p: where the update is far below p's ulp the final rounding IS the bound), 0.48 (m),
    0.38 (v)."""
    b1, b2, eps, lr = np.float32(0.9), np.float32(0.98), np.float32(1e-9), np.float32(1e-3)
    p0 = u("adam.p", (n,))
    g0 = u("adam.g", (n,)) * np.float32(0.01)
    m0 = u("adam.m", (n,)) * np.float32(0.01)
    v0 = (u("adam.v", (n,)) * np.float32(0.01)) ** 2
    if n > 40:
        g0, m0, v0 = g0.copy(), m0.copy(), v0.copy()
        g0[3:40] = m0[3:40] = v0[3:40] = 0
    gd = dev(g0)
    for step in (1, 2, 10000):
        for gscale in (1.0, 0.125):
            pd, md, vd = dev(p0), dev(m0), dev(v0)
            ops.call("sbl_adam_step", P(pd), P(gd), P(md), P(vd), n, float(lr), float(b1), float(b2), float(eps), step, gscale, S())
            B1, B2 = float(b1), float(b2)
            g = f64(g0) * gscale
            m = B1 * f64(m0) + (1 - B1) * g
            v = B2 * f64(v0) + (1 - B2) * g * g
            e_m = 4 * U * (np.abs(B1 * f64(m0)) + np.abs((1 - B1) * g))
            e_v = 7 * U * (B2 * f64(v0) + (1 - B2) * g * g)
            ss = float(lr) / (1 - B1 ** step)
            den = np.sqrt(v) / np.sqrt(1 - B2 ** step) + float(eps)
            upd = ss * m / den
            p = f64(p0) - upd
            e_p = np.abs(upd) * 10.5 * U + ss * e_m / den + U * (np.abs(f64(p0)) + np.abs(upd))
            e_p = np.where(upd == 0, 0.0, e_p)
            tag = "adam[n=%d step=%d gs=%g] " % (n, step, gscale)
            check(tag + "m", md, m, e_m)
            check(tag + "v", vd, v, e_v)
            check(tag + "p", pd, p, e_p)
            if n > 40:
                exact(tag + "zero-gradient block", pd[3:40], p0[3:40])


# --------------------------------------------------------------------------- small elementwise kernels
@pytest.mark.parametrize("M,Dm", [(37, 20), (EW_CAP // 128 + 3, 512)])
def test_rowscale(ops, M, Dm):
    """y[m, :] = x[m, :] * s[m]: one fp32 product, so it must equal numpy's fp32 product bit for bit; (16387, 512) is three
    rows past one pass of the capped grid."""
    assert M * (Dm // 4) > EW_CAP or M == 37
    x, s = u("rs.x", (M, Dm)), u("rs.s", (M,))
    y = torch.full((M, Dm), float("nan"), device=DEV)
    xd, sd = dev(x), dev(s)
    ops.call("sbl_rowscale", P(xd), P(sd), P(y), M, Dm, S())
    exact("rowscale", y, x * s[:, None])


@pytest.mark.parametrize("B,L,Dm", [(3, 29, 20), (566, 29, 512)])
def test_add_pe(ops, B, L, Dm):
    """y[b, l, :] = x[b, l, :] + pe[l, :], exact in fp32.  L = 29 divides neither the 256-lane block nor the grid stride;
    (566, 29, 512) is 2,100,992 float4s, just past one pass."""
    assert B * L * (Dm // 4) > EW_CAP or B == 3
    assert (8192 * 256) % (L * (Dm // 4)) != 0
    x, pe = u("pe.x", (B, L, Dm)), u("pe.pe", (L, Dm))
    y = torch.full((B, L, Dm), float("nan"), device=DEV)
    xd, ped = dev(x), dev(pe)
    ops.call("sbl_add_pe", P(xd), P(ped), P(y), B, L, Dm, S())
    exact("add_pe", y, x + pe[None])


@pytest.mark.parametrize("NIMG,C,HW", [(3, 20, 1), (3, 20, 9), (5, 64, 30), (2049, 512, 9)])
def test_avgpool(ops, NIMG, C, HW):
    """Global average pool over NHWC.  Forward: HW sequential fp32 additions then one division: (HW * U * sum|x_p|) / HW +
    U * |y| (exact at HW = 1).  Backward: dy * (1 / HW) with the reciprocal rounded to fp32 first: bit-identical to numpy's
    fp32 evaluation.  (2049, 512, 9) is 512 outputs past the forward's 4096-block cap (and nine times past the backward's).
    measured: worst err/bound 0.45."""
    assert NIMG * C > 4096 * 256 or NIMG < 10
    x, dy = u("ap.x", (NIMG, HW, C)), u("ap.dy", (NIMG, C))
    y = torch.full((NIMG, C), float("nan"), device=DEV)
    xd, dyd = dev(x), dev(dy)
    ops.call("sbl_avgpool_fwd", P(xd), P(y), NIMG, HW, C, S())
    ref = f64(x).mean(1)
    if HW == 1:
        exact("avgpool_fwd", y, x[:, 0])
    else:
        check("avgpool_fwd", y, ref, U * np.abs(f64(x)).sum(1) + U * np.abs(ref))
    dx = torch.full((NIMG, HW, C), float("nan"), device=DEV)
    ops.call("sbl_avgpool_bwd", P(dyd), P(dx), NIMG, HW, C, S())
    inv = np.float32(1) / np.float32(HW)
    exact("avgpool_bwd", dx, np.broadcast_to((dy * inv)[:, None, :], (NIMG, HW, C)))


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_dropout(ops, p):
    """sbl_dropout at n = 2,097,152 + 333 (past one pass of the capped grid): p = 0 is the identity; otherwise every value
    is 0 or x * (1 / (1 - p)) in fp32, the keep fraction is within 5 binomial standard deviations of 1 - p (also on the
    wrapped tail alone), the same (seed, offset) gives the same mask and another offset or seed a different one."""
    n = EW_CAP + 333
    x = u("do.x", (n,))
    x = np.where(x == 0, np.float32(0.5), x)
    xd = dev(x)
    seed = torch.tensor([0x5B1C0FFEE], dtype=torch.int64, device=DEV)

    def run(sd, offset):
        y = torch.full((n,), float("nan"), device=DEV)
        ops.call("sbl_dropout", P(xd), P(y), n, p, P(sd), offset, S())
        return host(y)

    y = run(seed, 5)
    if p == 0.0:
        exact("dropout p=0", y, x)
        return
    keep = y != 0
    exact("dropout values", y, np.where(keep, x * keep_scale(p), np.float32(0)))
    assert abs(keep.mean() - (1 - p)) < 5 * np.sqrt(p * (1 - p) / n)
    assert abs(keep[:EW_CAP].mean() - (1 - p)) < 5 * np.sqrt(p * (1 - p) / EW_CAP)
    assert 0 < keep[EW_CAP:].sum() < 333
    exact("dropout replay", run(seed, 5), y)
    lo, hi = p * (1 - p), 3 * p * (1 - p)            # two independent masks differ on a fraction 2 p (1 - p)
    assert lo < np.mean((run(seed, 6) != 0) != keep) < hi
    assert lo < np.mean((run(seed + 1, 5) != 0) != keep) < hi
