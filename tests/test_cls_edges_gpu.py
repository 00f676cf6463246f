"""The four stage-1 classification entry points of csrc/cls_head.hip (sbl_cls_head_fwd, sbl_cls_loss_fwd, sbl_cls_loss_bwd,
sbl_cls_head_bwd), one by one through the C ABI, against tests/cls_reference.py at the edges of the kernel's tiles: the
8-class slice, the 4-clip input-gradient group, the 512-class LDS chunk and its 128-class wavefront quarters (empty ones
included), the 64-clip pass of the logits kernel, the 256-clip chunk of the dW1 / db1 loop, the 16 wavefronts of the loss
forward and the 4 rows per workgroup of the loss backward.

Every test drives ops.call with tensors it allocates itself.  Outputs are pre-filled with NaN (with the integer or real
preset where accumulate = 1 adds to them, and d_enc with a preset there too, so that a `+=` shows), so an element the kernel
does not write fails the comparison.  The heads are plain fp32 FMA in every matmul precision; the module pins "f32" and the
repeatability test switches to "bf16x6" itself.

Comparisons are of two kinds, both from cls_reference:
  * exact(): integer operands (-3..3, T in {1, 2, 4}) keep every product, partial sum and quotient a float32, so the result
    equals the float64 reference bit for bit whatever the summation order;
  * check() at 2x the bound cls_reference derives for that element from the case's own operands (the factor 2: the GPU's
    expf / logf against the host's by an ulp).  check() prints the worst error / bound ratio of every comparison.
The worst ratios measured on an MI355X (against 1x the bound) are in the docstrings of the bounded tests.
"""
import numpy as np
import pytest
import torch

import cls_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GPU_FACTOR = 2.0
ids = lambda cases: [c["id"] for c in cases]


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
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def P(t):
    return None if t is None else t.data_ptr()


def S():
    return torch.cuda.current_stream().cuda_stream


def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def operands(o):
    return {k: dev(o[k]) for k in ("enc", "w1", "b1", "w2", "b2", "d1", "d2")}


def run_fwd(ops, g, case):
    N, C1, C2, T, li = (case[k] for k in ("N", "C1", "C2", "T", "li"))
    out = {"pooled": nan(N, R.D), "pooled_t": nan(R.D, N), "logits1": nan(N, C1), "logits2": nan(N, C2)}
    ops.call("sbl_cls_head_fwd", P(g["enc"]), P(g["w1"]), P(g["b1"]), P(g["w2"]), P(g["b2"]), P(out["pooled"]),
             P(out["pooled_t"]), P(out["logits1"]), P(out["logits2"]), N, T, R.D, C1, C2, li, S())
    torch.cuda.synchronize()
    return out


def run_bwd(ops, g, case, pooled, want, accumulate, preset):
    """Calls sbl_cls_head_bwd with the outputs in `want` (the others NULL).  Returns all five buffers, pre-filled with the
    preset when accumulate = 1 and with NaN otherwise, and a copy of the pre-fill."""
    N, C1, C2, T, li = (case[k] for k in ("N", "C1", "C2", "T", "li"))
    shapes = {"d_enc": (N, T, R.D), "dW1": (C1, R.D), "db1": (C1,), "dW2": (C2, R.D), "db2": (C2,)}
    buf = {k: (dev(preset[k]) if accumulate else nan(*s)) for k, s in shapes.items()}
    before = {k: v.clone() for k, v in buf.items()}
    ops.call("sbl_cls_head_bwd", P(g["enc"]), P(pooled), P(g["d1"]), P(g["d2"]), P(g["w1"]), P(g["w2"]),
             *[P(buf[k]) if k in want else None for k in R.OUT_BWD], N, T, R.D, C1, C2, li, accumulate, S())
    torch.cuda.synchronize()
    return buf, before


def untouched(what, buf, before):
    """Bitwise the pre-fill (NaN included)."""
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), what + ": an output that was not asked for changed"


def run_loss(ops, o, lw, gscale=None, ignore_id=R.IGN):
    """sbl_cls_loss_fwd, then (gscale given) sbl_cls_loss_bwd on the forward's stats.  Host arrays."""
    l1, l2, t1, t2 = dev(o["l1"]), dev(o["l2"]), dev(o["t1"]), dev(o["t2"])
    (N, C1), C2 = l1.shape, l2.shape[1]
    loss, stats = nan(1), nan(6)
    ops.call("sbl_cls_loss_fwd", P(l1), P(l2), P(t1), P(t2), N, C1, C2, float(lw), ignore_id, P(loss), P(stats), S())
    torch.cuda.synchronize()
    out = {"loss": host(loss)[0], "stats": host(stats)}
    if gscale is not None:
        gs, d1, d2 = dev(np.float32([gscale])), nan(N, C1), nan(N, C2)
        ops.call("sbl_cls_loss_bwd", P(l1), P(l2), P(t1), P(t2), P(stats), P(gs), P(d1), P(d2), N, C1, C2, float(lw),
                 ignore_id, S())
        torch.cuda.synchronize()
        out["d1"], out["d2"] = host(d1), host(d2)
    return out


def check_loss_fwd(tag, got, fw):
    R.exact("counts [%s]" % tag, got["stats"][[1, 2, 4, 5]], fw["stats"][[1, 2, 4, 5]])
    for i in (0, 3):
        R.check("stats[%d] [%s]" % (i, tag), got["stats"][i], fw["stats"][i], fw["b_stats"][i], GPU_FACTOR)
    R.check("loss [%s]" % tag, got["loss"], fw["loss"], fw["b_loss"], GPU_FACTOR)


def check_loss_bwd(tag, got, bw, o, heads=(1, 2)):
    for h in heads:
        k = "d%d" % h
        R.check("dlogits%d [%s]" % (h, tag), got[k], bw[k], bw["b_" + k], GPU_FACTOR, rows=bw["rows%d" % h])
        ign = o["t%d" % h] == R.IGN
        assert not got[k][ign].any(), "%s: an ignored row of head %d is not 0" % (tag, h)


# --------------------------------------------------------------------------- heads, exact
@pytest.mark.parametrize("case", R.HEAD_EXACT, ids=ids(R.HEAD_EXACT))
def test_head_exact(ops, case):
    """Integer operands: pooled, pooled_t, both logits and the five gradients equal the reference bit for bit, with
    accumulate = 0 onto NaN and accumulate = 1 onto integer presets (d_enc is written over its preset)."""
    o = R.exact_head_case(case)
    g = operands(o)
    li = case["li"]
    fw = R.head_fwd(o["enc"], o["w1"], o["b1"], o["w2"], o["b2"], li)
    out = run_fwd(ops, g, case)
    for k in R.OUT_FWD:
        R.exact("%s [%s]" % (k, case["id"]), out[k], fw[k])
    for acc in (0, 1):
        ref = R.head_bwd(o["enc"], host(out["pooled"]), o["d1"], o["d2"], o["w1"], o["w2"], li, accumulate=acc, preset=o["preset"])
        buf, _ = run_bwd(ops, g, case, out["pooled"], R.OUT_BWD, acc, o["preset"])
        for k in R.OUT_BWD:
            R.exact("%s acc=%d [%s]" % (k, acc, case["id"]), buf[k], ref[k])


@pytest.mark.parametrize("acc", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("combo", list(R.NULL_COMBOS), ids=list(R.NULL_COMBOS))
@pytest.mark.parametrize("case", R.HEAD_NULL, ids=ids(R.HEAD_NULL))
def test_head_bwd_null_outputs(ops, case, combo, acc):
    """The NULL-output combinations the header allows: what is asked for equals the full call's result bit for bit, what is
    not keeps its pre-fill."""
    want = R.NULL_COMBOS[combo]
    o = R.exact_head_case(case)
    g = operands(o)
    pooled = dev(R.f32(R.head_fwd(o["enc"], o["w1"], o["b1"], o["w2"], o["b2"], case["li"])["pooled"]))
    ref = R.head_bwd(o["enc"], host(pooled), o["d1"], o["d2"], o["w1"], o["w2"], case["li"], want=want, accumulate=acc,
                     preset=o["preset"])
    assert set(ref) == set(want)
    buf, before = run_bwd(ops, g, case, pooled, want, acc, o["preset"])
    for k in R.OUT_BWD:
        if k in want:
            R.exact("%s %s acc=%d [%s]" % (k, combo, acc, case["id"]), buf[k], ref[k])
        else:
            untouched("%s %s acc=%d [%s]" % (k, combo, acc, case["id"]), buf[k], before[k])


def test_head_bwd_without_outputs_is_a_no_op(ops):
    case = R.HEAD_NULL[0]
    o = R.exact_head_case(case)
    g = operands(o)
    buf, before = run_bwd(ops, g, case, dev(R.f32(o["enc"].mean(1))), (), 0, o["preset"])
    for k in R.OUT_BWD:
        untouched(k, buf[k], before[k])


# --------------------------------------------------------------------------- heads, float64 bounds
@pytest.mark.parametrize("case", R.HEAD_REAL, ids=ids(R.HEAD_REAL))
def test_head_real(ops, case):
    """randn operands with rows scaled across 2^-6 .. 2^6 and T in {3, 31}: every element of every output within 2x its own
    bound.  The backward reference takes the pooled buffer the kernel is handed (the forward's).
    measured (err / 1x bound, worst over the table): pooled 0.60, logits1 0.002, logits2 0.001, d_enc 0.24, dW1 0.35,
    db1 0.25, dW2 0.32, db2 0.16 (the term counts of the long sums are worst cases the tree-shaped sums stay far below)."""
    o = R.real_head_case(case)
    g = operands(o)
    li = case["li"]
    args = (o["enc"], o["w1"], o["b1"], o["w2"], o["b2"], li)
    fw, fb = R.head_fwd(*args), R.head_fwd_bounds(*args)
    out = run_fwd(ops, g, case)
    for k in R.OUT_FWD:
        R.check("%s [%s]" % (k, case["id"]), out[k], fw[k], fb[k], GPU_FACTOR)
    assert torch.equal(out["pooled_t"], out["pooled"].t())
    pooled = host(out["pooled"])
    for acc in (0, 1):
        bargs = (o["enc"], pooled, o["d1"], o["d2"], o["w1"], o["w2"], li)
        ref = R.head_bwd(*bargs, accumulate=acc, preset=o["preset"])
        bound = R.head_bwd_bounds(*bargs, accumulate=acc, preset=o["preset"])
        buf, _ = run_bwd(ops, g, case, out["pooled"], R.OUT_BWD, acc, o["preset"])
        for k in R.OUT_BWD:
            R.check("%s acc=%d [%s]" % (k, acc, case["id"]), buf[k], ref[k], bound[k], GPU_FACTOR)


# --------------------------------------------------------------------------- loss
@pytest.mark.parametrize("case", R.LOSS_CASES, ids=ids(R.LOSS_CASES))
def test_loss_case(ops, case):
    """Counts exact; loss sums and loss within 2x their bounds; every dlogits element within 2x B_d; ignored rows exactly 0;
    gscale = 0 gives +-0 everywhere.
    measured (err / 1x bound, worst over the table): loss 0.09, stats[0] 0.10, stats[3] 0.12, dlogits1 0.79,
    dlogits2 0.73 (the float32 restatement on the CPU: row loss 0.72, dlogits 0.79)."""
    o = R.loss_case(case)
    got = run_loss(ops, o, case["lw"], case["gscale"])
    check_loss_fwd(case["id"], got, R.loss_fwd(o["l1"], o["l2"], o["t1"], o["t2"], case["lw"]))
    check_loss_bwd(case["id"], got, R.loss_bwd(o["l1"], o["l2"], o["t1"], o["t2"], case["lw"], case["gscale"]), o)
    if case["gscale"] == 0.0:
        assert not got["d1"].any() and not got["d2"].any()
    if case["lw"] == 0.0:
        assert not got["d2"].any()


@pytest.mark.parametrize("target", ["lower", "higher"])
@pytest.mark.parametrize("C1,C2", [(1500, 65), (65, 1500)], ids=["C1500x65", "C65x1500"])
def test_argmax_ties_go_to_the_lowest_index(ops, C1, C2, target):
    """Equal maxima at neighbours (5, 6), in one lane over two passes (5, 69: the in-lane tie), with the lower index in the
    higher lane (64, 1: the cross-lane tie) and at the two ends (0, C - 1): `correct` counts a row only when the target is
    the lower of the two."""
    o = R.tie_case(C1, C2, target)
    n = len(o["t1"])
    fw = R.loss_fwd(o["l1"], o["l2"], o["t1"], o["t2"], 0.1)
    assert fw["stats"][[1, 2, 4, 5]].tolist() == ([n, n, n, n] if target == "lower" else [n, 0, n, 0])
    got = run_loss(ops, o, 0.1, 1.0)
    tag = "ties C%dx%d %s" % (C1, C2, target)
    check_loss_fwd(tag, got, fw)
    check_loss_bwd(tag, got, R.loss_bwd(o["l1"], o["l2"], o["t1"], o["t2"], 0.1, 1.0), o)


@pytest.mark.parametrize("dead", [1, 2])
def test_head_without_valid_rows(ops, dead):
    """One head ignored on every row: loss is NaN like torch's mean reduction, that head's stats are 0 and its dlogits
    exactly 0, the other head's loss sum and dlogits stay within their bounds."""
    o = R.loss_case(R.LOSS_BY_ID["N17-C1500x2-spread3-g1-lw0.1-ign-loss-fwd-17th-row"])
    o["t%d" % dead][:] = R.IGN
    live = 3 - dead
    fw = R.loss_fwd(o["l1"], o["l2"], o["t1"], o["t2"], 0.1)
    bw = R.loss_bwd(o["l1"], o["l2"], o["t1"], o["t2"], 0.1, 0.37)
    assert np.isnan(fw["loss"]) and fw["stats"][3 * live - 2] > 0
    got = run_loss(ops, o, 0.1, 0.37)
    assert np.isnan(got["loss"])
    R.exact("counts", got["stats"][[1, 2, 4, 5]], fw["stats"][[1, 2, 4, 5]])
    assert got["stats"][3 * dead - 3:3 * dead].tolist() == [0.0, 0.0, 0.0]
    R.check("stats[%d] head %d dead" % (3 * live - 3, dead), got["stats"][3 * live - 3], fw["stats"][3 * live - 3],
            fw["b_stats"][3 * live - 3], GPU_FACTOR)
    assert not got["d%d" % dead].any()
    check_loss_bwd("head %d dead" % dead, got, bw, o, heads=(live,))


@pytest.mark.parametrize("head,value", [(1, -5), (1, "C"), (2, -5), (2, "C")])
def test_target_outside_the_classes_gives_a_nan_loss(ops, head, value):
    """include/sbl_hip.h / cls_head.hip: a target outside [0, C) that is not ignore_id is never used as an index, its row's
    loss is NaN.  The call returns; loss and that head's loss sum are NaN; the counts are the reference's (the row is
    valid and never correct); every other row's dlogits stays within its bound."""
    case = R.LOSS_BY_ID["N5-C65x64-spread3-g0.37-lw0.1-gscale-fraction"]
    o = R.loss_case(case)
    C = o["l%d" % head].shape[1]
    o["t%d" % head][2] = C if value == "C" else value
    fw = R.loss_fwd(o["l1"], o["l2"], o["t1"], o["t2"], case["lw"])
    bw = R.loss_bwd(o["l1"], o["l2"], o["t1"], o["t2"], case["lw"], case["gscale"])
    assert bw["rows%d" % head].tolist() == [True, True, False, True, True] and bw["rows%d" % (3 - head)].all()
    got = run_loss(ops, o, case["lw"], case["gscale"])
    assert np.isnan(got["loss"]) and np.isnan(got["stats"][3 * head - 3])
    R.exact("counts", got["stats"][[1, 2, 4, 5]], fw["stats"][[1, 2, 4, 5]])
    other = 3 * (3 - head) - 3
    R.check("stats[%d] target %s" % (other, value), got["stats"][other], fw["stats"][other], fw["b_stats"][other], GPU_FACTOR)
    check_loss_bwd("target %s in head %d" % (value, head), got, bw, o)


# --------------------------------------------------------------------------- repeatability
def test_chunked_paths_are_bitwise_repeatable_in_both_precisions(ops):
    """Two runs of the N = 300 exact case and of the N = 17, C1 = 1500 loss case under "f32" and under "bf16x6": every
    output bitwise equal to the first run's."""
    case = R.HEAD_EXACT[-1]
    assert (case["N"], case["C1"], case["C2"], case["T"]) == (300, 1500, 16, 4)
    real = dict(case, T=3, li=1)
    lcase = R.LOSS_BY_ID["N17-C1500x2-spread3-g0.37-lw1.5-ign-lang-weight-other"]
    oe, orl, ol = R.exact_head_case(case), R.real_head_case(real), R.loss_case(lcase)

    def run():
        outs = []
        for c, o in ((case, oe), (real, orl)):
            g = operands(o)
            fw = run_fwd(ops, g, c)
            buf, _ = run_bwd(ops, g, c, fw["pooled"], R.OUT_BWD, 0, o["preset"])
            outs += [fw[k] for k in R.OUT_FWD] + [buf[k] for k in R.OUT_BWD]
        got = run_loss(ops, ol, lcase["lw"], lcase["gscale"])
        return outs + [torch.from_numpy(np.asarray(got[k])) for k in ("loss", "stats", "d1", "d2")]

    runs = []
    try:
        for prec in ("f32", "f32", "bf16x6", "bf16x6"):
            ops.set_matmul_precision(prec)
            runs.append(run())
    finally:
        ops.set_matmul_precision("f32")
    for other in runs[1:]:
        assert len(other) == len(runs[0])
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


# --------------------------------------------------------------------------- the autograd wrappers
@pytest.mark.parametrize("how", ["gradient=0.37", "2*loss"])
def test_autograd_wrappers_carry_gscale_to_the_kernel(ops, how):
    """ops.ClsHeadFn and ops.ClsLossFn, C1 = 9, C2 = 3, N = 5, T = 3: loss.backward(gradient=0.37) and (2 * loss).backward().
    Stage by stage against the float64 reference under the kernels' own bounds: each stage's reference takes the float32
    tensors the stage was handed (the logits, then their gradients, which autograd keeps with retain_grad())."""
    case = {"id": "autograd", "N": 5, "C1": 9, "C2": 3, "T": 3, "li": 1}
    N, C1, C2, T, li, lw = 5, 9, 3, 3, 1, 1.5
    rng = np.random.default_rng(11)
    o = {"enc": R.f32(rng.standard_normal((N, T, R.D))), "w1": R.f32(rng.standard_normal((C1, R.D)) * 0.05),
         "b1": R.f32(rng.standard_normal(C1) * 0.1), "w2": R.f32(rng.standard_normal((C2, R.D)) * 0.05),
         "b2": R.f32(rng.standard_normal(C2) * 0.1)}
    t1, t2 = rng.integers(0, C1, N).astype(np.int64), rng.integers(0, C2, N).astype(np.int64)
    t1[3] = R.IGN                                    # 4 valid rows of 5 in head 1
    gscale = 0.37 if how == "gradient=0.37" else 2.0
    leaves = {k: dev(v).requires_grad_(True) for k, v in o.items()}
    l1, l2 = ops.ClsHeadFn.apply(leaves["enc"], leaves["w1"], leaves["b1"], leaves["w2"], leaves["b2"], li)
    l1.retain_grad()
    l2.retain_grad()
    loss, stats = ops.ClsLossFn.apply(l1, l2, dev(t1), dev(t2), lw, R.IGN)
    if how == "gradient=0.37":
        loss.backward(gradient=torch.tensor(0.37, device=DEV))
    else:
        (2 * loss).backward()
    torch.cuda.synchronize()
    args = (o["enc"], o["w1"], o["b1"], o["w2"], o["b2"], li)
    fw, fb = R.head_fwd(*args), R.head_fwd_bounds(*args)
    R.check("wrapper logits1 " + how, l1, fw["logits1"], fb["logits1"], GPU_FACTOR)
    R.check("wrapper logits2 " + how, l2, fw["logits2"], fb["logits2"], GPU_FACTOR)
    h1, h2 = host(l1), host(l2)
    ol = {"l1": h1, "l2": h2, "t1": t1, "t2": t2}
    check_loss_fwd("wrapper " + how, {"loss": host(loss), "stats": host(stats)}, R.loss_fwd(h1, h2, t1, t2, lw))
    g1, g2 = host(l1.grad), host(l2.grad)
    check_loss_bwd("wrapper " + how, {"d1": g1, "d2": g2}, R.loss_bwd(h1, h2, t1, t2, lw, gscale), ol)
    # the pooled buffer the wrapper saved is the forward's, which is bitwise repeatable: take it from a direct call
    direct = run_fwd(ops, {k: leaves[k].detach() for k in o}, case)
    assert torch.equal(direct["logits1"], l1.detach()) and torch.equal(direct["logits2"], l2.detach())
    bargs = (o["enc"], host(direct["pooled"]), g1, g2, o["w1"], o["w2"], li)
    ref, bound = R.head_bwd(*bargs), R.head_bwd_bounds(*bargs)
    for k, name in zip(R.OUT_BWD, ("enc", "w1", "b1", "w2", "b2")):
        R.check("wrapper %s %s" % (k, how), leaves[name].grad, ref[k], bound[k], GPU_FACTOR)
