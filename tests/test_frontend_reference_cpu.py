"""tests/frontend_reference.py against the oracle and the reference's fixture, the measurement that motivates it, and proof
that the bound it allows the GPU tests is sharp enough to see the faults a backward rewrite would make.  No GPU.

Inputs: weights are the deterministic fill (oracle.make_state_dict); clips and dy are detfill.normal streams selected by
frontend_reference.CASES' salt, except that the 12-image case uses the inputs of tests/golden/modules.npz ("fe.x", "fe.dy"), which the
fixture check needs anyway.  The two `flip` cases were chosen as the first salt at which this torch build's fp32 CPU
evaluation takes one ReLU decision differently from float64 ((8,8,32,32): salt 0 has none, salt 1 has one; the result is the same with 1 to 16 threads).  fp32 CPU
arithmetic differs between torch builds; if a build stops showing a flip at these salts, search for the next salt that
does (the smallest |z| / max|z| is 1e-9 to 1e-6 in every case, so one is always near) and update CASES - the claim under
test is "a single decision costs 1e-3 to 1e-1", not the particular element.
With 12 images and a final 1x1 map the shared-mask fp32 error is 0.7e-5 to 1.3e-5 over inputs; the fixture's gives 6.8e-6."""
import functools

import numpy as np
import pytest
import torch

import frontend_reference as R
from conftest import maxdiff
from oracle import sbl_oracle as O

CASES, inputs = R.CASES, R.inputs
ODD = CASES[1]


@functools.lru_cache(None)
def base_sd():
    return {k: v for k, v in O.make_state_dict(0, 0).items() if k.startswith(R.PREFIX)}


@functools.lru_cache(None)
def evals(case):
    """(float64 own masks, fp32 own masks, float64 under fp32's masks) of a case; shared, never modified."""
    shape, salt, _ = case
    x, dy = inputs(shape, salt)
    e64 = R.evaluate(base_sd(), x, dy)
    e32 = R.evaluate(base_sd(), x, dy, dtype=torch.float32)
    return e64, e32, R.evaluate(base_sd(), x, dy, masks=e32.masks)


def gpu_bounds(case):
    """(tol_fwd, tol_grad) as tests/test_frontend_grads_gpu.py derives them: 8x the fp32 CPU evaluation's error against
    float64 under the same masks."""
    _, e32, s64 = evals(case)
    e_fwd = max(R.rel(a, b) for a, b in zip(e32.blocks + [e32.out], s64.blocks + [s64.out]))
    return 8 * e_fwd, 8 * R.worst(e32.grads, s64.grads)[0]


def test_sixty_parameters_seventeen_relus():
    e64 = evals(CASES[1])[0]
    assert len(e64.grads) == 60 and len(e64.masks["relu"]) == R.N_RELU == 17
    assert e64.masks["pool"].shape == (6, 64, 6, 10) and int(e64.masks["pool"].max()) <= 8


def test_own_masks_float64_equals_the_oracle():
    """z * mask and the gather are the oracle's relu and max_pool3d.  Not bit-identical: a stem pixel that is the arg-max of
    several overlapping pool windows has their gradients summed in another order, so 1e-12 instead of 0."""
    shape, salt, _ = CASES[0]
    x, dy = inputs(shape, salt)
    sd = R.leaves({k: (v.double() if v.is_floating_point() else v) for k, v in base_sd().items()})
    ref = O.frontend(sd, x.double().unsqueeze(1), training=True)
    ref.backward(dy.double().view(ref.shape))
    e64 = evals(CASES[0])[0]
    assert R.rel(e64.out, ref.reshape(-1, 512)) < 1e-12
    for k, g in e64.grads.items():
        assert R.rel(g, sd[k].grad) < 1e-12, k
    for k, v in e64.sd.items():
        if "running_" in k or "num_batches" in k:
            assert maxdiff(v, sd[k]) == 0, k
    assert int(e64.sd[R.PREFIX + "resnet18.layer1.0.bn1.num_batches_tracked"]) == 1


def test_own_masks_match_the_reference_fixture(golden_modules):
    """tests/golden/modules.npz was written by the reference itself in fp32.  The fp32 evaluation meets
    test_oracle_golden.py's tolerances (2e-5 on the output, 1e-4 * max(1, max|ref|) on the eight stored gradients, 1e-6 on
    the running statistics); the float64 one meets them too except on the output, where the fixture's own fp32 rounding
    (values up to 5) is 3e-5 and the bound is test_frontend_small_golden's 1e-4."""
    g = golden_modules
    keys = [k for k in g.files if k.startswith("fe.grad:")]
    assert len(keys) == 8
    for e, tol_out in ((evals(CASES[0])[1], 2e-5), (evals(CASES[0])[0], 1e-4)):
        assert maxdiff(e.out.view(2, 6, 512), g["fe.out"]) < tol_out
        for k in keys:
            ref = g[k]
            assert maxdiff(e.grads[R.PREFIX + k[len("fe.grad:"):]], ref) < 1e-4 * max(1.0, float(np.abs(ref).max())), k
        for s in ("running_mean", "running_var"):
            assert maxdiff(e.sd[R.PREFIX + "frontend3D.1." + s], g["fe.after:frontend3D.1." + s]) < 1e-6


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_one_decision_is_the_whole_fp32_error(case):
    """The frontend chain is conditioned near 6e-6; the 1e-2 that the end-to-end tests allow is one ReLU / pool decision."""
    e64, e32, s64 = evals(case)
    n = R.n_differing(e32.masks, e64)
    own, shared = R.worst(e32.grads, e64.grads), R.worst(e32.grads, s64.grads)
    minz = min(float(z.abs().min() / z.abs().max()) for z in e64.z)
    print("%s: %d decisions differ; fp32 vs f64: own masks %.1e (%s), f64 under fp32's masks %.1e (%s); min|z|/max|z| %.0e"
          % (case[0], n, own[0], own[1], shared[0], shared[1], minz))
    assert shared[0] <= 1e-5
    assert n <= 1 and (n == 1) == case[2]
    if case[2]:
        assert own[0] >= 1e-3
    else:
        assert abs(own[0] - shared[0]) < 1e-9
    tol_fwd, _ = gpu_bounds(case)
    assert tol_fwd <= 8 * 8e-6 and R.invalid_flips(e32.masks, e64, tol_fwd) == []


def _flipped(masks, i, j):
    relu = [m.clone() for m in masks["relu"]]
    relu[i].view(-1)[j] ^= True
    return {"relu": relu, "pool": masks["pool"].clone()}


def test_planted_faults_exceed_ten_times_the_gpu_bound():
    """What a wrong backward would do, planted in the reference, against 10x the bound the GPU tests hold: one flipped mask
    bit in layer 4, one dgamma off by 1e-3, the shortcut's input gradient of a stride-2 block missing on the last row of an
    odd map (the (H+1)//2 edge of the compact form)."""
    shape, salt, _ = ODD
    x, dy = inputs(shape, salt)
    e64 = evals(ODD)[0]
    bound = gpu_bounds(ODD)[1]
    assert bound <= 2e-4
    print("GPU gradient bound of %s: %.2e" % (shape, bound))
    # a layer-4 ReLU bit (bn1 of layer4.0: ReLU 13), at the element of smallest |z|
    i = 13
    assert e64.z[i].shape[1] == 512
    j = int(e64.z[i].abs().argmin())
    f = R.evaluate(base_sd(), x, dy, masks=_flipped(e64.masks, i, j))
    moved = R.worst(f.grads, e64.grads)
    print("flipped bit: %.2e (%s)" % moved)
    assert moved[0] >= 10 * bound
    # dgamma * (1 + 1e-3)
    k = R.PREFIX + "resnet18.layer2.0.bn2.weight"
    assert R.rel(e64.grads[k] * (1 + 1e-3), e64.grads[k]) >= 10 * bound
    # the shortcut addend of layer3.0 (input map 3 x 5) dropped on row 2 = compact row (3 + 1) // 2 - 1
    assert e64.blocks[2].shape[2:] == (3, 5)

    def tap(name, t):
        if name != "resnet18.layer3.0.shortcut_in":
            return t
        t = t * 1
        t.register_hook(lambda g: torch.cat([g[:, :, :2], torch.zeros_like(g[:, :, 2:])], 2))
        return t
    f = R.evaluate(base_sd(), x, dy, masks=e64.masks, tap=tap)
    assert R.rel(f.out, e64.out) == 0
    moved = R.worst(f.grads, e64.grads)
    print("dropped shortcut row: %.2e (%s)" % moved)
    assert moved[0] >= 10 * bound
    unmoved = [k for k in f.grads if "layer3" in k or "layer4" in k]
    assert all(R.rel(f.grads[k], e64.grads[k]) == 0 for k in unmoved)


def test_invalid_flips_accepts_rounding_and_rejects_errors():
    e64 = evals(ODD)[0]
    tol_fwd = gpu_bounds(ODD)[0]
    assert R.invalid_flips(e64.masks, e64, tol_fwd) == []
    near = [i for i, z in enumerate(e64.z) if float(z.abs().min()) <= tol_fwd * float(z.abs().max())]
    assert 0 in near and len(near) >= 4, near                  # the stem and some trunk layers have an element that close to 0
    for i in near:
        z = e64.z[i].flatten()
        j = int(z.abs().argmin())
        assert R.invalid_flips(_flipped(e64.masks, i, j), e64, tol_fwd) == []                  # within rounding of 0
        j = int(z.abs().argsort()[z.numel() // 2])
        bad = R.invalid_flips(_flipped(e64.masks, i, j), e64, tol_fwd)
        assert [(b[0], b[1]) for b in bad] == [("relu%d" % i, j)]                              # a median element
    # a pool code naming a tap below the window maximum, one naming the padding, one out of range
    taps, code = e64.taps, e64.masks["pool"]
    gap = taps.max(0).values - taps.min(0).values
    j = int(gap.flatten().argmax())
    assert torch.isinf(gap.flatten()[j])                                                        # a border window
    interior = torch.where(torch.isinf(gap), torch.zeros_like(gap), gap).flatten()
    j2 = int(interior.argmax())
    for jj, wrong in ((j, int(taps.flatten(1)[:, j].argmin())), (j2, int(taps.flatten(1)[:, j2].argmin())), (j2, 9)):
        c = code.clone()
        c.view(-1)[jj] = wrong
        bad = R.invalid_flips({"relu": e64.masks["relu"], "pool": c}, e64, tol_fwd)
        assert [(b[0], b[1]) for b in bad] == [("pool", jj)]
    # two exactly tied taps (both clamped to 0 by the ReLU): either code is as good
    tied = ((taps == taps.max(0).values).sum(0) > 1).flatten().nonzero().flatten()
    assert tied.numel() > 0
    jj = int(tied[0])
    c = code.clone()
    c.view(-1)[jj] = int((taps.flatten(1)[:, jj] == taps.flatten(1)[:, jj].max()).nonzero().flatten()[-1])
    assert int(c.view(-1)[jj]) != int(code.view(-1)[jj])
    assert R.invalid_flips({"relu": e64.masks["relu"], "pool": c}, e64, tol_fwd) == []
