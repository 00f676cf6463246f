"""The last decoder layer on its "ends" rows (Decoder.last_layer_ends_only, transformer/decoder_stages.py): behind the
self-attention core of layer nl-1 only positions 0 and L-1 of every sequence are computed, forward and backward.  The full-row
launch sequence (switch off) is the reference: same tokens, logits, loss and gradients, with dropout off and on (every mask
must be the one the full-row computation draws), for a single-layer decoder too; and the three small movers of the compact
layout against torch indexing on the host.  Bounds: those of test_stage_batched_decoder_backward_equals_per_stage_tape."""
import ctypes
import random

import pytest
import torch

from conftest import maxdiff
from sbl_for_multilingual_lip_reading_amd import detfill
from sbl_for_multilingual_lip_reading_amd.transformer.decoder import ends_rows
from test_hip_parity import DEV, build_model, ops      # noqa: F401  (ops: the fixture that runs a test under f32 and bf16x6)

pytestmark = pytest.mark.gpu

T, HW, NE = 4, 24, 1


def _run_both(ops, B, nd, two, drop_p, coins, seed):
    """One training step with the switch off (full rows) and on (end rows) on the same model -> [(full), (ends)] of
    (pred_l2r, pred_r2l, loss, gradients by name, coins, tokens)."""
    from sbl_for_multilingual_lip_reading_amd import dp
    from sbl_for_multilingual_lip_reading_amd.transformer.loss import cal_performance_device
    x, l2r, r2l = detfill.synthetic_batch(B, T, HW, HW, 71)
    xd, ld, rd = torch.from_numpy(x).to(DEV), torch.from_numpy(l2r).to(DEV), torch.from_numpy(r2l).to(DEV)
    m = build_model(NE, nd).train()
    for mm in m.modules():
        if isinstance(mm, torch.nn.Dropout):
            mm.p = drop_p
    m.decoder.two_streams = two
    m.decoder.coins_host = coins
    flat = dp.FlatModel(m)
    st = ops.dropout_state(torch.device(DEV))
    res = []
    for on in (False, True):
        m.decoder.last_layer_ends_only = on
        flat.zero_grad()
        st._offset = 0                                   # same (seed, offsets) for both runs
        random.seed(seed)
        pl, gl, pr, gr = m(xd, ld, rd)
        loss = 0.5 * (cal_performance_device(pl, gl, 0.1)[0] + cal_performance_device(pr, gr, 0.1)[0])
        loss.backward()
        ops.join_side_streams()
        torch.cuda.synchronize()
        res.append((pl.detach().clone(), pr.detach().clone(), float(loss.item()), {n: p.grad.clone() for n, p in m.named_parameters()},
                    list(m.decoder.last_coins), [t.clone() for t in m.decoder.last_ys]))
    return res


def _check(res):
    full, ends = res
    assert full[4] == ends[4]
    assert all(torch.equal(a, b) for a, b in zip(full[5], ends[5]))
    dl, dr, dloss = maxdiff(ends[0], full[0]), maxdiff(ends[1], full[1]), abs(full[2] - ends[2])
    print("max|dlogit| %.3e %.3e  |dloss| %.3e" % (dl, dr, dloss))
    assert dl < 2e-5 and dr < 2e-5 and dloss < 2e-5
    worst = 0.0
    for n, g in ends[3].items():
        ref = full[3][n]
        if n.startswith("decoder") or n.startswith("encoder"):
            bound = 1e-3 * float(ref.abs().max()) + 2e-6
            d = maxdiff(g, ref)
            worst = max(worst, d / bound)
            assert d < bound, (n, d, bound)
    print("worst gradient difference / bound %.3f" % worst)


@pytest.mark.parametrize("B,two", [(16, True), (16, False), (3, True), (3, False)])
def test_ends_equal_full_rows_without_dropout(ops, B, two):
    """nd = 2: one full-row layer feeding one ends layer; mixed coins.  B = 3: 93 compact rows, the per-weight dW fallback."""
    res = _run_both(ops, B, 2, two, 0.0, None, 17)
    assert 0 < sum(res[0][4]) < 16
    _check(res)


@pytest.mark.parametrize("coins", [[False] * 16, [True, False] * 8], ids=["one-stage", "alternating"])
def test_ends_equal_full_rows_with_dropout(ops, coins):
    """Dropout 0.1 everywhere: the compact kernels must draw, for every element they keep, the decision of the full layout (the
    three sub-layer output dropouts and the cross-attention probability dropout, forward and backward).  One 16-segment stage,
    and many short stages that begin with the L = 1 step alone.  A mask drawn from a compact index is an O(1) error."""
    _check(_run_both(ops, 16, 2, True, 0.1, coins, 17))


def test_ends_equal_full_rows_single_layer_decoder(ops):
    """nd = 1: the last layer is also the first (causal self-attention, x from the embedding)."""
    res = _run_both(ops, 16, 1, True, 0.0, None, 17)
    assert 0 < sum(res[0][4]) < 16
    _check(res)


# --------------------------------------------------------------------------- the movers of the compact layout
def _segs(seg):
    return (ctypes.c_int * len(seg))(*seg), len(seg)


@pytest.mark.parametrize("seg", [tuple(range(1, 17)), (1, 2, 3)], ids=["L1..16", "L1..3"])
def test_ends_gather_scatter_tail_adjoint_match_host_indexing(seg):
    from sbl_for_multilingual_lip_reading_amd import _lib
    _lib.load()
    B, D = 3, 512
    arr, nseg = _segs(seg)
    rows = ends_rows(B, seg)
    R, Rc = B * sum(seg), len(rows)
    idx = torch.tensor(rows, dtype=torch.long)
    g = torch.Generator().manual_seed(3)
    stream = torch.cuda.current_stream().cuda_stream
    # gather: four tensors, then two
    src = [torch.randn(R, D, generator=g) for _ in range(4)]
    srcd = [t.to(DEV) for t in src]
    dst = [torch.full((Rc, D), float("nan"), device=DEV) for _ in range(4)]
    _lib.call("sbl_ends_gather4", *[t.data_ptr() for t in srcd], *[t.data_ptr() for t in dst], B, arr, nseg, D, stream)
    for s, d in zip(src, dst):
        assert torch.equal(d.cpu(), s[idx])
    dst2 = [torch.full((Rc, D), float("nan"), device=DEV) for _ in range(2)]
    _lib.call("sbl_ends_gather4", srcd[2].data_ptr(), srcd[3].data_ptr(), None, None, dst2[0].data_ptr(), dst2[1].data_ptr(), None, None,
              B, arr, nseg, D, stream)
    assert torch.equal(dst2[0].cpu(), src[2][idx]) and torch.equal(dst2[1].cpu(), src[3][idx])
    # scatter: every full row is written - the compact row at the end rows, zero elsewhere
    cs = [torch.randn(Rc, D, generator=g) for _ in range(2)]
    csd = [t.to(DEV) for t in cs]
    full = [torch.full((R, D), float("nan"), device=DEV) for _ in range(2)]
    _lib.call("sbl_ends_scatter2", csd[0].data_ptr(), csd[1].data_ptr(), full[0].data_ptr(), full[1].data_ptr(), B, arr, nseg, D, stream)
    for c, f in zip(cs, full):
        assert torch.equal(f.cpu(), torch.zeros(R, D).index_copy_(0, idx, c))
    one = torch.full((R, D), float("nan"), device=DEV)
    _lib.call("sbl_ends_scatter2", csd[1].data_ptr(), None, one.data_ptr(), None, B, arr, nseg, D, stream)
    assert torch.equal(one.cpu(), torch.zeros(R, D).index_copy_(0, idx, cs[1]))
    # tail adjoint: row (s, b, last) of direction d gets kf_d * dlast_d, row (s, b, first) gets dlast_{1-d}, the L = 1 row both
    dl = [torch.randn(nseg * B, D, generator=g) for _ in range(2)]
    dld = [t.to(DEV) for t in dl]
    sb, first, last = [], [], []
    for s, L in enumerate(seg):
        for b in range(B):
            for k in range(min(2, L)):
                sb.append(s * B + b)
                first.append(k == 0)
                last.append(k == min(2, L) - 1)
    assert seg[0] == 1 and first[0] and last[0]           # the doubly-hit row is among them
    sb = torch.tensor(sb)
    first, last = torch.tensor(first).float()[:, None], torch.tensor(last).float()[:, None]
    for have in ((True, True), (True, False), (False, True)):
        dy = [torch.full((Rc, D), float("nan"), device=DEV) for _ in range(2)]
        _lib.call("sbl_ends_tail_bwd", dld[0].data_ptr() if have[0] else None, dld[1].data_ptr() if have[1] else None,
                  dy[0].data_ptr(), dy[1].data_ptr(), B, arr, nseg, D, stream)
        z = [dl[d][sb] if have[d] else torch.zeros(Rc, D) for d in (0, 1)]
        for d, kf in ((0, 1.0), (1, 2.0)):
            want = last * (kf * z[d]) + first * z[1 - d]
            assert torch.equal(dy[d].cpu(), want), (have, d)
