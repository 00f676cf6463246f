"""tests/decoder_rows_reference.py and tests/ln_reference.py without a GPU: every table and formula the GPU module
tests/test_decoder_rows_gpu.py compares the kernels with is held here to something that does not share its code - a
brute-force triple loop over (segment, b, l), transformer.decoder.ends_rows, torch.flip, F.embedding / F.layer_norm with
float64 autograd, torch.argmax, exact rational arithmetic for the one-rounding fused multiply-add, and the golden entries
fus.a_out / fus.b_out / pe of tests/golden/modules.npz.  The last tests show on the reference side that the GPU module's
comparisons can fail: the four one-line mistakes a kernel could make each change the reference's result on its shapes."""
import fractions

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decoder_rows_reference as R
import ln_reference as LN
from sbl_for_multilingual_lip_reading_amd import detfill
from sbl_for_multilingual_lip_reading_amd.transformer.decoder import ends_rows

SEG_LISTS = [R.EDGE, R.SMALL, R.FULL, R.WIDE]


def u(name, shape):
    return detfill.uniform(name, tuple(shape))


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# --------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("seg_L", SEG_LISTS, ids=["edge", "small", "full", "wide"])
def test_row_tables_against_a_triple_loop(seg_L, B):
    rows, firsts, lasts, flips, ends = [], [], [], {}, []
    r = 0
    for s, L in enumerate(seg_L):
        for b in range(B):
            for l in range(L):
                rows.append((s, b, l))
                flips[r + b * L + l] = r + b * L + (L - 1 - l)
            firsts.append(r + b * L)
            lasts.append(r + b * L + L - 1)
            for k in range(min(2, L)):
                ends.append((s, b, k, r + b * L + k * (L - 1)))
        r += B * L
    seg, b, l, off = R.stage_rows(B, seg_L)
    assert R.n_rows(B, seg_L) == r == len(rows)
    assert list(zip(seg.tolist(), b.tolist(), l.tolist())) == rows
    assert off.tolist() == [B * sum(seg_L[:s]) for s in range(len(seg_L))]
    assert R.flip_rows(B, seg_L).tolist() == [flips[i] for i in range(r)]
    assert R.first_rows(B, seg_L).tolist() == firsts and R.last_rows(B, seg_L).tolist() == lasts
    assert list(zip(*[a.tolist() for a in R.ends_table(B, seg_L)])) == ends
    assert R.ends_full_rows(B, seg_L).tolist() == ends_rows(B, seg_L)
    # the ends rows are exactly the rows the stage tail reads: position 0 and position L-1 of every sequence
    assert sorted(set(R.ends_full_rows(B, seg_L).tolist())) == sorted(set(firsts) | set(lasts))


def test_geometry_of_the_named_shapes():
    """Stage and Wide are the smallest row counts of their kind past one pass of the capped grid."""
    assert R.n_rows(R.STAGE_B, R.FULL) == 4352 and R.ew_passes(4352 * 512) == 2 and R.ew_passes(4352 * 128) == 1
    assert R.n_rows(R.WIDE_B, R.WIDE) == 16512 and R.ew_passes(16512 * 128) == 2 and R.ew_passes(16384 * 128) == 1
    assert len(R.ends_full_rows(R.STAGE_B, R.FULL)) == 992
    assert R.ew_passes(1) == 1 and R.ew_passes(8192 * 256) == 1 and R.ew_passes(8192 * 256 + 1) == 2


# --------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("seg_L", [R.SMALL, R.FULL], ids=["small", "full"])
def test_embedding_against_torch(seg_L):
    B, V = 3, 11
    emb, pe = u("rc.emb", (V, R.D)), u("rc.pe", (20, R.D))
    tok = np.floor((u("rc.tok", (B, 19)).astype(np.float64) + 1) * 0.5 * (V + 8)).astype(np.int64) - 4      # some ids out of range
    assert tok.min() < 0 and tok.max() >= V
    t, pos = R.embed_index(tok, B, seg_L, V)
    E = t64(emb).requires_grad_(True)
    outs, r = [], 0
    for L in seg_L:
        ids = torch.from_numpy(tok[:, :L]).clamp(0, V - 1)
        outs.append((F.embedding(ids, E) + t64(pe)[:L]).reshape(B * L, R.D))
    ref = torch.cat(outs)
    assert np.array_equal(R.embed_pe64(emb, pe, t, pos), ref.detach().numpy())
    assert np.array_equal(R.embed_pe32(emb, pe, t, pos).astype(np.float64), ref.detach().numpy().astype(np.float32))
    dy = u("rc.dy", (ref.shape[0], R.D))
    ref.backward(t64(dy))
    demb, mag, cnt = R.embed_grad64(dy, t, V)
    assert rel(demb, E.grad.numpy()) <= 1e-14
    assert cnt.sum() == ref.shape[0] and np.all(mag >= np.abs(demb) - 1e-12) and np.all((cnt == 0) == (mag.sum(1) == 0))


def test_scaled_embedding_against_torch_and_exact_fma():
    B, L, V, pos0 = 3, 5, 11, 2
    scale = np.float32(np.sqrt(512.0))
    emb, pe = u("rc.emb", (V, R.D)), u("rc.pe", (20, R.D))
    tok = np.floor((u("rc.tok", (B, 19)).astype(np.float64) + 1) * 0.5 * V).astype(np.int64).clip(0, V - 1)
    t, pos = R.embed_index_flat(tok, B, L, V, pos0)
    E = t64(emb).requires_grad_(True)
    ref = (F.embedding(torch.from_numpy(tok[:, pos0:pos0 + L]), E) * float(scale) + t64(pe)[pos0:pos0 + L]).reshape(B * L, R.D)
    assert rel(R.embed_pe64(emb, pe, t, pos, scale), ref.detach().numpy()) <= 1e-15
    dy = u("rc.dy", (B * L, R.D))
    ref.backward(t64(dy))
    assert rel(R.embed_grad64(dy, t, V, scale)[0], E.grad.numpy()) <= 1e-14
    two, one = R.embed_scale_pe32(emb, pe, t, pos, scale)
    r64 = ref.detach().numpy()
    assert np.all(np.abs(two - r64) <= 2 * R.U * (np.abs(r64) + np.abs(np.float64(scale) * emb[t])))
    assert np.all(np.abs(one - r64) <= R.U * np.abs(r64) * (1 + 1e-9))
    assert 0 < np.count_nonzero(two != one) < two.size          # the two forms do differ: the GPU test must accept either


def test_fma32_is_one_rounding():
    """Against exact rationals, on random operands and on constructed midpoints where the double sum alone would round
    the wrong way (a * b + c one quarter-ulp to either side of an fp32 midpoint that the double sum lands on exactly)."""
    a = u("fma.a", (400,)).astype(np.float32)
    b = (u("fma.b", (400,)) * np.float32(23)).astype(np.float32)
    c = u("fma.c", (400,)).astype(np.float32)
    # midpoints: a * b = 1 + 2^-24 (exact: (1 + 2^-12)^2 - 2^-11 is not needed; use a = 1 + 2^-23, b = 1, c = +-2^-60 ... via products)
    a2 = np.array([1 + 2.0 ** -12] * 4, np.float32)
    b2 = np.array([1 + 2.0 ** -12] * 4, np.float32)                      # a * b = 1 + 2^-11 + 2^-24: 2^-24 is half an ulp of 1
    c2 = np.array([2.0 ** -80, -2.0 ** -80, 0.0, 2.0 ** -30], np.float32)
    a, b, c = np.concatenate([a, a2]), np.concatenate([b, b2]), np.concatenate([c, c2])
    got = R.fma32(a, b, c)
    for i in range(a.size):
        exact = fractions.Fraction(float(a[i])) * fractions.Fraction(float(b[i])) + fractions.Fraction(float(c[i]))
        lo = np.float32(float(exact))          # float(Fraction) rounds correctly to double; narrow and look at both neighbours
        cands = sorted({float(np.nextafter(lo, np.float32(-np.inf))), float(lo), float(np.nextafter(lo, np.float32(np.inf)))})
        dist = [abs(fractions.Fraction(x) - exact) for x in cands]
        best = min(dist)
        winners = [x for x, d in zip(cands, dist) if d == best]
        if len(winners) == 2:                  # a true tie: round half to even
            winners = [x for x in winners if (np.float32(x).view(np.uint32) & 1) == 0]
        assert float(got[i]) == winners[0], (i, float(got[i]), winners)
    base = np.float32(1 + 2.0 ** -11)
    assert got[-4] == np.nextafter(base, np.float32(2)) and got[-3] == base and got[-2] == base      # above / below / tie to even


# --------------------------------------------------------------------------- fusion, gather-last
@pytest.mark.parametrize("seg_L", [R.EDGE, R.SMALL, R.FULL], ids=["edge", "small", "full"])
def test_fusion_against_torch_flip_and_autograd(seg_L):
    B = 3
    n = R.n_rows(B, seg_L)
    a, b = u("rc.fa", (n, R.D)), u("rc.fb", (n, R.D))
    flip = R.flip_rows(B, seg_L)
    A, Bt = t64(a).requires_grad_(True), t64(b).requires_grad_(True)
    oa, ob, r = [], [], 0
    for L in seg_L:
        x, y = A[r:r + B * L].view(B, L, R.D), Bt[r:r + B * L].view(B, L, R.D)
        oa.append((x + torch.flip(y, [1])).reshape(B * L, R.D))
        ob.append((2 * y + torch.flip(x, [1])).reshape(B * L, R.D))
        r += B * L
    oa, ob = torch.cat(oa), torch.cat(ob)
    a2, b2 = R.fusion64(a, b, flip)
    assert np.array_equal(a2, oa.detach().numpy()) and np.array_equal(b2, ob.detach().numpy())
    s2, t2 = R.fusion32(a, b, flip)
    assert np.array_equal(s2, a2.astype(np.float32)) and np.array_equal(t2, b2.astype(np.float32))
    wa, wb = u("rc.wa", (n, R.D)), u("rc.wb", (n, R.D))
    (oa * t64(wa)).sum().add((ob * t64(wb)).sum()).backward()
    da, db = R.fusion_bwd64(wa, wb, flip)
    assert rel(da, A.grad.numpy()) <= 1e-15 and rel(db, Bt.grad.numpy()) <= 1e-15
    d32 = R.fusion_bwd32(wa, wb, flip)
    assert np.array_equal(d32[0], da.astype(np.float32)) and np.array_equal(d32[1], db.astype(np.float32))
    # adjoint identity in float64
    lhs = (a2 * wa).sum() + (b2 * wb).sum()
    rhs = (da * a).sum() + (db * b).sum()
    assert abs(lhs - rhs) <= 1e-12 * (np.abs(a2 * wa).sum() + np.abs(b2 * wb).sum())


def test_fusion_against_the_golden_fixture(golden_modules):
    """fus.a_out / fus.b_out were written by the reference model's own fusion of detfill 'fus.a' / 'fus.b' (2, 6, 512)."""
    a, b = u("fus.a", (2, 6, 512)).reshape(12, 512), u("fus.b", (2, 6, 512)).reshape(12, 512)
    a2, b2 = R.fusion32(a, b, R.flip_rows(2, (6,)))
    assert np.array_equal(a2.reshape(2, 6, 512), golden_modules["fus.a_out"])
    assert np.array_equal(b2.reshape(2, 6, 512), golden_modules["fus.b_out"])


def test_embedding_against_the_golden_positional_encoding(golden_modules):
    """With the golden sinusoid table as pe and a one-hot-free identity embedding of zeros, the rows are pe[l] itself."""
    pe = golden_modules["pe"]
    B, seg_L, V = 2, (1, 4, 16), 5
    tok = np.zeros((B, 16), np.int64)
    t, pos = R.embed_index(tok, B, seg_L, V)
    out = R.embed_pe32(np.zeros((V, 512), np.float32), pe, t, pos)
    r = 0
    for L in seg_L:
        assert np.array_equal(out[r:r + B * L].reshape(B, L, 512), np.broadcast_to(pe[:L], (B, L, 512)))
        r += B * L
    assert pe[0, 0] == 0 and pe[0, 1] == 1 and abs(pe[1, 0] - np.sin(1.0)) < 1e-6


@pytest.mark.parametrize("seg_L", [R.EDGE, R.SMALL, R.FULL], ids=["edge", "small", "full"])
def test_gather_last_and_ends_adjoints(seg_L):
    B = 3
    n = R.n_rows(B, seg_L)
    x = u("rc.gx", (n, R.D))
    last, first = R.last_rows(B, seg_L), R.first_rows(B, seg_L)
    X = t64(x).requires_grad_(True)
    outs, r = [], 0
    for L in seg_L:
        outs.append(X[r:r + B * L].view(B, L, R.D)[:, -1])
        r += B * L
    out = torch.cat(outs)
    assert np.array_equal(R.gather_last(x, last).astype(np.float64), out.detach().numpy())
    w = u("rc.gw", (len(last), R.D))
    (out * t64(w)).sum().backward()
    dx = R.gather_last_bwd(w, last, n)
    assert np.array_equal(dx.astype(np.float64), X.grad.numpy())
    assert abs((R.gather_last(x, last).astype(np.float64) * w).sum() - (dx.astype(np.float64) * x).sum()) <= 1e-12 * np.abs(w).sum()
    # the ends layout: gather by the table, scatter-add back; <G x, w> == <x, G^T w> in float64
    er = R.ends_full_rows(B, seg_L)
    wc = u("rc.ew", (len(er), R.D)).astype(np.float64)
    back = np.zeros((n, R.D))
    np.add.at(back, er, wc)
    assert abs((x[er].astype(np.float64) * wc).sum() - (back * x).sum()) <= 1e-12 * np.abs(wc).sum()
    # the tail's `last` is the fusion at the last position
    a, b = u("rc.fa", (n, R.D)), u("rc.fb", (n, R.D))
    a2, b2 = R.fusion32(a, b, R.flip_rows(B, seg_L))
    l0, l1 = R.tail_last32(a, b, first, last)
    assert np.array_equal(l0, a2[last]) and np.array_equal(l1, b2[last])
    m0, m1 = R.tail_last64(a, b, first, last)
    f0, f1 = R.fusion64(a, b, R.flip_rows(B, seg_L))
    assert np.array_equal(m0, f0[last]) and np.array_equal(m1, f1[last])


# --------------------------------------------------------------------------- arg-max
def test_first_argmax_is_torch_argmax():
    x = np.rint(u("rc.am", (64, 200)) * np.float32(3)).astype(np.float32)          # values in -3..3: every row is full of ties
    assert np.array_equal(R.first_argmax(x), torch.argmax(torch.from_numpy(x), dim=1).numpy())
    assert (np.sort(x, 1)[:, -1] == np.sort(x, 1)[:, -2]).all()
    assert R.first_argmax(np.full((3, 7), -np.inf, np.float32)).tolist() == [0, 0, 0]
    pred = u("rc.am2", (5, 58))
    gold = np.arange(5 * 9).reshape(5, 9)
    ys = np.full((5, 9), -7)
    own = R.argmax_select(pred, gold, ys, 3, 1)
    assert np.array_equal(own[:, 4], torch.argmax(torch.from_numpy(pred), 1).numpy()) and (np.delete(own, 4, 1) == -7).all()
    tf = R.argmax_select(pred, gold, ys, 3, 0)
    assert np.array_equal(tf[:, 4], gold[:, 3]) and (np.delete(tf, 4, 1) == -7).all()
    logits = u("rc.am3", (4 * 5, 58))
    tk = R.tail_tokens(ys, logits, 5, 4, 7)
    assert np.array_equal(tk[:, 8], torch.argmax(torch.from_numpy(logits[15:]), 1).numpy()) and (np.delete(tk, 8, 1) == -7).all()


def test_tail_logits_against_torch():
    last, w = u("rc.tl", (9, R.D)), u("rc.tw", (17, R.D))
    lg, mag = R.tail_logits64(last, w)
    assert rel(lg, F.linear(t64(last), t64(w)).numpy()) <= 1e-14 and np.all(mag >= np.abs(lg))


# --------------------------------------------------------------------------- LayerNorm model
@pytest.mark.parametrize("with_res,p", [(1, 0.0), (0, 0.0), (1, 0.1)])
def test_layernorm_reference_against_torch_autograd(with_res, p):
    M = 7
    x, res = u("rc.lx", (M, R.D)) * np.float32(2), (u("rc.lr", (M, R.D)) if with_res else None)
    gamma, beta = np.float32(1) + np.float32(0.2) * u("rc.lg", (R.D,)), np.float32(0.1) * u("rc.lb", (R.D,))
    dy = u("rc.ldy", (M, R.D))
    mask = (u("rc.lm", (M, R.D)) > -0.8) if p else None
    f = LN.ln_fwd_ref(x, res, gamma, beta, mask, p)
    X = t64(x).requires_grad_(True)
    v = X * t64(mask * float(LN.keep_scale(p))) if p else X
    v = v + t64(res) if with_res else v
    v.retain_grad()
    G = t64(gamma).requires_grad_(True)
    y = F.layer_norm(v, (R.D,), G, t64(beta), float(np.float32(LN.LN_EPS)))
    assert rel(f["y"], y.detach().numpy()) <= 1e-13
    y.backward(t64(dy))
    dz, e_dz, t, e_t = LN.ln_bwd_ref(dy, f["v"], f["e_v"], gamma, f["mean"], f["rstd"])
    assert rel(dz, v.grad.numpy()) <= 1e-12 and rel(t.sum(0), G.grad.numpy()) <= 1e-12
    if p:
        assert rel(dz * mask * float(LN.keep_scale(p)), X.grad.numpy()) <= 1e-12
    assert np.all(f["e_y"] > 0) and np.all(e_dz > 0) and np.all(f["e_y"] < 1e-4) and np.all(e_dz < 1e-4)
    assert LN.ln_geometry(992) == (32, 31) and LN.ln_geometry(4352) == (32, 136) and LN.ln_geometry(3) == (16, 1)


# --------------------------------------------------------------------------- the comparisons can fail
def test_the_four_one_line_mistakes_change_the_reference():
    """(i) the compact-index mask differs from the full-layout mask wherever the ends rows are not 0..M-1; (ii) swapping the
    tail's factors changes `last`; (iii) the last-index tie rule differs on a planted tie; (iv) the factor 2 on the flipped
    term changes the fusion's adjoint."""
    B = 3
    for seg_L, same in ((R.EDGE, True), (R.SMALL, False), (R.FULL, False)):
        er = R.ends_full_rows(B, seg_L)
        assert np.array_equal(er, np.arange(len(er))) == same
    n = R.n_rows(B, R.SMALL)
    a, b = u("rc.fa", (n, R.D)), u("rc.fb", (n, R.D))
    first, last = R.first_rows(B, R.SMALL), R.last_rows(B, R.SMALL)
    l0, l1 = R.tail_last32(a, b, first, last)
    assert not np.array_equal(l0, np.float32(2) * a[last] + b[first]) and not np.array_equal(l1, b[last] + a[first])
    x = np.zeros((1, 65), np.float32)
    x[0, 1] = x[0, 64] = 1
    assert R.first_argmax(x)[0] == 1
    flip = R.flip_rows(B, R.SMALL)
    da, db = R.fusion_bwd32(a, b, flip)
    assert not np.array_equal(db, np.float32(2) * a[flip] + b)
