"""Route-aware float64 tests of csrc/attention.hip on the GPU: every case of tests/attention_routes.py, on the leaf written
next to it, in a contiguous and in the production-packed layout, with flat, peaked and planted inputs, without and with
dropout - the dropout path as a direct comparison with the float64 reference under the numpy restatement of the mask.  Bounds,
reference and case table: tests/attention_routes.py (checked on the CPU by tests/test_attention_routes_cpu.py).

Every output buffer is pre-filled with a sentinel, every input buffer's padding with NaN: gap columns, rows past the end and
the tail of the probability buffer must keep the sentinel bit for bit, and a read outside an operand poisons the result."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import attention_routes as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 777.25
SEED = 1234567
OFFSETS = (7, 12)                   # offset0 != offset1 of the dual launches
SEEDS = {}


@pytest.fixture(scope="module", params=["f32", "bf16x6"])
def ops(request):
    """Both fp32-grade arithmetics of the tile engine, as in tests/test_hip_parity.py: the attention kernels use fp32 MFMA
    either way, and the parametrisation pins that they do not depend on the mode."""
    from sbl_for_multilingual_lip_reading_amd import _lib, ops as _ops
    _lib.load()
    assert torch.cuda.is_available()
    _ops.set_matmul_precision(request.param)
    yield _ops
    _ops.set_matmul_precision("f32")


def _seed(value=SEED):
    if value not in SEEDS:
        SEEDS[value] = torch.tensor([value], dtype=torch.int64, device=DEV)
    return SEEDS[value]


class Buf:
    """(rows + 2, nslots * HD + pad) floats filled with `fill`, `lead` floats in front; slot i is the column block
    [i * HD, (i + 1) * HD) of the first `rows` rows."""

    def __init__(self, rows, nslots, HD, fill, lead=0, pad=0):
        self.rows, self.HD, self.ld, self.lead, self.fill = rows, HD, nslots * HD + pad, lead, fill
        self.flat = torch.full((lead + (rows + 2) * self.ld,), fill, dtype=torch.float32, device=DEV)
        self.mat = self.flat[lead:].view(rows + 2, self.ld)

    def slot(self, i):
        return self.mat[:self.rows, i * self.HD:(i + 1) * self.HD]

    def ptr(self, i):
        return self.slot(i).data_ptr()

    def put(self, i, arr):
        self.slot(i).copy_(torch.from_numpy(np.ascontiguousarray(arr)))
        return self

    def get(self, i):
        return self.slot(i).cpu().numpy()

    def assert_rest_untouched(self, written):
        """everything outside the written slots still holds the fill value bit for bit: gap columns, the rows past the end,
        the floats in front"""
        m = self.flat.clone()
        for i in written:
            m[self.lead:].view(self.rows + 2, self.ld)[:self.rows, i * self.HD:(i + 1) * self.HD] = self.fill
        assert bool((m == self.fill).all()), "a store outside the output rows / columns"


def _arr(segL):
    return (ctypes.c_int * len(segL))(*segL)


@functools.lru_cache(maxsize=None)
def _inputs(name, family, direction=0, full_row=False):
    return A.make_inputs(A.CASE[name], family, direction, full_row)


@functools.lru_cache(maxsize=None)
def _reference(name, family, drop_p, direction=0, full_row=False):
    return A.reference(A.CASE[name], _inputs(name, family, direction, full_row), drop_p, SEED, OFFSETS[direction])


class Operands:
    """The device buffers of one direction of a case in one layout family.
    contig: every tensor its own (rows, H*64) buffer.  packed: q, k, v (self-attention) column slices of one (rows, 3*H*64)
    buffer, or q a slice of such a buffer and K / V slices of a (B*Lk, 2*H*64) buffer (cross-attention); o, dout and the
    gradients slices of equally packed buffers.  Flags of the case: o / the gradients offset by one float, gradient stride + 2."""

    def __init__(self, c, inp, layout):
        HD, Rq, Rk = c.H * 64, A.rows_q(c), A.rows_k(c)
        nan = float("nan")
        o_lead = 1 if "o_off1" in c.flags else 0
        g_lead = 1 if "dq_off1" in c.flags else 0
        g_pad = 2 if "gstride2" in c.flags else 0
        if layout == "contig":
            self.q, self.k, self.v, self.do = ((Buf(r, 1, HD, nan).put(0, inp[n]), 0) for n, r in (("q", Rq), ("k", Rk), ("v", Rk), ("do", Rq)))
            self.o = (Buf(Rq, 1, HD, SENT, o_lead), 0)
            self.dq, self.dk, self.dv = ((Buf(r, 1, HD, SENT, g_lead, g_pad), 0) for r in (Rq, Rk, Rk))
        else:
            qb = Buf(Rq, 3, HD, nan).put(0, inp["q"])
            gq = Buf(Rq, 3, HD, SENT, g_lead, g_pad)
            if c.Lk:
                kvb = Buf(Rk, 2, HD, nan).put(0, inp["k"]).put(1, inp["v"])
                gkv = Buf(Rk, 2, HD, SENT, g_lead, g_pad)
                self.k, self.v, self.dk, self.dv = (kvb, 0), (kvb, 1), (gkv, 0), (gkv, 1)
            else:
                qb.put(1, inp["k"]).put(2, inp["v"])
                self.k, self.v, self.dk, self.dv = (qb, 1), (qb, 2), (gq, 1), (gq, 2)
            self.q, self.dq = (qb, 0), (gq, 0)
            self.o = (Buf(Rq, 3, HD, SENT, o_lead), 1)
            self.do = (Buf(Rq, 3, HD, nan).put(2, inp["do"]), 2)
        self.ptot = A.p_offsets(A.q_lengths(c), c.B, c.H, c.Lk)[1]
        self.p = torch.full((self.ptot + 8,), SENT, dtype=torch.float32, device=DEV)
        self.mask = None if inp["mask"] is None else torch.from_numpy(inp["mask"]).to(DEV)

    @staticmethod
    def pl(t):
        return t[0].ptr(t[1]), t[0].ld

    def forward_out(self, c):
        self.o[0].assert_rest_untouched([self.o[1]])
        out = dict(o=self.o[0].get(self.o[1]), p=None)
        if c.entry != "grouped":
            assert bool((self.p[self.ptot:] == SENT).all()), "a store past the probability buffer"
            out["p"] = self.p[:self.ptot].cpu().numpy()
        else:
            assert bool((self.p == SENT).all())
        return out

    def backward_out(self, out):
        bufs = {}
        for n in ("dq", "dk", "dv"):
            b, i = getattr(self, n)
            bufs.setdefault(id(b), (b, []))[1].append(i)
            out[n] = b.get(i)
        for b, written in bufs.values():
            b.assert_rest_untouched(written)
        return out


def run_forward(ops, c, sets, drop_p):
    """one forward call of the case's entry point on the operand sets of its directions (two for the dual / ends launches)"""
    mk = {None: 0, "causal": 1, "tensor": 2}[c.mask]
    seed = _seed().data_ptr() if drop_p else None
    a = sets[0]
    (q, ldq), (k, ldk), (v, ldv), (o, ldo) = (Operands.pl(t) for t in (a.q, a.k, a.v, a.o))
    if c.entry == "seg" and mk == 2:
        ops.call("sbl_attention_fwd", q, ldq, k, ldk, v, ldv, o, ldo, a.p.data_ptr(), 2, a.mask.data_ptr(), c.B, c.H, c.segL[0], c.Lk,
                 A.SCALE, drop_p, seed, OFFSETS[0], ops._s())
    elif c.entry == "seg":
        ops.call("sbl_attention_seg_fwd", q, ldq, k, ldk, v, ldv, o, ldo, a.p.data_ptr(), mk, None, c.B, c.H, _arr(c.segL), len(c.segL),
                 c.Lk, A.SCALE, drop_p, seed, OFFSETS[0], ops._s())
    elif c.entry == "grouped":
        ops.call("sbl_attention_seg_grouped_fwd", q, ldq, k, ldk, v, ldv, o, ldo, c.B, c.H, _arr(c.segL), len(c.segL), c.Lk, c.kvg,
                 A.SCALE, drop_p, seed, OFFSETS[0], ops._s())
    else:
        b = sets[1]
        args = [q, b.q[0].ptr(b.q[1]), ldq, k, b.k[0].ptr(b.k[1]), ldk, v, b.v[0].ptr(b.v[1]), ldv, o, b.o[0].ptr(b.o[1]), ldo,
                a.p.data_ptr(), b.p.data_ptr()]
        if c.entry == "seg2":
            ops.call("sbl_attention_seg2_fwd", *args, mk, c.B, c.H, _arr(c.segL), len(c.segL), c.Lk, A.SCALE, drop_p, seed, OFFSETS[0],
                     OFFSETS[1], ops._s())
        else:
            ops.call("sbl_attention_ends2_fwd", *args, c.B, c.H, _arr(c.segL), len(c.segL), c.Lk, A.SCALE, drop_p, seed, OFFSETS[0],
                     OFFSETS[1], ops._s())
    torch.cuda.synchronize()
    return [s.forward_out(c) for s in sets]


def run_backward(ops, c, a, drop_p, offset, times=1):
    """sbl_attention_seg_bwd / sbl_attention_ends_bwd from the kernel's own p, into sentinel-filled gradient buffers"""
    seed = _seed().data_ptr() if drop_p else None
    args = []
    for t in (a.do, a.q, a.k, a.v):
        args += list(Operands.pl(t))
    args.append(a.p.data_ptr())
    for t in (a.dq, a.dk, a.dv):
        args += list(Operands.pl(t))
    name = "sbl_attention_ends_bwd" if c.entry == "ends" else "sbl_attention_seg_bwd"
    for _ in range(times):
        ops.call(name, *args, c.B, c.H, _arr(c.segL), len(c.segL), c.Lk, A.SCALE, drop_p, seed, offset, ops._s())
    torch.cuda.synchronize()


def _directions(c):
    return (0, 1) if c.entry in ("seg2", "ends") else (0,)


def check(c, family, drop_p, direction, out, names, full_row=False):
    ref = _reference(c.name, family, drop_p, direction, full_row)
    ratios = A.compare(ref, out, names)
    bad = A.exact_failures(c, _inputs(c.name, family, direction, full_row), ref, out, family)
    print("%s %s p=%.1f dir=%d: %s" % (c.name, family, drop_p, direction, " ".join("%s %.3g" % kv for kv in ratios.items())))
    assert not bad, bad
    assert all(r <= 1.0 for r in ratios.values()), (c.name, family, drop_p, direction, ratios)


def run_case(ops, c, layout, family, drop_p, full_row=False):
    sets = [Operands(c, _inputs(c.name, family, d, full_row), layout) for d in _directions(c)]
    outs = run_forward(ops, c, sets, drop_p)
    for d, out in zip(_directions(c), outs):
        check(c, family, drop_p, d, out, ("p", "o"), full_row)
    if c.bwd is not None:
        for d, (a, out) in enumerate(zip(sets, outs)):
            # the atomics leaf zero-fills inside the call: twice into the same buffers must give the value once, not twice
            run_backward(ops, c, a, drop_p, OFFSETS[d], times=2 if c.bwd.red == "atomics" else 1)
            check(c, family, drop_p, d, a.backward_out(out), ("dq", "dk", "dv"), full_row)
    return sets, outs


@pytest.mark.parametrize("layout", ["contig", "packed"])
@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_forward_backward_without_dropout(ops, case, layout):
    """p, o against float64; dq, dk, dv from the kernel's own p against the float64 backward; the sentinels hold; a row with
    one visible key (row 0 under the causal mask) has p exactly 1; masked positions are exactly 0 (their bound is 0);
    planted: duplicate keys get bit-identical probabilities."""
    for family in A.FAMILIES + (("planted",) if case.name in A.PLANTED else ()):
        run_case(ops, case, layout, family, 0.0)


@pytest.mark.parametrize("layout", ["contig", "packed"])
@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_forward_backward_with_dropout(ops, case, layout):
    """The same comparisons with the float64 reference given the numpy keep mask at the documented indices: full layout, query
    tiles, the dual launch (offset0 != offset1), grouped and ends."""
    for family in A.FAMILIES:
        for drop_p in (0.3, 0.1):
            run_case(ops, case, layout, family, drop_p)


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_dropout_mask_read_back_through_identity_values(ops, case):
    """V = the first Lk rows of the 64 x 64 identity: o[:, :Lk] is the dropped p itself.  Every element is 0 or p * keep_scale,
    at exactly the positions the numpy mask gives."""
    c, drop_p = case, 0.3
    HD = c.H * 64
    v = np.zeros((A.rows_k(c), HD), dtype=np.float32)
    for pr in A.problems(c):
        v[pr["krows"], pr["h"] * 64 + np.arange(pr["Lk"])] = 1.0
    sets = [Operands(c, dict(_inputs(c.name, "flat", d), v=v), "contig") for d in _directions(c)]
    outs = run_forward(ops, c, sets, drop_p)
    ks = A.keep_scale(drop_p)
    for d, out in zip(_directions(c), outs):
        ref_p = _reference(c.name, "flat", 0.0, d)["p"][0]
        for pr in A.problems(c):
            keep = A.keep_mask(SEED, OFFSETS[d], A.documented_mask_index(c, pr), drop_p)
            got = out["o"][pr["qrows"]][:, pr["h"] * 64:pr["h"] * 64 + pr["Lk"]]
            vis = ref_p[pr["pidx"]] > 0
            assert np.array_equal(got != 0, keep & vis), (c.name, d, pr["s"], pr["h"], pr["b"])
            if out["p"] is not None:
                want = np.where(keep, out["p"][pr["pidx"]] * ks, np.float32(0.0)).astype(np.float32)
                assert np.array_equal(got, want), (c.name, d, pr["s"], pr["h"], pr["b"])


def test_hash_pinned_to_the_library(ops):
    """numpy rand_u32 against sbl_dropout over ones: the keep masks match bit for bit (a length that is no multiple of the
    256-thread block, three (seed, offset) pairs, one seed with the top bit set)."""
    n = 70001
    x = torch.ones(n, device=DEV)
    for seed, offset, p in ((SEED, 7, 0.3), (-5, 0, 0.1), (0x0123456789ABCDEF, (1 << 40) + 3, 0.5)):
        y = torch.full((n + 3,), SENT, device=DEV)
        ops.call("sbl_dropout", x.data_ptr(), y.data_ptr(), n, p, _seed(seed).data_ptr(), offset, ops._s())
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        keep = A.keep_mask(seed & A.M64, offset, np.arange(n), p)
        assert np.array_equal(got[:n] != 0, keep) and np.all(got[n:] == SENT)
        assert np.array_equal(got[:n], np.where(keep, A.keep_scale(p), np.float32(0.0)))


ENDS_SMALL = [c for c in A.CASES if c.entry == "ends" and max(c.segL) <= 16]


@pytest.mark.parametrize("case", ENDS_SMALL, ids=lambda c: c.name)
def test_ends_equal_the_full_batch_on_the_kept_rows(ops, case):
    """sbl_attention_ends2_fwd / sbl_attention_ends_bwd against sbl_attention_seg2_fwd / sbl_attention_seg_bwd over the full
    batch at the same (seed, offset): o, p and dq of positions 0 and L-1 bit for bit (dropout 0.3), dK / dV (dout zero on
    the other rows) within the float64 bounds.  Prefixes up to 16 rows: both sides run the one-wavefront kernels."""
    c, drop_p = case, 0.3
    HD = c.H * 64
    full = A.Case(c.name, "seg2", c.B, c.H, c.segL, c.Lk, None, 1, (), None, None)
    sets_c = [Operands(c, _inputs(c.name, "flat", d), "contig") for d in (0, 1)]
    outs_c = run_forward(ops, c, sets_c, drop_p)
    rows = []                                  # full row of every compact row
    off = 0
    for L in c.segL:
        for b in range(c.B):
            rows += [off + b * L + kk * (L - 1) for kk in range(min(2, L))]
        off += c.B * L
    rows = np.array(rows)
    sets_f = []
    for d in (0, 1):
        inp = dict(_inputs(c.name, "flat", d))
        qf = A.detfill.uniform("ar.%s.qfull%d" % (c.name, d), (off, HD))
        qf[rows] = inp["q"]
        dof = np.zeros((off, HD), dtype=np.float32)
        dof[rows] = inp["do"]
        inp["q"], inp["do"] = qf, dof
        sets_f.append(Operands(full, inp, "contig"))
    outs_f = run_forward(ops, full, sets_f, drop_p)
    for d in (0, 1):
        assert np.array_equal(outs_c[d]["o"], outs_f[d]["o"][rows])
        pf = outs_f[d]["p"]
        for prc, prf in zip(A.problems(c), A.problems(full)):
            sel = [0, prf["Lq"] - 1][:prc["Lq"]]
            assert np.array_equal(outs_c[d]["p"][prc["pidx"]], pf[prf["pidx"]][sel])
        run_backward(ops, c, sets_c[d], drop_p, OFFSETS[d])
        run_backward(ops, full, sets_f[d], drop_p, OFFSETS[d])
        gc, gf = sets_c[d].backward_out({}), sets_f[d].backward_out({})
        assert np.array_equal(gc["dq"], gf["dq"][rows])
        ref = _reference(c.name, "flat", drop_p, d)
        ratios = A.compare(ref, gf, ("dk", "dv"))
        print(c.name, d, ratios)
        assert all(r <= 1.0 for r in ratios.values()), ratios


@pytest.mark.parametrize("name", ["wg_mask7x11", "wg_mask29x29", "wg_mask33x64"])
def test_fully_masked_row_under_a_tensor_mask(ops, name):
    """Library-defined behaviour (include/sbl_hip.h), not a parity claim - the reference's softmax of an all -inf row is NaN:
    p and o of the row are exactly 0, backward gives finite gradients, a zero dq row and no contribution to dK / dV."""
    c = A.CASE[name]
    for family in A.FAMILIES:
        for drop_p in (0.0, 0.3):
            sets, outs = run_case(ops, c, "contig", family, drop_p, full_row=True)
            out = outs[0]
            L, Lk = c.segL[0], c.Lk
            row = (c.B - 1) * L + 2
            assert np.all(out["o"][row] == 0) and np.all(out["dq"][row] == 0)
            for h in range(c.H):
                at = ((h * c.B + c.B - 1) * L + 2) * Lk
                assert np.all(out["p"][at:at + Lk] == 0)
            assert all(np.all(np.isfinite(out[n])) for n in ("p", "o", "dq", "dk", "dv"))


def test_abi_refusals_near_the_routes(ops):
    """Non-zero status, a message from sbl_last_error, nothing launched (the sentinel-filled outputs are untouched)."""
    from sbl_for_multilingual_lip_reading_amd import _lib
    lib = _lib.load()
    B, H = 3, 2
    HD = H * 64
    x = torch.zeros(B * 70 * 3, 3 * HD, device=DEV)
    o = torch.full((B * 70 * 3, 3 * HD), SENT, device=DEV)
    p = torch.full((H * B * 70 * 70 * 3,), SENT, device=DEV)
    m = torch.zeros(B * 70 * 70, dtype=torch.uint8, device=DEV)
    X, O, P, s = x.data_ptr(), o.data_ptr(), p.data_ptr(), ops._s()

    def seg_fwd(segL, Lk, ldq=HD, mk=0, mask=None):
        return lib.sbl_attention_seg_fwd(X, ldq, X, HD, X, HD, O, HD, P, mk, mask, B, H, _arr(segL), len(segL), Lk, A.SCALE, 0.0, None, 0, s)

    calls = {
        "Lk_fixed = 65": lambda: seg_fwd((5,), 65),
        "a segment of 65 rows": lambda: seg_fwd((3, 65), 0),
        "ldq = H*64 + 2": lambda: seg_fwd((5,), 13, ldq=HD + 2),
        "tensor mask with two segments": lambda: seg_fwd((5, 3), 13, mk=2, mask=m.data_ptr()),
        "Lk_fixed = 65, backward": lambda: lib.sbl_attention_seg_bwd(X, HD, X, HD, X, HD, X, HD, P, O, HD, O, HD, O, HD, B, H, _arr((5,)), 1, 65,
                                                                     A.SCALE, 0.0, None, 0, s),
        "Lk_fixed = 33 on ends2_fwd": lambda: lib.sbl_attention_ends2_fwd(X, X, HD, X, X, HD, X, X, HD, O, O, HD, P, P, B, H, _arr((5, 2)), 2, 33,
                                                                          A.SCALE, 0.0, None, 0, 1, s),
        "Lk_fixed = 33 on ends_bwd": lambda: lib.sbl_attention_ends_bwd(X, HD, X, HD, X, HD, X, HD, P, O, HD, O, HD, O, HD, B, H, _arr((5, 2)), 2, 33,
                                                                        A.SCALE, 0.0, None, 0, s),
        "kv_group not dividing B": lambda: lib.sbl_attention_seg_grouped_fwd(X, HD, X, HD, X, HD, O, HD, B, H, _arr((5,)), 1, 13, 2, A.SCALE, 0.0,
                                                                             None, 0, s),
    }
    for what, fn in calls.items():
        rc = fn()
        assert rc != 0, what
        assert lib.sbl_last_error().decode("utf-8", "replace").strip(), what
    torch.cuda.synchronize()
    assert bool((o == SENT).all()) and bool((p == SENT).all())


# --------------------------------------------------------------------------- the softmax of the decode-step kernels
def _step_check(out, q, K, V, what):
    ref, bound = A.step_reference(q, K, V)
    ratio = float((np.abs(out.astype(np.float64) - ref) / bound).max())
    print(what, "largest |err| / bound = %.3g" % ratio)
    assert np.all(np.isfinite(out)) and ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize("n_prev", [13, 63])
def test_decode_attn_step_peaked(ops, n_prev):
    """sbl_decode_attn_step (append mode) against float64 with the peaked family: score spreads beyond 87 inside rows that
    hold a probability near 1.  The float64 comparison of tests/test_seq2seq_gpu.py with the bounds of attention_routes."""
    B, H, Lcap = 5, 8, 64
    HD = H * 64
    kc, vc = (A.detfill.uniform("ar.step.%s%d" % (n, n_prev), (B, Lcap, HD)) for n in "kv")
    kn, vn, q = (A.detfill.uniform("ar.step.%s%d" % (n, n_prev), (B, HD)) for n in ("kn", "vn", "q"))
    K, V = kc[:, :n_prev + 1].copy(), vc[:, :n_prev + 1].copy()
    K[:, n_prev], V[:, n_prev] = kn, vn
    q = A.peak_rows(q, K)
    qkv = torch.from_numpy(np.concatenate([q, kn, vn], 1)).to(DEV)
    kd, vd = torch.from_numpy(kc).to(DEV), torch.from_numpy(vc).to(DEV)
    out = torch.full((B, HD), SENT, device=DEV)
    ops.decode_attn_step(qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:], kd, vd, Lcap, out, H, n_prev, True)
    torch.cuda.synchronize()
    _step_check(out.cpu().numpy(), q, K, V, "decode step n_prev=%d" % n_prev)


@pytest.mark.parametrize("n_prev", [13, 63])
def test_beam_attn_step_peaked(ops, n_prev):
    """sbl_beam_attn_step (append mode, W = 3, a scrambled ancestry table) against float64 with the peaked family."""
    N, W, H, Lcap = 3, 3, 8, 64
    S, HD = N * W, H * 64
    kc, vc = (A.detfill.uniform("ar.beam.%s%d" % (n, n_prev), (S, Lcap, HD)) for n in "kv")
    kn, vn, q = (A.detfill.uniform("ar.beam.%s%d" % (n, n_prev), (S, HD)) for n in ("kn", "vn", "q"))
    anc = ((A.detfill.uniform("ar.beam.anc%d" % n_prev, (S, Lcap)).astype(np.float64) + 1.0) * 0.5 * S).astype(np.int32).clip(0, S - 1)
    j = np.arange(n_prev)
    K = np.concatenate([kc[anc[:, :n_prev], j], kn[:, None]], 1)
    V = np.concatenate([vc[anc[:, :n_prev], j], vn[:, None]], 1)
    q = A.peak_rows(q, K)
    qkv = torch.from_numpy(np.concatenate([q, kn, vn], 1)).to(DEV)
    kd, vd, ad = torch.from_numpy(kc).to(DEV), torch.from_numpy(vc).to(DEV), torch.from_numpy(anc).to(DEV)
    out = torch.full((S, HD), SENT, device=DEV)
    ops.beam_attn_step(qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:], kd, vd, Lcap, ad, out, W, H, n_prev, True)
    torch.cuda.synchronize()
    _step_check(out.cpu().numpy(), q, K, V, "beam step n_prev=%d" % n_prev)
