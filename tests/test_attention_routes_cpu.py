"""CPU checks of tests/attention_routes.py: the case table lands on the leaves written next to it and covers the dispatch of
csrc/attention.hip, the error bounds hold for a float32 emulation with room to spare and still catch planted bugs, the dropout
hash restatement reproduces hand-computed values, and the input families do what their names say.  No GPU, no torch."""
import functools

import numpy as np
import pytest

import attention_routes as A

SEED, OFFSET = 1234567, 7


@functools.lru_cache(maxsize=None)
def _run(name, family, drop_p, mutant=None):
    c = A.CASE[name]
    inp = A.make_inputs(c, family)
    ref = A.reference(c, inp, drop_p, SEED, OFFSET)
    out = A.emulate_f32(c, inp, drop_p, SEED, OFFSET, mutant)
    return A.compare(ref, out), A.exact_failures(c, inp, ref, out, family)


def _families(c):
    return A.FAMILIES + (("planted",) if c.name in A.PLANTED else ())


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_case_lands_on_its_leaf(case):
    fwd, bwd = A.route_case(case)
    assert fwd == case.fwd, (case.name, fwd)
    assert bwd == case.bwd, (case.name, bwd)
    assert len(case.segL) <= A.MAX_SEG and max(case.segL) <= 64 and case.Lk <= 64 and case.B % case.kvg == 0


def test_table_reaches_every_leaf_and_no_unreachable_one():
    leaves = A.all_leaves()
    for side, hit in (("fwd", {c.fwd for c in A.CASES}), ("bwd", {c.bwd for c in A.CASES if c.bwd is not None})):
        reachable = {leaf for leaf, ok in leaves[side].items() if ok}
        assert not reachable - hit, (side, "not reached", sorted(reachable - hit, key=str))
        assert not hit - reachable, (side, "the enumeration calls these unreachable", sorted(hit - reachable, key=str))
    # one-wavefront self-attention has Lk = L <= 16: its two-tile form cannot be reached
    assert not leaves["fwd"][A.Leaf("seg", "small", 2, "self", "none", 4, None)]


def test_table_has_the_sizes_the_issue_names():
    by = lambda **kw: [c for c in A.CASES if all(getattr(c, k) == v for k, v in kw.items())]
    assert all(c.B == 3 and c.H in (2, 8) or (c.B, c.H) == (1, 1) for c in A.CASES)
    for kernel in ("small", "qtile", "workgroup"):
        assert any(c.H == 8 and c.fwd.kernel == kernel for c in A.CASES), kernel
    small11 = {(c.fwd.entry, c.fwd.tiles, c.fwd.kv) for c in by(B=1, H=1)}
    assert {(c.fwd.entry, c.fwd.tiles, c.fwd.kv) for c in A.CASES if c.fwd.kernel == "small"} <= small11      # three idle wavefronts
    plain_bwd = lambda c: c.bwd is not None and c.bwd.kernel == "small" and c.bwd.red == "none"
    assert {c.bwd for c in A.CASES if plain_bwd(c)} <= {c.bwd for c in by(B=1, H=1) if plain_bwd(c)}
    assert {c.Lk for c in A.CASES if c.fwd == A.Leaf("seg", "small", 2, "cross", "none", 4, None)} >= {29, 32}
    assert any(1 in c.segL and 16 in c.segL for c in by(entry="seg")) and any(len(c.segL) == 16 for c in by(entry="seg", Lk=0))
    assert {c.segL[0] for c in A.CASES if c.fwd.kernel == "qtile" and c.Lk == 0} >= {17, 29, 32}
    assert {c.fwd.fallback for c in A.CASES if c.fwd.kernel == "workgroup"} == {"tensor-mask", "keys>32", "rows>32", "multiseg>16", "o-unaligned"}
    assert {len(c.segL) for c in A.CASES if c.bwd and c.bwd.red == "lds" and c.bwd.entry == "seg" and c.bwd.kernel == "small"} >= {2, 8, 9, 16}
    assert {c.bwd.fallback for c in A.CASES if c.bwd} >= {"grad-stride", "grad-unaligned"}
    ends = by(entry="ends")
    assert {len(c.segL) for c in ends} >= {1, 3, 9, 16} and {c.Lk for c in ends} >= {29, 32}
    assert any(1 in c.segL for c in ends) and any(2 in c.segL for c in ends) and any(max(c.segL) > 2 for c in ends)
    assert {c.kvg for c in by(entry="grouped", B=3)} == {1, 3} and {c.fwd.kernel for c in by(entry="grouped")} == {"small", "qtile", "workgroup"}
    assert {c.fwd.entry for c in by(entry="seg2")} == {"dual", "two"}
    assert max(max(A.q_lengths(c)) for c in A.CASES) <= 64


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_emulation_stays_inside_every_bound(case):
    """... by a factor of two at least: the bounds are not tuned to the emulation."""
    for family in _families(case):
        for drop_p in (0.0, 0.3):
            ratios, bad = _run(case.name, family, drop_p)
            assert not bad, (family, drop_p, bad)
            assert max(ratios.values()) <= 0.5, (family, drop_p, ratios)


# mutant -> (case, family, drop_p, an output that must leave its bound)
CAUGHT_BY = {
    "no_max": ("small_cross29_n5", "peaked", 0.0, "p"),
    "max16": ("small_cross29_n5", "peaked", 0.0, "p"),
    "causal_off1": ("small_self_causal", "flat", 0.0, "p"),
    "causal_qtile": ("qtile_self17_causal", "flat", 0.0, "p"),
    "mask_bji": ("wg_mask29x29", "flat", 0.0, "p"),
    "ends_step": ("ends_n3", "flat", 0.3, "o"),
    "no_poff": ("small_cross29_n5", "flat", 0.3, "o"),
    "ks_fwd_only": ("qtile_self29", "flat", 0.3, "dv"),
    "scale2_dq": ("wg_rows33_self", "flat", 0.0, "dq"),
    "dkv_last": ("wg_keys64_n2", "flat", 0.0, "dk"),
    "p_bh": ("small_self_causal", "flat", 0.0, "p"),
}


@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_bounds_catch_the_planted_mutant(mutant):
    name, family, drop_p, which = CAUGHT_BY[mutant]
    clean, bad = _run(name, family, drop_p)
    assert max(clean.values()) <= 0.5 and not bad
    ratios, _ = _run(name, family, drop_p, mutant)
    assert ratios[which] > 1.0, (mutant, name, ratios)


def test_rand_u32_reproduces_hand_computed_values():
    """z = seed + 0x9E3779B97F4A7C15 (offset + 1) + idx 0xD1B54A32D192ED03, two xor-shift-multiply rounds, high word: worked
    out with unbounded integers reduced mod 2^64 after every product.  The third and fourth have products that wrap."""
    for (seed, offset, idx), want in (((0, 0, 0), 3793791033), ((1234567, 7, 12345), 2595842412),
                                      (((1 << 64) - 1, 1 << 40, (1 << 33) + 5), 490768515),
                                      ((0x0123456789ABCDEF, 3, 1 << 62), 551710387)):
        assert int(A.rand_u32(seed, offset, [idx])[0]) == want
    assert A.drop_thresh(0.0) == 0 and A.drop_thresh(0.5) == 1 << 31
    assert A.drop_thresh(0.3) == 1288490240 and A.drop_thresh(0.1) == 429496736        # float32(p) * 2^32, truncated
    assert A.keep_scale(0.5) == np.float32(2.0)


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_keep_fraction(p):
    n = 1 << 16
    keep = A.keep_mask(SEED, OFFSET, np.arange(n), p)
    assert abs(keep.mean() - (1 - p)) < 4 * np.sqrt(p * (1 - p) / n)


def test_mask_index_functions():
    """Hand-worked indices of the three layouts, and problems() (what the emulation uses) against them on every case."""
    # B = 3, H = 2, segments (5, 16, 1) self: blocks of 2*3*25 = 150 and 2*3*256 = 1536 floats
    assert A.p_offsets((5, 16, 1), 3, 2, 0) == ([0, 150, 1686], 1692)
    assert A.mask_index_full((5, 16, 1), 3, 2, 0, 1, 1, 2, 3, 4) == 150 + ((1 * 3 + 2) * 16 + 3) * 16 + 4
    # query tiles over L = 29, Lk = 29: row 3 of the second tile is row 19 of the (H*B, 29, 29) block
    assert A.mask_index_qtile(29, 29, 3, 2, 1, 0, 1, 3, 7) == A.mask_index_full((29,), 3, 2, 0, 0, 1, 0, 19, 7) == (3 * 29 + 19) * 29 + 7
    # ends: full lengths (1, 2, 9), 29 keys: compact row 1 of segment 2 is position 8; of segment 1 position 1; L = 1 has only row 0
    full = A.p_offsets((1, 2, 9), 3, 2, 29)[0]
    assert A.mask_index_ends((1, 2, 9), 3, 2, 29, 2, 1, 0, 1, 5) == full[2] + ((1 * 3 + 0) * 9 + 8) * 29 + 5
    assert A.mask_index_ends((1, 2, 9), 3, 2, 29, 1, 0, 2, 1, 0) == full[1] + ((0 * 3 + 2) * 2 + 1) * 29
    assert A.mask_index_ends((1, 2, 9), 3, 2, 29, 0, 1, 1, 0, 28) == ((1 * 3 + 1) * 1 + 0) * 29 + 28
    for c in A.CASES:
        seen = np.zeros(A.p_offsets(A.q_lengths(c), c.B, c.H, c.Lk)[1], dtype=int)
        for pr in A.problems(c):
            assert np.array_equal(pr["midx"], A.documented_mask_index(c, pr)), c.name
            seen[pr["pidx"]] += 1
        assert np.all(seen == 1), c.name                     # the problems tile the probability buffer exactly once


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_input_families_do_what_their_names_say(case):
    """peaked: every row with at least two visible keys (a single visible key has p = 1 at any scale) has a float64 score
    spread above 87, a probability above 0.5 and one below 2^-126.  flat: no row has a spread above 87 or such a probability."""
    stats = {}
    for family in A.FAMILIES:
        inp = A.make_inputs(case, family)
        assert all(np.all(np.isfinite(inp[n])) for n in ("q", "k", "v", "do"))
        ref = A.reference(case, inp)
        rows = []
        for pr in A.problems(case):
            cols = slice(pr["h"] * 64, pr["h"] * 64 + 64)
            s = inp["q"][pr["qrows"], cols].astype(np.float64) @ inp["k"][pr["krows"], cols].astype(np.float64).T * A.SCALE
            vis = A.visible(case, pr, inp["mask"])
            p = ref["p"][0][pr["pidx"]]
            for i in range(pr["Lq"]):
                if vis[i].sum() >= 2:
                    rows.append((np.ptp(s[i][vis[i]]), p[i][vis[i]].max(), p[i][vis[i]].min()))
        stats[family] = np.array(rows).reshape(-1, 3)
    pk, fl = stats["peaked"], stats["flat"]
    assert len(pk) == len(fl)
    assert np.all(pk[:, 0] > 87) and np.all(pk[:, 1] > 0.5) and np.all(pk[:, 2] < 2.0 ** -126)
    assert np.all(fl[:, 0] < 87) and np.all(fl[:, 2] > 2.0 ** -126)


def test_planted_family():
    for name in A.PLANTED:
        c = A.CASE[name]
        inp = A.make_inputs(c, "planted")
        ref = A.reference(c, inp)
        onehot = 0
        for pr in A.problems(c):
            vis = A.visible(c, pr, inp["mask"])
            p = ref["p"][0][pr["pidx"]]
            cols = slice(pr["h"] * 64, pr["h"] * 64 + 64)
            if pr["Lk"] >= 2:
                assert np.array_equal(inp["k"][pr["krows"][0], cols], inp["k"][pr["krows"][1], cols])
                both = vis[:, 0] & vis[:, 1]
                assert np.array_equal(p[both, 0], p[both, 1])
            if c.B > 1 and pr["b"] == c.B - 1:               # q = 0: uniform over the visible keys
                assert np.allclose(p[vis], (vis / vis.sum(1, keepdims=True))[vis], rtol=1e-15)
            else:
                onehot += int((p.max(1) > 0.45).sum())       # near one-hot (0.5 each when the planted key is one of the copies)
                assert np.all(p.max(1) > 0.45)
        assert onehot > 0
