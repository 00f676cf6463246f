"""CPU checks of the dropout-site bookkeeping helpers (tests/dropout_sites.py, tests/dropout_reference.py): the canonical
position makes folded and whole-buffer offsets comparable, the audits flag the ledgers they exist to flag, the recorder sees
every offset of a launch without launching anything, the per-rank default seeds cannot alias each other's streams, and the
float64 reference of tests/test_train_dropout_gpu.py moves far outside its bounds when one site draws another site's mask."""
import ctypes

import numpy as np
import pytest
import torch

import attention_routes as AR
import decoder_rows_reference as RR
import dropout_reference as DR
import dropout_sites as DS
from oracle import sbl_oracle as O

D = 512


# --------------------------------------------------------------------------- canonical position
def test_canonical_position_of_a_folded_offset():
    """canon(fold(o, base), i) == canon(o, base + i): for the restated fold and for the one the stage-batched decoder uses."""
    from sbl_for_multilingual_lip_reading_amd.transformer import decoder_stages
    rng = np.random.RandomState(3)
    bases = [0, 1, 511, 512, 3 * 136 * 512, (1 << 31) - 1, 1 << 31, (1 << 40) - 3, 1 << 40] + [int(b) for b in rng.randint(0, 1 << 40, 50, dtype=np.int64)]
    offs = [0, 1, 2, 63, 4095, 4096] + [int(o) for o in rng.randint(0, 4097, 20)]
    for base in bases:
        for o in offs:
            for f in (DS.fold(o, base), decoder_stages._fold(o, base)):
                assert 0 <= f <= DS.M64
                for i in (0, 1, 12345, (1 << 33) + 7):
                    assert DS.canon(f, i) == DS.canon(o, base + i), (o, base, i)
            assert DS.unfold(DS.fold(o, base), base) == o
    # ... and equal canonical positions are equal random numbers, different ones are not (one seed)
    idx = np.arange(64, dtype=np.uint64)
    a = AR.rand_u32(0x5B1C0FFEE, DS.fold(7, 1000), idx)
    assert np.array_equal(a, AR.rand_u32(0x5B1C0FFEE, 7, idx + np.uint64(1000)))
    assert not np.array_equal(a, AR.rand_u32(0x5B1C0FFEE, 7, idx + np.uint64(999)))


def test_keep_scale_and_mask_builder():
    assert DS.keep_scale(0.1) == np.float32(1.0) / (np.float32(1.0) - np.float32(0.1)) and DS.keep_scale(0.5) == np.float32(2.0)
    m = DS.mask_range(5, 3, 100, 4096, 0.5)
    assert m.dtype == np.bool_ and np.array_equal(m, AR.keep_mask(5, 3, np.arange(100, 4196, dtype=np.uint64), 0.5))
    assert 0.45 < m.mean() < 0.55
    assert np.array_equal(DS.mask(5, 3, [100, 4195], 0.5), m[[0, -1]])


# --------------------------------------------------------------------------- index table
def test_index_table_restates_the_documented_layouts():
    from sbl_for_multilingual_lip_reading_amd import _lib
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import ends_rows
    takes_offset = sorted(n for n, s in _lib.SIGNATURES.items() if _lib.U64 in s)
    assert takes_offset == sorted(DS.INDEX_TABLE), set(takes_offset) ^ set(DS.INDEX_TABLE)
    B, segL = 3, (1, 2, 5, 16)
    rows = DS._ends_full_rows(B, segL)
    assert rows == list(RR.ends_full_rows(B, segL)) == ends_rows(B, segL)
    assert DS._idx_ends_rows((B, segL, len(segL), D)) == DS._merge((r * D, (r + 1) * D) for r in rows)
    # the compact cross-attention draws exactly the probabilities attention_routes documents for an "ends" case
    c = AR.CASE["ends_n3"]
    want = sorted(int(v) for pr in AR.problems(c) for v in AR.documented_mask_index(c, pr).ravel())
    got = [i for a, b in DS._idx_att_ends((c.B, c.H, c.segL, len(c.segL), c.Lk)) for i in range(a, b)]
    assert got == want
    assert DS._idx_att_seg((B, 8, segL, 4, 0)) == [(0, 8 * B * sum(L * L for L in segL))]
    assert DS._idx_att_seg((B, 8, segL, 4, 5)) == [(0, 8 * B * sum(segL) * 5)]


def test_recorder_sees_every_offset_and_launches_nothing(monkeypatch):
    from sbl_for_multilingual_lip_reading_amd import _lib, ops
    seen = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: seen.append(name))
    monkeypatch.setattr(ops, "call", _lib.call)
    stub = _lib.call
    segs = (ctypes.c_int * 2)(3, 4)
    with DS.recording() as led:
        assert ops.call is _lib.call and _lib.call is not stub
        ops.call("sbl_dropout", 1, 2, 1025, 0.5, 99, 7, 0)
        ops.call("sbl_add_pe", 1, 2, 3, 4, 5, 6, 0)                    # no offset: no record
        with led.backward():
            ops.call("sbl_dropout", 1, 2, 1025, 0.5, 99, 7, 0)
        ops.call("sbl_add_layernorm2_ends_fwd", *range(14), 3, segs, 2, D, 1e-5, 0.1, None, 11, 12, 0)
    assert ops.call is stub and _lib.call is stub
    assert seen == ["sbl_dropout", "sbl_add_pe", "sbl_dropout", "sbl_add_layernorm2_ends_fwd"]
    assert [(r.name, r.phase, r.offset, r.slot, r.null_seed) for r in led] == [
        ("sbl_dropout", "fwd", 7, 0, False), ("sbl_dropout", "bwd", 7, 0, False),
        ("sbl_add_layernorm2_ends_fwd", "fwd", 11, 0, True), ("sbl_add_layernorm2_ends_fwd", "fwd", 12, 1, True)]
    assert led[0].ints == (1025,) and led[0].p == 0.5 and led[0].ranges() == [(0, 1025)]
    assert led[2].ints == (3, (3, 4), 2, D) and abs(led[2].p - 0.1) < 1e-7
    assert led[2].count() == 3 * 4 * D                                 # min(2, L) rows per sequence
    assert DS.audit_seed(led) == [led[2], led[3]]


# --------------------------------------------------------------------------- audits on hand-made ledgers
def _stage_ledger(N=3, segs=((1, 2), (3,)), offs=(1, 2, 3), bwd_offs=None, base_shift=0):
    """Two row sites and (offs[2]) an embedding over the stages `segs`, forward folded per stage, backward whole-buffer."""
    led = DS.Ledger()
    r0 = 0
    for s, segL in enumerate(segs):
        base = r0 * D - (base_shift if s else 0)
        M = N * sum(segL)
        led.append(DS.Record("sbl_add_layernorm2_fwd", 0.1, DS.fold(offs[0], base), False, (M, D), 0))
        led.append(DS.Record("sbl_add_layernorm2_fwd", 0.1, DS.fold(offs[1], base), False, (M, D), 1))
        led.append(DS.Record("sbl_embed_pe_drop2_fwd", 0.1, DS.fold(offs[2], base), False, (17, N, tuple(segL), len(segL), D, 58), 0))
        r0 += M
    for o in (offs if bwd_offs is None else bwd_offs):
        led.append(DS.Record("sbl_dropout", 0.1, o, False, (r0 * D,), 0, "bwd"))
    return led


def test_clean_ledger_passes():
    led = _stage_ledger()
    assert DS.audit_disjoint(led) == [] and DS.audit_backward(led) == ([], []) and DS.audit_seed(led) == []
    DS.audit(led)


def test_audit_flags_two_sites_sharing_an_offset():
    led = _stage_ledger(offs=(1, 2, 2))
    bad = DS.audit_disjoint(led)
    assert bad and all({a.name, b.name} == {"sbl_add_layernorm2_fwd", "sbl_embed_pe_drop2_fwd"} for a, b in bad)
    with pytest.raises(AssertionError, match="share random numbers"):
        DS.audit(led)


def test_audit_flags_a_stage_base_one_row_into_its_neighbour():
    led = _stage_ledger(base_shift=D)
    bad = DS.audit_disjoint(led)
    assert len(bad) == 3 and all(a.name == b.name and a.slot == b.slot for a, b in bad)      # each site against its own earlier stage
    extra, missing = DS.audit_backward(led)
    assert missing == [] and len(extra) == 3      # the last row of every site is drawn by backward only
    with pytest.raises(AssertionError):
        DS.audit(led)


def test_audit_flags_a_backward_draw_without_a_forward_twin():
    led = _stage_ledger(bwd_offs=(1, 2, 4))
    extra, missing = DS.audit_backward(led)
    assert extra and missing and DS.audit_disjoint(led) == []
    led = _stage_ledger()
    led[0].null_seed = True
    with pytest.raises(AssertionError, match="null seed"):
        DS.audit(led)


def test_rank_seeds_do_not_alias_each_others_streams():
    """Rank r's stream o would be rank s's stream o + k if seed_r = seed_s + k * C1 (the hash adds C1 * (offset + 1) to the
    seed): no such k with |k| < 1000 among 64 ranks, and the seeds are distinct."""
    seeds = [DS.rank_seed(r) for r in range(64)]
    assert seeds[0] == DS.DEFAULT_SEED and len(set(seeds)) == 64 and all(0 <= s < (1 << 63) for s in seeds)
    shifts = {(k * DS.C1) & DS.M64 for k in range(-999, 1000)}
    for r in range(64):
        for s in range(64):
            if r != s:
                assert ((seeds[r] - seeds[s]) & DS.M64) not in shifts, (r, s)
    assert DS.bumped(DS.DEFAULT_SEED) == (DS.DEFAULT_SEED * 6364136223846793005 + 1442695040888963407) % (1 << 64)


# --------------------------------------------------------------------------- plans and the reference
def test_plans_of_both_decoder_paths_address_the_same_layout():
    """A per-stage plan over folded offsets and the whole-buffer plan over the sites' own offsets are the same masks."""
    N, T, nl, p = 3, 5, 2, 0.1
    coins = [False, True, False, False, True] + [False] * 10 + [True]
    assert DR.stages_of(coins) == [(0, 1), (2, 4), (5, 15)] and DR.stages_of([False] * 16) == [(0, 15)]
    full = DR.seg_bases(N, T, tuple(range(1, 17)))
    assert full[2] == (N * 3 * D, 8 * N * 5, 8 * N * T * 3)
    raw = {s: 3 + i for i, s in enumerate(DR.site_order(nl))}
    recs = []
    for i0, i1 in DR.stages_of(coins):
        segL = tuple(range(i0 + 1, i1 + 2))
        M = N * sum(segL)
        for (d, n, k) in [(0, -1, -1), (1, -1, -1)] + [(d, n, k) for n in range(nl) for k in range(5) for d in (0, 1)]:
            name = "sbl_embed_pe_drop2_fwd" if k < 0 else "sbl_attention_seg2_fwd" if k in (0, 2) else "sbl_add_layernorm2_fwd"
            ints = (17, N, segL, len(segL), D, 58) if k < 0 else (N, 8, segL, len(segL), 0 if k == 0 else T) if k in (0, 2) else (M, D)
            recs.append(DS.Record(name, p, DS.fold(raw[(d, n, k)], DR._site_base(full[i0], k)), False, ints, d))
    assert DR.batched_site_offsets(recs, N, T, nl, coins) == raw
    recs[5].offset = DS.fold(raw[(1, 0, 1)], DR._site_base(full[0], 1) + D)          # a stage base off by one row
    with pytest.raises(AssertionError, match="un-fold"):
        DR.batched_site_offsets(recs, N, T, nl, coins)
    plan = DR.batched_decoder_plan(raw, N, T, nl, p)
    assert len(plan) == 16 * (2 + 10 * nl)
    us = sorted((DS.canon(o, b), DS.canon(o, b) + c) for o, b, _, c in plan)
    assert all(a[1] <= b[0] for a, b in zip(us, us[1:]))


@pytest.fixture(scope="module")
def small_step():
    """The smallest decoder case of the GPU test (B = 3, T = 5, 1 + 2 layers, "varied" gains) under a synthetic ledger."""
    from sbl_for_multilingual_lip_reading_amd import detfill
    N, T, ne, nd, p, salt = 3, 5, 1, 2, 0.1, 0
    coins = [bool(c) for c in (0, 1, 0, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0)]
    feats = torch.from_numpy(detfill.uniform("train_dropout.feats", (N, T, 512), salt)).double()
    _, l2r, r2l = detfill.synthetic_batch(N, 1, 1, 1, salt)
    l2r, r2l = torch.from_numpy(l2r), torch.from_numpy(r2l)

    def run(swap=None, fed=None):
        sd = DR.to64(O.make_state_dict(ne, nd, salt, gains="varied"))
        out = DR.sbl_step(sd, feats, l2r, r2l, coins, ne, nd, p, DS.DEFAULT_SEED, DR.synthetic_batched_plan(N, T, ne, nd, p, swap), fed)
        out["loss"].backward()
        return out, sd

    base, sd = run()
    fed = [torch.zeros(N, 16, dtype=torch.long), torch.zeros(N, 16, dtype=torch.long)]
    for i, al, ar in base["argmax"]:
        fed[0][:, i], fed[1][:, i] = al, ar
    return run, base, sd, fed


def test_reference_margins_of_the_small_step(small_step):
    _, base, sd, _ = small_step
    assert len(base["argmax"]) == 4 and base["margin"] > DR.MARGIN, base["margin"]
    assert base["pred_l2r"].dtype == torch.float64 and sd["decoder.tgt_word_emb.weight"].grad.dtype == torch.float64


@pytest.mark.parametrize("swap", [((1, 0, 1), (0, 0, 1)), ((0, 1, 4), (0, 1, 3)), ((0, -1, -1), (1, -1, -1)), ((1, 1, 2), (1, 0, 2))])
def test_reference_leaves_its_bounds_when_a_site_draws_another_sites_mask(small_step, swap):
    """One site's mask replaced by another site's (same tokens fed back): logits move by more than 10 x the logit bar and at
    least one gradient by more than 10 x its element-wise bound, so the GPU test fails on a mis-assigned mask."""
    run, base, sd, fed = small_step
    out, sd2 = run(swap, fed)
    dl = max(float((out[k] - base[k]).detach().abs().max()) for k in ("pred_l2r", "pred_r2l"))
    worst = max(float((sd2[k].grad - v.grad).abs().max()) / DR.grad_bound(v.grad)
                for k, v in sd.items() if v.grad is not None and k.startswith(("encoder", "decoder")))
    print("swap %s: max|dlogit| %.3e (bar %.0e)  worst gradient move / bound %.1f" % (swap, dl, DR.LOGIT_BAR, worst))
    assert dl > 10 * DR.LOGIT_BAR and worst > 10, (dl, worst)
