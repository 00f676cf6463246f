"""tests/cls_reference.py without a GPU: the float64 restatement of the classification heads and their loss is held to
float64 torch autograd (F.cross_entropy with ignore_index, .backward(gradient=gscale)); its derived bounds are held to a
float32 restatement of the loss rows that sums as the kernel does (one partial sum per lane over the passes, then a xor
butterfly) and must stay within 1x the bounds the GPU module allows 2x of; the exact cases are shown to lie in the exact
regime; and the last tests show that the comparison functions the GPU module uses (exact, check at 2x) flag the one-line
mistakes a kernel could make, each on the shape that exposes it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cls_reference as R

ids = lambda cases: [c["id"] for c in cases]
by_edge = lambda cases, edge: next(c for c in cases if c["id"].endswith(edge))


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def close(what, a, b, rel=1e-12):
    a, b = R.f64(a), R.f64(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    d = float(np.abs(a - b).max()) if a.size else 0.0
    assert d <= rel * max(float(np.abs(b).max()), 1e-300), (what, d)


# --------------------------------------------------------------------------- the tables name every edge
def test_tables_hit_every_tile_edge():
    ex = R.HEAD_EXACT
    assert {c["N"] for c in ex} >= {1, 3, 4, 5, 63, 64, 65, 256, 257, 300}
    assert {c["C1"] for c in ex} >= {1, 7, 8, 9, 127, 128, 129, 511, 512, 513, 1500}
    assert {c["C2"] for c in ex} >= {1, 2, 3, 16} and max(c["C2"] for c in ex) == R.MAX_C2
    assert {(c["T"], c["li"]) for c in ex} >= {(1, 0), (2, 0), (2, 1), (4, 0), (4, 2), (4, 3)}
    assert any((c["N"], c["C1"], c["C2"], c["T"]) == (300, 1500, 16, 4) for c in ex)
    assert 25 <= len(ex) <= 35 and len(set(ids(ex))) == len(ex)
    # a chunk of kn classes leaves wavefront w without work when kn <= 128 w
    tagged = {c["C1"] for c in ex if "empty-quarters" in c["id"]}
    assert tagged == {1, 7, 8, 127, 128, 513} and all((C1 % R.KC or R.KC) <= R.KC // 4 for C1 in tagged)
    assert {c["T"] for c in R.HEAD_REAL} == {3, 31} and max(c["N"] for c in R.HEAD_REAL) == 300
    assert {c["N"] for c in R.HEAD_REAL} >= {1, 4, 5, 64, 65, 256, 257} and {c["C1"] for c in R.HEAD_REAL} >= {8, 9, 128, 129, 512, 513, 1500}
    ls = R.LOSS_CASES
    assert {c["N"] for c in ls} == {1, 4, 5, 15, 16, 17, 33}
    assert {(c["C1"], c["C2"]) for c in ls} == {(1, 1), (2, 16), (63, 2), (64, 3), (65, 64), (129, 65), (1500, 2)}
    assert {c["spread"] for c in ls} == {3, 30, 80} and {c["gscale"] for c in ls} == {1.0, 0.37, -2.0, 0.0}
    assert {c["lw"] for c in ls} == {0.1, 0.0, 1.5} and any(c["ignore"] for c in ls)
    assert 20 <= len(ls) <= 30 and len(R.LOSS_BY_ID) == len(ls)
    for c in ls:                               # an all-equal row and a +60 peak in every case, valid rows in both heads
        o = R.loss_case(c)
        for h in (1, 2):
            x, t = o["l%d" % h], o["t%d" % h]
            assert (t != R.IGN).any()
            if c["N"] > 1 or h == 1:
                assert (x[0] == x[0, 0]).all() and t[0] != R.IGN
            if c["N"] > 1 or h == 2:
                top = np.sort(R.f64(x), 1)
                peaked = (top[:, -1] - top[:, -2] > 59.99) if x.shape[1] > 1 else np.ones(len(x), bool)
                assert (peaked & (t != R.IGN)).any()
        if c["ignore"]:
            assert (o["t1"] == R.IGN).any() and (o["t2"] == R.IGN).any()


@pytest.mark.parametrize("case", R.HEAD_EXACT + R.HEAD_NULL, ids=ids(R.HEAD_EXACT + R.HEAD_NULL))
def test_exact_cases_stay_in_the_exact_regime(case):
    o = R.exact_head_case(case)                # asserts sum|terms| < 2^24 in units of 1/T
    assert o["grid_max"] < 2.0 ** 24
    if (case["N"], case["C1"]) == (300, 1500):
        assert o["grid_max"] < 6400 * 4        # the largest shape: far below 2^24
    for k in ("enc", "w1", "b1", "w2", "b2", "d1", "d2"):
        assert o[k].dtype == np.float32 and np.abs(o[k]).max() <= 3 and np.array_equal(o[k], np.rint(o[k]))
    fw = R.head_fwd(o["enc"], o["w1"], o["b1"], o["w2"], o["b2"], case["li"])
    pooled = R.f32(fw["pooled"])
    bw = R.head_bwd(o["enc"], pooled, o["d1"], o["d2"], o["w1"], o["w2"], case["li"], accumulate=1, preset=o["preset"])
    T = case["T"]
    for k, v in list(fw.items()) + list(bw.items()):
        assert np.array_equal(R.f64(R.f32(v)), v), k                      # a float32 ...
        assert np.array_equal(np.rint(v * T), v * T), k                   # ... on the grid of 1/T
    # d_enc on the li row: a float32 add of two exact values
    de = R.f32(R.f32(R.f64(o["d1"]) @ R.f64(o["w1"]) / T) + R.f32(R.f64(o["d2"]) @ R.f64(o["w2"])))
    assert np.array_equal(de, R.f32(bw["d_enc"][:, case["li"]]))


# --------------------------------------------------------------------------- against float64 torch autograd
@pytest.mark.parametrize("case", R.LOSS_CASES, ids=ids(R.LOSS_CASES))
def test_loss_reference_against_torch_autograd(case):
    o = R.loss_case(case)
    lw, gs = float(np.float32(case["lw"])), float(np.float32(case["gscale"]))
    l1, l2 = t64(o["l1"]).requires_grad_(True), t64(o["l2"]).requires_grad_(True)
    t1, t2 = torch.from_numpy(o["t1"]), torch.from_numpy(o["t2"])
    loss = F.cross_entropy(l1, t1, ignore_index=R.IGN) + lw * F.cross_entropy(l2, t2, ignore_index=R.IGN)
    loss.backward(gradient=torch.tensor(gs, dtype=torch.float64))
    stats = []
    for l, t in ((l1, t1), (l2, t2)):
        v = t != R.IGN
        stats += [float(F.cross_entropy(l.detach(), t, ignore_index=R.IGN, reduction="sum")), float(v.sum()),
                  float(((l.detach().argmax(1) == t) & v).sum())]
    fw = R.loss_fwd(o["l1"], o["l2"], o["t1"], o["t2"], case["lw"])
    bw = R.loss_bwd(o["l1"], o["l2"], o["t1"], o["t2"], case["lw"], case["gscale"])
    close("loss", fw["loss"], loss.item())
    close("stats", fw["stats"], stats)
    assert fw["stats"][[1, 2, 4, 5]].tolist() == [stats[i] for i in (1, 2, 4, 5)]
    # 1e-12 of the tensor's largest entry; the gradient of an all-equal or saturated row is a difference of O(1) softmax terms
    close("d1", bw["d1"], l1.grad.numpy())
    close("d2", bw["d2"], l2.grad.numpy())
    assert bw["rows1"].all() and bw["rows2"].all()
    for h, t in ((1, o["t1"]), (2, o["t2"])):
        ign = t == R.IGN
        assert not bw["d%d" % h][ign].any() and not bw["b_d%d" % h][ign].any()
        assert (bw["b_d%d" % h][~ign] >= R.TINY).all()
    assert np.isfinite(fw["b_loss"]) and fw["b_loss"] > 0 and (fw["b_stats"][[1, 2, 4, 5]] == 0).all()


def test_loss_reference_nan_and_contract_rows():
    """A head without valid rows: NaN like torch's mean reduction, zero gradient.  A target outside [0, C) that is not
    ignore_id: NaN row loss, counted valid, never correct, and its row is taken out of the gradient comparison."""
    o = R.loss_case(R.LOSS_BY_ID["N5-C65x64-spread3-g1-lw0.1-ign-loss-bwd-fifth-row"])
    t2 = np.full(5, R.IGN, dtype=np.int64)
    fw = R.loss_fwd(o["l1"], o["l2"], o["t1"], t2, 0.1)
    ref = F.cross_entropy(t64(o["l1"]), torch.from_numpy(o["t1"]), ignore_index=R.IGN) + \
        0.1 * F.cross_entropy(t64(o["l2"]), torch.from_numpy(t2), ignore_index=R.IGN)
    assert np.isnan(fw["loss"]) and bool(torch.isnan(ref)) and fw["stats"][3:].tolist() == [0.0, 0.0, 0.0]
    bw = R.loss_bwd(o["l1"], o["l2"], o["t1"], t2, 0.1, 1.0)
    assert not bw["d2"].any() and not bw["b_d2"].any() and bw["d1"].any()
    t1 = o["t1"].copy()
    t1[2] = -5
    fw = R.loss_fwd(o["l1"], o["l2"], t1, o["t2"], 0.1)
    assert np.isnan(fw["loss"]) and np.isnan(fw["stats"][0]) and np.isfinite(fw["stats"][3])
    assert fw["stats"][1] == float((t1 != R.IGN).sum())
    bw = R.loss_bwd(o["l1"], o["l2"], t1, o["t2"], 0.1, 1.0)
    assert bw["rows1"].tolist() == [True, True, False, True, True] and bw["rows2"].all()


@pytest.mark.parametrize("case", [R.HEAD_REAL[1], R.HEAD_REAL[3], R.HEAD_REAL[6], R.HEAD_EXACT[26]],
                         ids=ids([R.HEAD_REAL[1], R.HEAD_REAL[3], R.HEAD_REAL[6], R.HEAD_EXACT[26]]))
def test_head_reference_against_torch_autograd(case):
    o = R.real_head_case(case) if case in R.HEAD_REAL else R.exact_head_case(case)
    li, T = case["li"], case["T"]
    e, W1, B1, W2, B2 = [t64(o[k]).requires_grad_(True) for k in ("enc", "w1", "b1", "w2", "b2")]
    pooled = e.mean(1)
    l1 = pooled @ W1.t() + B1
    l2 = e[:, li] @ W2.t() + B2
    ((l1 * t64(o["d1"])).sum() + (l2 * t64(o["d2"])).sum()).backward()
    fw = R.head_fwd(o["enc"], o["w1"], o["b1"], o["w2"], o["b2"], li)
    close("pooled", fw["pooled"], pooled.detach().numpy())
    close("pooled_t", fw["pooled_t"], pooled.detach().numpy().T)
    close("logits1", fw["logits1"], l1.detach().numpy())
    close("logits2", fw["logits2"], l2.detach().numpy())
    bw = R.head_bwd(o["enc"], fw["pooled"], o["d1"], o["d2"], o["w1"], o["w2"], li)
    for k, p in zip(R.OUT_BWD, (e, W1, B1, W2, B2)):
        close(k, bw[k], p.grad.numpy())
    # accumulate adds the preset to the four parameter gradients and leaves d_enc alone; NULL outputs are absent
    acc = R.head_bwd(o["enc"], fw["pooled"], o["d1"], o["d2"], o["w1"], o["w2"], li, accumulate=1, preset=o["preset"])
    assert np.array_equal(acc["d_enc"], bw["d_enc"])
    for k in R.OUT_BWD[1:]:
        assert np.array_equal(acc[k], bw[k] + R.f64(o["preset"][k]))
    for want in R.NULL_COMBOS.values():
        part = R.head_bwd(o["enc"], fw["pooled"], o["d1"], o["d2"], o["w1"], o["w2"], li, want=want)
        assert set(part) == set(want) and all(np.array_equal(part[k], bw[k]) for k in want)
    # the bounds are positive where the sums have terms, and tiny next to them
    fb = R.head_fwd_bounds(o["enc"], o["w1"], o["b1"], o["w2"], o["b2"], li)
    bb = R.head_bwd_bounds(o["enc"], fw["pooled"], o["d1"], o["d2"], o["w1"], o["w2"], li)
    for k, v in list(fb.items()) + list(bb.items()):
        ref = fw[k] if k in fw else bw[k]
        assert v.shape == ref.shape and (v >= 0).all() and np.isfinite(v).all(), k
    assert (fb["logits1"] <= (R.D + T + 6) * R.U * (np.abs(R.f64(o["enc"])).mean(1) @ np.abs(R.f64(o["w1"])).T + np.abs(R.f64(o["b1"]))) * (1 + 1e-12)).all()


# --------------------------------------------------------------------------- float32 restatement of the loss rows
def _exp32(a):
    """A host expf: the float64 exponential rounded to float32 (half an ulp; the same on every machine)."""
    return np.exp(R.f64(a)).astype(np.float32)


def _log32(a):
    return np.log(R.f64(a)).astype(np.float32)


def _wave_sum32(v):
    v = v.astype(np.float32)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    assert v.dtype == np.float32
    return v[:, 0]


def _lane_sum32(vals):
    """sum over c = lane, lane + 64, .. in order per lane, then the butterfly."""
    N, C = vals.shape
    P = R.cdiv(C, 64)
    pad = np.zeros((N, P * 64), np.float32)
    pad[:, :C] = vals
    pad = pad.reshape(N, P, 64)
    s = np.zeros((N, 64), np.float32)
    for k in range(P):
        s = s + pad[:, k]
    return _wave_sum32(s)


def _loss32(x, tgt, lwscale, gscale):
    """float32 throughout: (row losses, valid, loss sum over 16 wavefront partials, dlogits) of one head."""
    x = R.f32(x)
    N, C = x.shape
    valid = tgt != R.IGN
    mx = x.max(1)
    e = _exp32(x - mx[:, None])
    se = _lane_sum32(e)
    g = np.where(valid, tgt, 0)
    row = (_log32(se) + mx) - x[np.arange(N), g]
    assert row.dtype == np.float32
    red = np.zeros(16, np.float32)
    for n in range(N):
        if valid[n]:
            red[n % 16] = red[n % 16] + row[n]
    s = red[0]
    for w in range(1, 16):
        s = s + red[w]
    nv = np.float32(valid.sum())
    scale = np.float32(gscale) / nv if lwscale is None else (np.float32(gscale) * np.float32(lwscale)) / nv
    onehot = np.zeros((N, C), np.float32)
    onehot[np.arange(N), g] = 1
    d = scale * (e / se[:, None] - onehot)
    d[~valid] = 0
    assert d.dtype == np.float32 and s.dtype == np.float32
    return row, valid, s, nv, d


def _restate(case):
    """Checks the float32 restatement of one case at 1x; returns its worst (row loss, dlogits) ratios."""
    worst = {"loss": 0.0, "dlogits": 0.0}
    o = R.loss_case(case)
    fw = R.loss_fwd(o["l1"], o["l2"], o["t1"], o["t2"], case["lw"])
    bw = R.loss_bwd(o["l1"], o["l2"], o["t1"], o["t2"], case["lw"], case["gscale"])
    sums = []
    for h in (1, 2):
        x, t = o["l%d" % h], o["t%d" % h]
        row, valid, s, nv, d = _loss32(x, t, None if h == 1 else case["lw"], case["gscale"])
        r = R.ce_rows(x, t)
        w = R.check("row loss %d [%s]" % (h, case["id"]), row[valid], r["row"][valid], r["b_row"][valid])
        worst["loss"] = max(worst["loss"], w)
        R.check("stats[%d] [%s]" % (3 * h - 3, case["id"]), s, fw["stats"][3 * h - 3], fw["b_stats"][3 * h - 3])
        w = R.check("dlogits%d [%s]" % (h, case["id"]), d, bw["d%d" % h], bw["b_d%d" % h])
        worst["dlogits"] = max(worst["dlogits"], w)
        sums.append((s, nv))
    loss = sums[0][0] / sums[0][1] + np.float32(case["lw"]) * (sums[1][0] / sums[1][1])
    assert loss.dtype == np.float32
    R.check("loss [%s]" % case["id"], loss, fw["loss"], fw["b_loss"])
    return worst


@pytest.mark.parametrize("case", R.LOSS_CASES, ids=ids(R.LOSS_CASES))
def test_float32_restatement_stays_within_the_bounds(case):
    _restate(case)


def test_float32_restatement_bounds_are_not_vacuous():
    """Over the whole table the float32 restatement comes within a factor of a few of the bounds: they are not slack by
    orders of magnitude."""
    worst = [_restate(c) for c in R.LOSS_CASES]
    loss, dl = max(w["loss"] for w in worst), max(w["dlogits"] for w in worst)
    print("float32 restatement: worst row loss / bound %.3f, worst dlogits / bound %.3f" % (loss, dl))
    assert 0.05 <= loss <= 1.0 and 0.05 <= dl <= 1.0


# --------------------------------------------------------------------------- planted mistakes
def flagged(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


def _head(case, real=False):
    o = R.real_head_case(case) if real else R.exact_head_case(case)
    fw = R.head_fwd(o["enc"], o["w1"], o["b1"], o["w2"], o["b2"], case["li"])
    o["pooled"] = R.f32(fw["pooled"])
    return o, fw


def _bwd(o, li, fn=R.head_bwd, **kw):
    a = {k: kw.pop(k, o[k]) for k in ("enc", "pooled", "d1", "d2", "w1", "w2")}
    return fn(a["enc"], a["pooled"], a["d1"], a["d2"], a["w1"], a["w2"], li, **kw)


def _both(case_exact, case_real, name, wrong_of):
    """The mistake is flagged by exact() on the integer case and by check() at the GPU module's 2x on the real one; the
    unmistaken float32 result passes both."""
    for case, real in ((case_exact, False), (case_real, True)):
        o, fw = _head(case, real)
        ref, wrong = wrong_of(case, o, fw)
        bound = {**R.head_fwd_bounds(o["enc"], o["w1"], o["b1"], o["w2"], o["b2"], case["li"]), **_bwd(o, case["li"], R.head_bwd_bounds)}
        for k in name:
            if real:
                R.check(k, R.f32(ref[k]), ref[k], bound[k], 2.0)
                flagged(R.check, k, R.f32(wrong[k]), ref[k], bound[k], 2.0)
            else:
                R.exact(k, R.f32(ref[k]), ref[k])
                flagged(R.exact, k, R.f32(wrong[k]), ref[k])


def test_planted_clip_256_missing_from_dw1_db1():
    def wrong_of(case, o, fw):
        d1 = o["d1"].copy()
        d1[256] = 0
        return _bwd(o, case["li"]), _bwd(o, case["li"], d1=d1)
    _both(by_edge(R.HEAD_EXACT, "N257-C1_9-C2_2-T2-li1-dw1-second-256-clip-chunk"), by_edge(R.HEAD_REAL, "second-class-chunk"),
          ("dW1", "db1"), wrong_of)


def test_planted_class_512_missing_from_d_enc():
    def wrong_of(case, o, fw):
        d1 = o["d1"].copy()
        d1[:, 512] = 0
        return _bwd(o, case["li"]), _bwd(o, case["li"], d1=d1)
    _both(by_edge(R.HEAD_EXACT, "second-chunk-one-class-empty-quarters"), by_edge(R.HEAD_REAL, "second-class-chunk"), ("d_enc",), wrong_of)


def test_planted_class_8_missing_from_logits1():
    def wrong_of(case, o, fw):
        l1 = fw["logits1"].copy()
        l1[:, 8] = np.nan                        # the pre-fill an unwritten class keeps
        return fw, {"logits1": l1}
    small = by_edge(R.HEAD_REAL, "N5-C1_9-C2_3-T3-li1-small")
    _both(by_edge(R.HEAD_EXACT, "rc-group-plus-one"), small, ("logits1",), wrong_of)

    def wrong_term(case, o, fw):                 # written, but without its share of the sum: the bias alone
        l1 = fw["logits1"].copy()
        l1[:, 8] = o["b1"][8]
        return fw, {"logits1": l1}
    _both(by_edge(R.HEAD_EXACT, "rc-group-plus-one"), small, ("logits1",), wrong_term)


def test_planted_last_frame_instead_of_lang_index():
    def wrong_of(case, o, fw):
        T = case["T"]
        ref = {**fw, **_bwd(o, case["li"])}
        wrong = {**R.head_fwd(o["enc"], o["w1"], o["b1"], o["w2"], o["b2"], T - 1), **_bwd(o, T - 1)}
        return ref, wrong
    _both(by_edge(R.HEAD_EXACT, "middle-frame"), by_edge(R.HEAD_REAL, "N5-C1_9-C2_3-T3-li1-small"), ("logits2", "dW2", "d_enc"), wrong_of)


def test_planted_d_enc_accumulated_instead_of_written():
    def wrong_of(case, o, fw):
        ref = _bwd(o, case["li"], accumulate=1, preset=o["preset"])
        return ref, {"d_enc": ref["d_enc"] + R.f64(o["preset"]["d_enc"])}
    _both(by_edge(R.HEAD_EXACT, "rc-group-plus-one"), by_edge(R.HEAD_REAL, "N5-C1_9-C2_3-T3-li1-small"), ("d_enc",), wrong_of)


def _loss(case_id, **kw):
    c = dict(R.LOSS_BY_ID[case_id])
    o = R.loss_case(c)
    c.update(kw)
    return o, R.loss_fwd(o["l1"], o["l2"], o["t1"], o["t2"], c["lw"]), R.loss_bwd(o["l1"], o["l2"], o["t1"], o["t2"], c["lw"], c["gscale"])


def _loss_flagged(ref, wrong, keys):
    fw, bw = ref
    wfw, wbw = wrong
    for k in keys:
        if k == "loss":
            R.check(k, np.float32(fw["loss"]), fw["loss"], fw["b_loss"], 2.0)
            flagged(R.check, k, np.float32(wfw["loss"]), fw["loss"], fw["b_loss"], 2.0)
        else:
            R.check(k, R.f32(bw[k]), bw[k], bw["b_" + k], 2.0)
            flagged(R.check, k, R.f32(wbw[k]), bw[k], bw["b_" + k], 2.0)


def test_planted_gscale_ignored():
    cid = "N5-C65x64-spread3-g0.37-lw0.1-gscale-fraction"
    _, fw, bw = _loss(cid)
    _, wfw, wbw = _loss(cid, gscale=1.0)
    _loss_flagged((fw, bw), (wfw, wbw), ("d1", "d2"))


def test_planted_row_count_instead_of_valid_count():
    cid = "N5-C65x64-spread3-g1-lw0.1-ign-loss-bwd-fifth-row"
    o, fw, bw = _loss(cid)
    wrong = dict(bw)
    for h in (1, 2):
        wrong["d%d" % h] = bw["d%d" % h] * float((o["t%d" % h] != R.IGN).sum()) / 5
    _loss_flagged((fw, bw), (fw, wrong), ("d1", "d2"))
    wfw = dict(fw)
    wfw["loss"] = fw["stats"][0] / 5 + float(np.float32(0.1)) * fw["stats"][3] / 5
    _loss_flagged((fw, bw), (wfw, bw), ("loss",))


def test_planted_lang_weight_fixed():
    cid = "N17-C1500x2-spread3-g0.37-lw1.5-ign-lang-weight-other"
    _, fw, bw = _loss(cid)
    _, wfw, wbw = _loss(cid, lw=0.1)
    _loss_flagged((fw, bw), (wfw, wbw), ("loss", "d2"))
    R.check("d1", R.f32(wbw["d1"]), bw["d1"], bw["b_d1"], 2.0)       # head 1 does not see lang_weight


@pytest.mark.parametrize("C1,C2", [(1500, 65), (65, 1500)])
def test_planted_ties_to_the_highest_index(C1, C2):
    for target in ("lower", "higher"):
        o = R.tie_case(C1, C2, target)
        fw = R.loss_fwd(o["l1"], o["l2"], o["t1"], o["t2"], 0.1)
        n = len(o["t1"])
        counts = R.f32(fw["stats"][[1, 2, 4, 5]])
        assert counts.tolist() == ([n, n, n, n] if target == "lower" else [n, 0, n, 0])
        wrong = []
        for h in (1, 2):
            x, t = o["l%d" % h], o["t%d" % h]
            last = x.shape[1] - 1 - x[:, ::-1].argmax(1)
            assert (last != x.argmax(1)).all() and (x.max(1) == x[np.arange(n), last]).all()
            wrong += [n, int((last == t).sum())]
        R.exact("counts", counts, fw["stats"][[1, 2, 4, 5]])
        flagged(R.exact, "counts", R.f32(wrong), fw["stats"][[1, 2, 4, 5]])
    assert {(5, 69), (64, 1)} <= set(R.TIE_PAIRS[1500]) and (64, 1) in R.TIE_PAIRS[65]
    assert 5 % 64 == 69 % 64 and 64 % 64 < 1 % 64            # one lane in two passes; the lower index in the higher lane
