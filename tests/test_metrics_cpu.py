"""Validation scoring (WER / PER of greedy decodes) without a GPU: ops.seq_score on CPU tensors, the meter built on it
and the public surface, against the plain-Python restatement of SBL/train.py:252-254 / :40-42 in metrics_cases.py.
Every comparison is exact: integers, or fp64 means formed from the same integers."""
import inspect
import os
import re
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import metrics_cases as MC
from conftest import load_golden
from sbl_for_multilingual_lip_reading_amd import _lib, detfill, ops
from sbl_for_multilingual_lip_reading_amd.transformer.metrics import ErrorRateMeter, wer_per

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = (MC.SOS, MC.EOS, MC.IGN)


def _score(ys_l, ys_r, gold_l, gold_r, names=None, valid_rows=None):
    """(per_sample (2, 3, N), acc (2, 37)) of one ops.seq_score call on CPU tensors."""
    t = [torch.from_numpy(np.ascontiguousarray(a)) for a in (ys_l, ys_r, gold_l, gold_r)]
    acc = torch.zeros(2, ops.SCORE_COUNTERS, dtype=torch.int64)
    per = torch.full((2, 3, t[0].size(0)), -7, dtype=torch.int32)
    tab = None if names is None else ops.pack_names(names)
    vr = None if valid_rows is None else torch.tensor([valid_rows], dtype=torch.int32)
    ops.seq_score(*t, acc, *IDS, names=tab, valid_rows=vr, per_sample=per)
    return per, acc


def _check_result(res, tag, want):
    assert res[tag + "_wer"] == want["wer"] and res[tag + "_per"] == want["per"] and res[tag + "_per_corpus"] == want["per_corpus"]
    assert res["n" if tag == "l2r" else "r2l_n"] == want["n"]
    assert res["n_empty" if tag == "l2r" else "r2l_n_empty"] == want["n_empty"]


def test_seq_score_matches_restatement_per_sample():
    ys, gold = MC.generate()
    M = len(ys)
    assert M >= 2000
    plain = [MC.restate(y, g) for y, g in zip(ys, gold)]
    named = [MC.restate(y, g, MC.NAMES) for y, g in zip(ys, gold)]
    # the classes the generator builds explicitly are really there
    kept = lambda row: [int(t) for t in row if t not in MC.SPECIAL]      # noqa: E731
    cs = [s[1] for s in plain]
    assert 0 in cs and 15 in cs
    assert any(s[0] == 0 and s[1] > 0 for s in plain)                                           # exact match
    assert any(any(y[i] == MC.EOS and y[i + 1] not in MC.SPECIAL for i in range(1, c)) for y, c in zip(ys, cs))     # eos mid-window
    assert any(len(kept(y[c + 1:])) > 0 and c > 0 for y, c in zip(ys, cs))                      # longer than the window
    assert any(all(t == MC.EOS for t in y[1:]) and c > 0 for y, c in zip(ys, cs))               # all-eos prediction
    twins = [i for i in range(M) if plain[i][0] > 0 and plain[i][2] == 1 and named[i][2] == 0]
    assert twins, "no pair that differs in ids and agrees in spelling"
    # r2l direction: the same pairs in another order, so that the two directions of a call differ
    perm = np.random.RandomState(3).permutation(M)
    for names, want in ((None, plain), (MC.NAMES, named)):
        per, acc = _score(ys, ys[perm], gold, gold[perm], names)
        assert per[0].t().tolist() == [list(s) for s in want]
        assert per[1].t().tolist() == [list(want[i]) for i in perm]
        assert acc[0].tolist() == MC.counters(want) == acc[1].tolist()
    # the fp64 read-out is the reference's mean of dist / c up to the rounding of a float sum
    e = MC.expect(plain)
    assert abs(e["per"] - np.mean([d / c for d, c, _ in plain if c > 0])) < 1e-12
    # one-shot form, the reference's 4-tuple order
    t = [torch.from_numpy(a) for a in (ys, ys[perm], gold, gold[perm])]
    en = MC.expect(named)
    assert wer_per(*t, names=MC.NAMES) == (en["wer"], en["per"], en["wer"], en["per"])
    assert wer_per(*t)[0] == e["wer"] > en["wer"]


def test_committed_greedy_fixtures():
    for tag in ("small", "full", "varied"):
        g = load_golden("recognize_%s.npz" % tag)
        _, l2r, r2l = detfill.synthetic_batch(int(g["B"]), int(g["T"]), int(g["H"]), int(g["W"]), int(g["salt"]))
        meter = ErrorRateMeter(device="cpu")
        meter.update(*[torch.from_numpy(np.ascontiguousarray(a)) for a in (g["ys_l2r"], g["ys_r2l"], l2r, r2l)])
        res = meter.result()
        for d, (ys, gold) in (("l2r", (g["ys_l2r"], l2r)), ("r2l", (g["ys_r2l"], r2l))):
            want = MC.expect([MC.restate(y, t) for y, t in zip(ys, gold)])
            assert want["n"] == int(g["B"]) and want["n_empty"] == 0
            _check_result(res, d, want)


def test_meter_accumulates_masks_and_resets():
    ys, gold = MC.generate(300, seed=5)
    ys_r, gold_r = ys[::-1].copy(), gold[::-1].copy()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731
    meter = ErrorRateMeter(MC.NAMES, device="cpu")
    cuts = [0, 7, 107, len(ys)]                               # three updates of different N
    for a, b in zip(cuts, cuts[1:]):
        meter.update(T(ys[a:b]), T(ys_r[a:b]), T(gold[a:b]), T(gold_r[a:b]))
    res = meter.result()
    _check_result(res, "l2r", MC.expect([MC.restate(y, g, MC.NAMES) for y, g in zip(ys, gold)]))
    _check_result(res, "r2l", MC.expect([MC.restate(y, g, MC.NAMES) for y, g in zip(ys_r, gold_r)]))
    assert res["n"] + res["n_empty"] == len(ys)
    meter.reset()
    assert int(meter.acc.abs().sum()) == 0
    # valid_rows masks the tail (and is clamped to the batch)
    for k in (0, 1, 40, 311, 5000):
        meter.reset()
        meter.update(T(ys), T(ys_r), T(gold), T(gold_r), valid_rows=torch.tensor([k], dtype=torch.int32))
        kk = min(k, len(ys))
        assert meter.acc[0].tolist() == MC.counters([MC.restate(y, g, MC.NAMES) for y, g in zip(ys[:kk], gold[:kk])])
        assert meter.acc[1].tolist() == MC.counters([MC.restate(y, g, MC.NAMES) for y, g in zip(ys_r[:kk], gold_r[:kk])])
    per, _ = _score(ys, ys_r, gold, gold_r, valid_rows=40)
    assert per[:, :, 40:].eq(-1).all() and per[:, :, :40].ge(0).all()
    meter.reset()
    assert all(v != v for k, v in meter.result().items() if k[4:7] in ("wer", "per"))      # nothing scored: nan, not an error


def _gloo_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ys, gold = MC.generate(200, seed=9)
    mine = slice(0, 77) if rank == 0 else slice(77, None)      # uneven shards
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))    # noqa: E731
    meter = ErrorRateMeter(MC.NAMES, device="cpu")
    meter.update(T(ys[mine]), T(ys[mine][::-1]), T(gold[mine]), T(gold[mine][::-1]))
    meter.all_reduce()
    q.put((rank, meter.result(), meter.acc.tolist()))
    dist.destroy_process_group()


def test_all_reduce_gloo_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, 29631, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=300) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    ys, gold = MC.generate(200, seed=9)
    samples = [MC.restate(y, g, MC.NAMES) for y, g in zip(ys, gold)]
    for rank, res, acc in got:
        assert acc[0] == MC.counters(samples) == acc[1]      # the r2l shards hold the same samples in another order
        _check_result(res, "l2r", MC.expect(samples))
        _check_result(res, "r2l", MC.expect(samples))
    assert got[0][1] == got[1][1]


def test_surface():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbl_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+sbl_seq_score\s*\(", src)
    assert "sbl_seq_score" in _lib.SIGNATURES
    from sbl_for_multilingual_lip_reading_amd.transformer.transformer import Transformer
    params = list(inspect.signature(Transformer.validate).parameters.values())
    assert [p.name for p in params[:5]] == ["self", "padded_input", "padded_target_l2r", "padded_target_r2l", "meter"]
    assert all(p.default is not inspect.Parameter.empty for p in params[5:])      # only optional arguments behind them
    assert ops.SCORE_COUNTERS == int(re.search(r"#define\s+SBL_SCORE_COUNTERS\s+(\d+)", src).group(1))


def test_bad_arguments_are_refused():
    import pytest
    ys, gold = MC.generate(4, seed=1)
    t = [torch.from_numpy(a) for a in (ys, ys, gold, gold)]
    acc = torch.zeros(2, ops.SCORE_COUNTERS, dtype=torch.int64)
    with pytest.raises(ValueError, match="7 bytes"):
        ops.pack_names(["a", "toolongname"])
    with pytest.raises(ValueError, match="ASCII"):
        ops.pack_names(["é"])
    with pytest.raises(ValueError, match="To=16"):
        ops.seq_score(t[0], t[1], torch.zeros(len(ys), 16, dtype=torch.int64), torch.zeros(len(ys), 16, dtype=torch.int64), acc, *IDS)
    with pytest.raises(ValueError, match="int64"):
        ops.seq_score(t[0].int(), t[1], t[2], t[3], acc, *IDS)
    # the host-side checks of the C entry point run before any launch (safe without a GPU)
    with pytest.raises(_lib.SblHipError, match="To=16"):
        _lib.call("sbl_seq_score", None, None, 17, None, None, 16, 4, 0, 1, -1, None, 0, None, None, 1, None)
    with pytest.raises(_lib.SblHipError, match="null accumulator"):
        _lib.call("sbl_seq_score", None, None, 17, None, None, 14, 4, 0, 1, -1, None, 0, None, None, None, None)
    _lib.call("sbl_seq_score", None, None, 17, None, None, 14, 0, 0, 1, -1, None, 0, None, None, 1, None)      # N = 0: no-op
