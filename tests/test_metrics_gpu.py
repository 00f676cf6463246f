"""Validation scoring on the MI355X: the sbl_seq_score kernel against the CPU form of the same definition (which
tests/test_metrics_cpu.py pins to the plain-Python restatement), Transformer.validate against the committed greedy fixture,
and validate under hipGraph replay.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import metrics_cases as MC
from conftest import load_golden
from sbl_for_multilingual_lip_reading_amd import detfill

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IDS = (MC.SOS, MC.EOS, MC.IGN)


@pytest.fixture(autouse=True)
def _f32_after():
    from sbl_for_multilingual_lip_reading_amd import ops
    yield
    ops.set_matmul_precision("f32")


def _pairs(N):
    """The first N generated pairs for l2r (the explicit classes come first), the same pairs rotated for r2l."""
    ys, gold = MC.generate()
    ys, gold = ys[:N], gold[:N]
    k = N // 3
    return [torch.from_numpy(np.ascontiguousarray(a)) for a in (ys, np.roll(ys, k, 0), gold, np.roll(gold, k, 0))]


def _run(ops, toks, dev, names, valid, acc=None):
    t = [a.to(dev) for a in toks]
    N = t[0].size(0)
    acc = torch.zeros(2, ops.SCORE_COUNTERS, dtype=torch.int64, device=dev) if acc is None else acc
    per = torch.full((2, 3, N), -7, dtype=torch.int32, device=dev)
    tab = None if names is None else ops.pack_names(names).to(dev)
    vr = None if valid is None else torch.tensor([valid], dtype=torch.int32, device=dev)
    ops.seq_score(*t, acc, *IDS, names=tab, valid_rows=vr, per_sample=per)
    return per.cpu(), acc.cpu()


@pytest.mark.parametrize("N", [1, 3, 32, 100, 257, 2059])
@pytest.mark.parametrize("named", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_kernel_equals_cpu_form(N, named, masked):
    from sbl_for_multilingual_lip_reading_amd import ops
    toks = _pairs(N)
    assert toks[0].size(0) == N
    names = MC.NAMES if named else None
    valid = N // 2 if masked else None
    per_c, acc_c = _run(ops, toks, "cpu", names, valid)
    per_g, acc_g = _run(ops, toks, DEV, names, valid)
    assert torch.equal(per_g, per_c)
    assert torch.equal(acc_g, acc_c)
    assert int(acc_c[:, :2].sum()) == 2 * (N if valid is None else valid)      # every live row is scored or empty


def test_repeatable_and_precision_independent():
    from sbl_for_multilingual_lip_reading_amd import ops
    toks = _pairs(257)
    accs = []
    for mode in ("f32", "f32", "bf16x6"):
        ops.set_matmul_precision(mode)
        accs.append(_run(ops, toks, DEV, MC.NAMES, None)[1])
    assert torch.equal(accs[0], accs[1]) and torch.equal(accs[0], accs[2])
    # the call ADDS: a second launch on the same accumulator doubles it
    acc = torch.zeros(2, ops.SCORE_COUNTERS, dtype=torch.int64, device=DEV)
    _run(ops, toks, DEV, MC.NAMES, None, acc)
    _run(ops, toks, DEV, MC.NAMES, None, acc)
    assert torch.equal(acc.cpu(), 2 * accs[0])


def _model(n_enc, n_dec, gains):
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    from sbl_for_multilingual_lip_reading_amd.transformer.transformer import Transformer
    m = Transformer(Encoder(512, n_enc, 8, 64, 64, 512, 2048), Decoder(0, 1, 58, 512, n_dec, 8, 64, 64, 512, 2048), None)
    m.load_state_dict({k: (v if k.endswith("pe") else torch.from_numpy(detfill.fill_value(k, tuple(v.shape), 0, gains).copy()))
                       for k, v in m.state_dict().items()})
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    m.visual_frontend.frontend_dropout_p = 0.0
    return m.to(DEV)


@pytest.mark.parametrize("mode", ["f32", "bf16x6"])
def test_validate_on_the_varied_fixture(mode):
    from sbl_for_multilingual_lip_reading_amd import ops
    from sbl_for_multilingual_lip_reading_amd.transformer.metrics import ErrorRateMeter
    ops.set_matmul_precision(mode)
    g = load_golden("recognize_varied.npz")
    m = _model(int(g["n_enc"]), int(g["n_dec"]), str(g["gains"]))
    m = m.train() if int(g["train_bn"]) else m.eval()
    x, l2r, r2l = detfill.synthetic_batch(int(g["B"]), int(g["T"]), int(g["H"]), int(g["W"]), int(g["salt"]))
    meter = ErrorRateMeter(device=DEV)
    with torch.no_grad():
        ys_l, ys_r = m.validate(torch.from_numpy(x).to(DEV), torch.from_numpy(l2r).to(DEV), torch.from_numpy(r2l).to(DEV), meter)
    assert np.array_equal(ys_l.cpu().numpy(), g["ys_l2r"]) and np.array_equal(ys_r.cpu().numpy(), g["ys_r2l"])
    res = meter.result()
    for tag, ys, gold in (("l2r", g["ys_l2r"], l2r), ("r2l", g["ys_r2l"], r2l)):
        want = MC.expect([MC.restate(y, t) for y, t in zip(ys, gold)])
        assert res[tag + "_wer"] == want["wer"] and res[tag + "_per"] == want["per"] and res[tag + "_per_corpus"] == want["per_corpus"]
    assert (res["n"], res["n_empty"], res["r2l_n"], res["r2l_n_empty"]) == (int(g["B"]), 0, int(g["B"]), 0)


def test_validate_under_graph_replay():
    """validate captured once, replayed three times: exactly three times the counters of one eager call, no host sync
    between the replays; then a fourth replay with valid_rows lowered on the device adds the first row only."""
    from sbl_for_multilingual_lip_reading_amd.transformer.metrics import ErrorRateMeter
    B, T, H, W = 4, 8, 24, 24
    m = _model(2, 2, "varied").eval()
    x, l2r, r2l = detfill.synthetic_batch(B, T, H, W, 41)
    x, l2r, r2l = (torch.from_numpy(a).to(DEV) for a in (x, l2r, r2l))
    vr = torch.tensor([B], dtype=torch.int32, device=DEV)
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    eager, eager1, meter = ErrorRateMeter(device=DEV), ErrorRateMeter(device=DEV), ErrorRateMeter(device=DEV)
    s = torch.cuda.Stream()
    with torch.no_grad():
        ys_e = m.validate(x, l2r, r2l, eager, valid_rows=vr)
        m.validate(x, l2r, r2l, eager1, valid_rows=one)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m.validate(x, l2r, r2l, meter, valid_rows=vr)      # warm-up on the capture stream
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ys_g = m.validate(x, l2r, r2l, meter, valid_rows=vr)
    meter.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            graph.replay()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    want = eager.acc.cpu()
    assert int(want[:, 0].sum()) == 2 * B and int(want[:, 3].sum()) > 0      # the eager call scored something
    assert torch.equal(meter.acc.cpu(), 3 * want)
    assert torch.equal(ys_g[0], ys_e[0]) and torch.equal(ys_g[1], ys_e[1])
    vr.copy_(one)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(meter.acc.cpu(), 3 * want + eager1.acc.cpu())
    assert int(eager1.acc[:, 0].sum()) == 2
