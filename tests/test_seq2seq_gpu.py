"""GPU checks of the single-direction seq2seq model against the reference's fixtures (tests/golden/s2s_*.npz) and the
plain-torch restatement (tests/seq2seq_oracle.py): teacher-forced pass and gradients, padded targets, encoder padding, the
KV-cached greedy decode (eager, under hipGraph replay, against the prefix-recompute path), the decode-step kernels alone,
device scoring, and the flat-model / optimizer / gradient-exchange plumbing with the tied weight."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, maxdiff
import seq2seq_oracle as S
from test_seq2seq_cpu import CASES, build_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=["f32", "bf16x6"])
def precision(request):
    from sbl_for_multilingual_lip_reading_amd import ops
    ops.set_matmul_precision(request.param)
    yield request.param
    ops.set_matmul_precision("f32")


def gpu_model(g, train):
    m = build_model(g)
    sd = S.case_state(g)
    m.load_state_dict({k: sd.get(k, v) for k, v in m.state_dict().items()})
    m.lipreading.frontend_dropout_p = 0.0
    m.to("cuda:0")
    return m.train() if train else m.eval()


@pytest.mark.parametrize("case", CASES)
def test_forward_loss_and_gradients_match_reference(case, precision):
    """Tolerances of tests/test_hip_parity.py's SBL end-to-end cases: logits and loss 1e-3, gradients 2e-3 of the reference's
    largest entry (3e-2 for the frontend) + 2e-6.  Most of gold is IGNORE_ID in row 0 (target length 1)."""
    from sbl_for_multilingual_lip_reading_amd.transformer.loss import cal_performance
    g = load_golden(case + ".npz")
    m = gpu_model(g, train=True)
    x, tgt = S.case_inputs(g)
    pred, gold = m(x.cuda(), tgt.cuda())
    loss, n_correct = cal_performance(pred, gold, smoothing=0.1)
    loss.backward()
    torch.cuda.synchronize()
    d = maxdiff(pred, g["pred"])
    print("s2s[%s/%s] max|dlogit| %.2e loss %.6f ref %.6f" % (case, precision, d, loss.item(), float(g["loss"])))
    assert np.array_equal(gold.cpu().numpy(), g["gold"])
    assert d < 1e-3 and abs(loss.item() - float(g["loss"])) < 1e-3 and n_correct == int(g["n_correct"])
    named = dict(m.named_parameters())
    for k in g.files:
        if k.startswith("grad:"):
            name = k[5:] if k[5:] in named else "decoder.tgt_word_emb.weight"
            ref = g[k]
            tol = 3e-2 if "lipreading" in k else 2e-3
            assert maxdiff(S.sub(named[name].grad.cpu()), ref) < tol * float(np.abs(ref).max()) + 2e-6, k


def test_mostly_ignored_gold_matches_oracle():
    """Every target has length 1: 12 of 14 gold entries per row are IGNORE_ID; mean and n_correct over the 2 that are not."""
    from oracle import sbl_oracle as O
    from sbl_for_multilingual_lip_reading_amd.transformer.loss import cal_performance
    g = load_golden("s2s_small.npz")
    c = S.case_config(g)
    m = gpu_model(g, train=True)
    x, tgt = S.case_inputs(g)
    tgt = tgt.clone()
    tgt[:, 1:] = -1
    pred, gold = m(x.cuda(), tgt.cuda())
    loss, n_correct = cal_performance(pred, gold, smoothing=0.1)
    sd = S.case_state(g)
    with torch.no_grad():
        rpred, rgold = S.decoder_forward(sd, tgt, S.encode(sd, x, c["ne"], training=True), c["nd"], c["scale"])
        rloss, rn = O.cal_performance(rpred, rgold, 0.1)
    assert int((rgold != -1).sum()) == 2 * c["B"] and torch.equal(gold.cpu(), rgold)
    assert maxdiff(pred, rpred) < 1e-3 and abs(loss.item() - rloss.item()) < 1e-3 and n_correct == int(rn)


def test_encoder_padding_matches_oracle(precision):
    g = load_golden("s2s_varied.npz")
    c = S.case_config(g)
    m = gpu_model(g, train=True)
    _, tgt = S.case_inputs(g)
    enc = torch.from_numpy(np.asarray(S.detfill.normal("enc", (c["B"], c["T"], 512), 11)))
    lengths = [c["T"], 3, 1, c["T"] - 1]
    pred, gold = m.decoder(tgt.cuda(), enc.cuda(), lengths)
    sd = S.case_state(g)
    with torch.no_grad():
        rpred, rgold = S.decoder_forward(sd, tgt, enc, c["nd"], c["scale"], enc_lengths=lengths)
    assert torch.equal(gold.cpu(), rgold) and maxdiff(pred, rpred) < 1e-3


@pytest.mark.parametrize("case", CASES)
def test_recognize_tokens_exact(case, precision):
    """Cached and prefix-recompute greedy decodes both equal the reference's tokens exactly, no row excluded (the
    generator guarantees top-2 margins >= 1e-2)."""
    g = load_golden(case + ".npz")
    m = gpu_model(g, train=False)
    x, _ = S.case_inputs(g)
    with torch.no_grad():
        ys_c = m.recognize(x.cuda())
        ys_r = m.recognize(x.cuda(), cached=False)
    assert ys_c.dtype == torch.int64 and tuple(ys_c.shape) == g["tokens"].shape
    assert np.array_equal(ys_c.cpu().numpy(), g["tokens"]), "cached"
    assert np.array_equal(ys_r.cpu().numpy(), g["tokens"]), "recompute"


def _ref_scores(ys, gold, sos=0, eos=1):
    """LRW/train.py:247-249 on the host: (distance, target length) per row."""
    out = []
    for y, t in zip(ys.tolist(), gold.tolist()):
        gl = [v for v in t if v not in (sos, eos, -1)]
        pl = [v for v in y[:len(gl) + 1] if v not in (sos, eos, -1)]
        D = list(range(len(gl) + 1))
        for a in pl:
            prev, D[0] = D[0], D[0] + 1
            for j, b in enumerate(gl, 1):
                prev, D[j] = D[j], min(D[j] + 1, D[j - 1] + 1, prev + (a != b))
        out.append((D[-1], len(gl)))
    return out


def test_graph_replay_and_validate():
    """recognize + scoring captured as ONE hipGraph: two replays with different clips equal the eager cached decode, and the
    meter's counters equal the host scoring of the same tokens (eager and replayed)."""
    from sbl_for_multilingual_lip_reading_amd.transformer.metrics import ErrorRateMeter
    g = load_golden("s2s_varied.npz")
    m = gpu_model(g, train=False)
    x, tgt = S.case_inputs(g)
    clips = [x.cuda(), x.flip(0).cuda()]       # the fixture's rows decode to different tokens, so the two clips do too
    tgt = tgt.cuda()
    eager, meter_e = [], ErrorRateMeter(device="cuda:0")
    with torch.no_grad():
        for c in clips:
            eager.append(m.validate(c, tgt, meter_e).clone())
        torch.cuda.synchronize()
        meter_g = ErrorRateMeter(device="cuda:0")
        static = clips[0].clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m.validate(static, tgt, meter_g)       # warm-up on the capture stream
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ys_static = m.validate(static, tgt, meter_g)
        meter_g.reset()
        for c, ref in zip(clips, eager):
            static.copy_(c)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(ys_static, ref)
    assert np.array_equal(eager[0].cpu().numpy(), g["tokens"]) and np.array_equal(eager[1].cpu().numpy(), g["tokens"][::-1])
    assert not torch.equal(eager[0], eager[1])
    assert torch.equal(meter_g.acc, meter_e.acc)
    scores = [s_ for ys in eager for s_ in _ref_scores(ys.cpu(), tgt.cpu())]
    r = meter_e.result()
    scored = [(d, c) for d, c in scores if c > 0]
    assert r["n"] == len(scored) and r["n_empty"] == len(scores) - len(scored)
    assert abs(r["per"] - sum(d / c for d, c in scored) / len(scored)) < 1e-12
    assert abs(r["wer"] - sum(d != 0 for d, c in scored) / len(scored)) < 1e-12
    assert abs(r["per_corpus"] - sum(d for d, _ in scored) / sum(c for _, c in scored)) < 1e-12


@pytest.mark.parametrize("Lcap", [32, 64])
@pytest.mark.parametrize("step", [0, 1, 13, 28])
def test_decode_attn_step_kernel(step, Lcap):
    """The cached step against float64 attention over the first step+1 cache rows, to the bound of the attention unit test
    (tests/test_hip_parity.py: 5e-6); the new row is written at `step`, rows beyond it and rows before it are untouched."""
    from sbl_for_multilingual_lip_reading_amd import ops
    B, H = 5, 8
    gen = torch.Generator().manual_seed(100 * Lcap + step)
    q, kn, vn = (torch.randn(B, H * 64, generator=gen) for _ in range(3))
    kc, vc = (torch.randn(B, Lcap, H * 64, generator=gen) for _ in range(2))
    qkv = torch.cat([q, kn, vn], 1).cuda()                      # column slices of one buffer, as the decoder passes them
    kd, vd = kc.cuda(), vc.cuda()
    out = torch.empty(B, H * 64, device="cuda")
    ops.decode_attn_step(qkv[:, :512], qkv[:, 512:1024], qkv[:, 1024:], kd, vd, Lcap, out, H, step, True)
    torch.cuda.synchronize()
    kr, vr = kc.clone(), vc.clone()
    kr[:, step], vr[:, step] = kn, vn
    assert torch.equal(kd.cpu(), kr) and torch.equal(vd.cpu(), vr)

    def ref(q_, k_, v_):
        qh = q_.double().view(B, H, 1, 64)
        kh = k_.double().view(B, -1, H, 64).transpose(1, 2)
        vh = v_.double().view(B, -1, H, 64).transpose(1, 2)
        p = torch.softmax(qh @ kh.transpose(2, 3) / 8.0, -1)
        return (p @ vh).transpose(1, 2).reshape(B, H * 64)

    assert maxdiff(out, ref(q, kr[:, :step + 1], vr[:, :step + 1])) < 5e-6
    # "no append": the same kernel over a strided K / V block of 29 rows (the hoisted cross-attention layout)
    n = 29
    kv = torch.randn(B, n, 2 * H * 64, generator=gen)
    kvd = kv.cuda()
    ops.decode_attn_step(qkv[:, :512], None, None, kvd[:, :, :512], kvd[:, :, 512:], n, out, H, n, False)
    torch.cuda.synchronize()
    assert maxdiff(out, ref(q, kv[:, :, :512], kv[:, :, 512:])) < 5e-6 and torch.equal(kvd.cpu(), kv)


def test_decode_tail_kernel():
    """Projection, arg-max with the lowest index on ties, token append and the next input row, in one launch."""
    from sbl_for_multilingual_lip_reading_amd import ops
    from sbl_for_multilingual_lip_reading_amd.transformer.module import PositionalEncoding
    B, V = 7, 48
    gen = torch.Generator().manual_seed(5)
    y, w, emb = torch.randn(B, 512, generator=gen), torch.randn(V, 512, generator=gen), torch.randn(V, 512, generator=gen)
    w[9] = w[4]                      # an exact tie between classes 4 and 9 ...
    y[0] = w[4] * 10                 # ... that wins in row 0
    pe = PositionalEncoding(512, max_len=64).pe[0]
    ys = torch.zeros(B, 30, dtype=torch.long).cuda()
    logits, xn = torch.empty(B, V, device="cuda"), torch.empty(B, 512, device="cuda")
    ops.decode_tail(y.cuda(), w.cuda(), ys, 3, emb.cuda(), pe.cuda(), 0.25, x_next=xn, logits=logits)
    ref = y.double() @ w.double().t()
    tok = ref.argmax(-1)
    assert maxdiff(logits, ref) < 2e-6 * 512 ** 0.5 * 4 * float(ref.abs().max())
    assert int(ys[0, 4]) == 4 and torch.equal(ys[:, 4].cpu(), tok) and int(ys.sum()) == int(tok.sum())
    assert maxdiff(xn, emb[tok] * 0.25 + pe[4]) < 1e-6


def test_cached_decode_launch_sequences(monkeypatch):
    """The library calls of one recognize_beam and one beam_search(W = 2) on a 2-layer decoder, N = 2, T = 3, in order, as
    DESIGN.md section 4.4 lists them: the K/V block GEMM, the first-row embedding, then per step and layer QKV GEMM, step
    attention (append), fc GEMM, add + LayerNorm, Q GEMM, step attention over the hoisted K/V, fc GEMM, add + LayerNorm, the
    two FFN GEMMs, add + LayerNorm (11), then the tail; the beam search ends with its finish."""
    from sbl_for_multilingual_lip_reading_amd import _lib, ops
    from sbl_for_multilingual_lip_reading_amd.transformer.seq2seq import Seq2SeqDecoder
    n_layers, N, T = 2, 2, 3
    torch.manual_seed(11)
    dec = Seq2SeqDecoder(0, 1, 42, 512, n_layers, 8, 64, 64, 512, 2048, dropout=0.1).to("cuda:0").eval()
    enc = torch.randn(N, T, 512, device="cuda")
    names = []
    monkeypatch.setattr(ops, "call", lambda name, *a: names.append(name) or _lib.call(name, *a))

    def expected(attn, tail):
        gemm, ln = "sbl_gemm_f32", "sbl_add_layernorm_fwd"
        layer = [gemm, attn, gemm, ln, gemm, attn, gemm, ln, gemm, gemm, ln]
        return [gemm, "sbl_embed_scale_pe_fwd"] + T * (n_layers * layer + [tail])

    dec.recognize_beam(enc)
    assert names == expected("sbl_decode_attn_step", "sbl_decode_tail")
    del names[:]
    dec.beam_search(enc, 2)
    assert names == expected("sbl_beam_attn_step", "sbl_beam_tail") + ["sbl_beam_finish"]


def test_flat_model_adam_step_keeps_the_tie():
    """One FlatModel + FusedAdam step: the tied weight is updated once, from the sum of the embedding scatter-add and the
    projection's weight gradient, and both modules read the same storage afterwards."""
    from sbl_for_multilingual_lip_reading_amd import dp
    from sbl_for_multilingual_lip_reading_amd.transformer.loss import cal_performance_device
    from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import FusedAdam
    g = load_golden("s2s_small.npz")
    m = gpu_model(g, train=True)
    flat = dp.FlatModel(m)
    opt = FusedAdam(flat, lr=1e-3)
    x, tgt = S.case_inputs(g)
    w = m.decoder.tgt_word_emb.weight
    before = w.detach().clone()
    flat.zero_grad()
    pred, gold = m(x.cuda(), tgt.cuda())
    assert maxdiff(pred, g["pred"]) < 1e-3                      # the flat layout computes the same pass
    cal_performance_device(pred, gold, 0.1)[0].backward()
    torch.cuda.synchronize()
    ref = g["grad:decoder.tgt_word_emb.weight"]
    assert maxdiff(w.grad, ref) < 2e-3 * float(np.abs(ref).max()) + 2e-6
    assert w.grad.data_ptr() == w._sbl_grad.data_ptr()
    moved = (w.grad.abs() > 1e-6).clone()
    opt.step()
    torch.cuda.synchronize()
    assert m.decoder.tgt_word_prj.weight is m.decoder.tgt_word_emb.weight
    assert m.decoder.tgt_word_prj.weight.data_ptr() == w.data_ptr()
    delta = (w.detach() - before).abs()
    # Adam's first step moves every entry with a non-zero gradient by lr (once: a double update would move it further)
    assert bool(moved.any())
    assert float(delta.max()) <= 1e-3 * 1.001 and float(delta[moved].min()) >= 1e-3 * 0.9


_GLOO = r"""
import os, sys
import torch, torch.distributed as dist
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
rank = int(sys.argv[1])
dist.init_process_group("gloo", init_method="file://" + sys.argv[2], rank=rank, world_size=2)
from conftest import load_golden
import seq2seq_oracle as S
from test_seq2seq_gpu import gpu_model
from sbl_for_multilingual_lip_reading_amd import dp
from sbl_for_multilingual_lip_reading_amd.transformer.loss import cal_performance_device
g = load_golden("s2s_small.npz")
m = gpu_model(g, train=True)
flat = dp.FlatModel(m)
x, tgt = S.case_inputs(g)
if rank == 1:
    x = x.flip(0) * 0.5
def grads(exchange):
    flat.zero_grad()
    pred, gold = m(x.cuda(), tgt.cuda())
    cal_performance_device(pred, gold, 0.1)[0].backward()
    if exchange is not None:
        exchange.finish()
    torch.cuda.synchronize()
    return flat.flat_grad.detach().cpu().clone()
local = grads(None)
both = [torch.empty_like(local), torch.empty_like(local)]
dist.all_gather(both, local)
ex = dp.GradientExchange(flat, 2, overlap=True, average=True)
got = grads(ex)
want = 0.5 * (both[0] + both[1])
err = float((got - want).abs().max()) / float(want.abs().max())
segs = [s for s, _ in ex.launches]
assert segs[0] == "decoder." and "encoder." in segs and segs[-1] == "lipreading.", segs
assert err < 1e-4, err
print("ok", rank, err)
"""


def test_two_ranks_exchange_the_new_segments(tmp_path):
    """Two processes over gloo on one device: the exchanged flat gradient is the mean of the two ranks' local gradients,
    launched segment by segment in the order decoder -> encoder -> ResNet stages -> stem."""
    script = tmp_path / "rank.py"
    script.write_text(_GLOO.format(root=ROOT))
    rdv = str(tmp_path / "rdv")
    procs = [subprocess.Popen([sys.executable, str(script), str(r), rdv], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0 and "ok" in o, o[-3000:]
