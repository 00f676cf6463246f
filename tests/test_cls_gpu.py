"""Stage-1 classification pre-training on the MI355X: the head kernels (sbl_cls_*) against fp64 torch on the CPU, the whole
ClassifierTransformer against the reference's fixture and a CPU-autograd training step, data parallel over two ranks,
save / resume, and the stage 1 -> 2 hand-off of the trained frontend."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from conftest import load_golden, maxdiff
from sbl_for_multilingual_lip_reading_amd import detfill

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGN = -100


@pytest.fixture(scope="module", params=["f32", "bf16x6"])
def ops(request):
    """Model-level tests run under both fp32-grade arithmetics of the tile engine (the heads themselves are plain fp32 FMA
    in every mode)."""
    from sbl_for_multilingual_lip_reading_amd import _lib, ops as _ops
    _lib.load()
    assert torch.cuda.is_available()
    _ops.set_matmul_precision(request.param)
    yield _ops
    _ops.set_matmul_precision("f32")


@pytest.fixture(autouse=True)
def _pin_precision(request):
    """Tests without the `ops` fixture run under the library default ("f32")."""
    if "ops" not in request.fixturenames:
        from sbl_for_multilingual_lip_reading_amd import ops as _ops
        prev = _ops.get_matmul_precision()
        _ops.set_matmul_precision("f32")
        yield
        _ops.set_matmul_precision(prev)
    else:
        yield


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# --------------------------------------------------------------------------- head kernels against fp64 torch
def _head_inputs(N, T, seed, tie2):
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(N, T, 512, generator=g)
    w1 = torch.randn(1500, 512, generator=g) * 0.05
    b1 = torch.randn(1500, generator=g) * 0.1
    w2 = torch.randn(2, 512, generator=g) * 0.05
    b2 = torch.randn(2, generator=g) * 0.1
    # tied maxima: word class 7 is a copy of class 3, and the even clips are pushed towards that pair so that it holds their
    # maximum (argmax must pick 3); with tie2 the two language classes are equal on every clip (argmax must pick 0)
    w1[7], b1[7] = w1[3], b1[3]
    enc[0::2] += 8.0 * w1[3] / w1[3].dot(w1[3])
    if tie2:
        w2[1], b2[1] = w2[0], b2[0]
    t1 = torch.randint(0, 1500, (N,), generator=g)
    t2 = torch.randint(0, 2, (N,), generator=g)
    t1[0::4] = 3
    t1[2::4] = 7
    t1[1::3] = IGN
    t2[2::4] = IGN
    return enc, w1, b1, w2, b2, t1, t2


def _head_ref(enc, w1, b1, w2, b2, t1, t2, li, lw=0.1):
    """fp64 torch on the CPU: logits, loss, stats and every gradient."""
    leaves = [t.double().requires_grad_(True) for t in (enc, w1, b1, w2, b2)]
    e, W1, B1, W2, B2 = leaves
    l1 = e.mean(1) @ W1.t() + B1
    l2 = e[:, li] @ W2.t() + B2
    loss = F.cross_entropy(l1, t1, ignore_index=IGN) + lw * F.cross_entropy(l2, t2, ignore_index=IGN)
    stats = []
    for l, t in ((l1, t1), (l2, t2)):
        v = t != IGN
        stats += [float(F.cross_entropy(l.detach(), t, ignore_index=IGN, reduction="sum")), float(v.sum()),
                  float(((l.argmax(1) == t) & v).sum())]
    if torch.isfinite(loss):
        loss.backward()
    return l1.detach(), l2.detach(), loss.detach(), torch.tensor(stats, dtype=torch.float64), [p.grad for p in leaves]


def _head_gpu(enc, w1, b1, w2, b2, t1, t2, li, lw=0.1):
    from sbl_for_multilingual_lip_reading_amd import ops
    leaves = [t.to(DEV).requires_grad_(True) for t in (enc, w1, b1, w2, b2)]
    l1, l2 = ops.ClsHeadFn.apply(*leaves, li)
    loss, stats = ops.ClsLossFn.apply(l1, l2, t1.to(DEV), t2.to(DEV), lw, IGN)
    if torch.isfinite(loss):
        loss.backward()
    torch.cuda.synchronize()
    return l1.detach(), l2.detach(), loss.detach(), stats, [p.grad for p in leaves]


CASES = [(N, T, li) for N in (1, 2, 32, 100) for T in (1, 30, 31) for li in sorted({0, T - 1})]


@pytest.mark.parametrize("N,T,li", CASES)
def test_head_kernels_match_fp64_torch(N, T, li):
    inp = _head_inputs(N, T, 1000 * N + 10 * T + li, tie2=(N >= 32))
    r = _head_ref(*inp, li)
    g = _head_gpu(*inp, li)
    assert relerr(g[0], r[0]) < 1e-5 and relerr(g[1], r[1]) < 1e-5
    assert abs(float(g[2]) - float(r[2])) <= 1e-5 * abs(float(r[2]))
    s, rs = g[3].cpu().double(), r[3]
    assert torch.equal(s[[1, 2, 4, 5]], rs[[1, 2, 4, 5]]), (s, rs)          # valid rows and correct counts: exact
    assert abs(s[0] - rs[0]) <= 1e-5 * abs(rs[0]) and abs(s[3] - rs[3]) <= 1e-5 * abs(rs[3]) + 1e-12
    for name, a, b in zip(("d_enc", "dW1", "db1", "dW2", "db2"), g[4], r[4]):
        # (with tied language classes db2 is analytically 0: the absolute floor covers it)
        assert maxdiff(a, b) <= 1e-5 * float(b.abs().max()) + 1e-12, (name, relerr(a, b))
    if N >= 32:                                   # the ties went to the lowest index
        assert int(s[5]) == int(((inp[6] == 0)).sum())
        boosted = torch.zeros(N, dtype=torch.bool)
        boosted[0::2] = True
        assert bool((g[0].cpu().argmax(1)[boosted] == 3).all())


def test_head_loss_with_every_row_ignored_is_nan_like_torch():
    enc, w1, b1, w2, b2, t1, t2 = _head_inputs(5, 31, 77, tie2=False)
    t1[:] = IGN
    r = _head_ref(enc, w1, b1, w2, b2, t1, t2, 30)
    g = _head_gpu(enc, w1, b1, w2, b2, t1, t2, 30)
    assert torch.isnan(r[2]) and torch.isnan(g[2].cpu())
    s = g[3].cpu()
    assert float(s[0]) == 0.0 and float(s[1]) == 0.0 and float(s[2]) == 0.0 and float(s[4]) == float(r[3][4])
    # the ignored head contributes exactly nothing to the gradients: only the language head's path is left
    from sbl_for_multilingual_lip_reading_amd import ops
    l1 = torch.randn(5, 1500, device=DEV)
    l2 = torch.randn(5, 2, device=DEV, requires_grad=True)
    l1.requires_grad_(True)
    loss, _ = ops.ClsLossFn.apply(l1, l2, t1.to(DEV), t2.to(DEV), 0.1, IGN)
    loss.backward(torch.ones((), device=DEV))
    assert float(l1.grad.abs().max()) == 0.0


def test_head_is_bitwise_repeatable_and_independent_of_matmul_precision():
    from sbl_for_multilingual_lip_reading_amd import ops
    inp = _head_inputs(100, 31, 5, tie2=False)
    runs = [_head_gpu(*inp, 30), _head_gpu(*inp, 30)]
    ops.set_matmul_precision("bf16x6")
    try:
        runs.append(_head_gpu(*inp, 30))
    finally:
        ops.set_matmul_precision("f32")
    flat = lambda r: [r[0], r[1], r[2], r[3]] + list(r[4])
    for other in runs[1:]:
        for a, b in zip(flat(runs[0]), flat(other)):
            assert torch.equal(a, b)


def test_head_backward_accumulates_and_skips_null_outputs():
    from sbl_for_multilingual_lip_reading_amd import ops
    from sbl_for_multilingual_lip_reading_amd.ops import _p, _s
    N, T, li = 32, 31, 30
    g = torch.Generator().manual_seed(9)
    enc = torch.randn(N, T, 512, generator=g).to(DEV)
    w1, b1 = (torch.randn(1500, 512, generator=g) * 0.05).to(DEV), torch.randn(1500, generator=g).to(DEV)
    w2, b2 = (torch.randn(2, 512, generator=g) * 0.05).to(DEV), torch.randn(2, generator=g).to(DEV)
    pooled, pooled_t = torch.empty(N, 512, device=DEV), torch.empty(512, N, device=DEV)
    l1, l2 = torch.empty(N, 1500, device=DEV), torch.empty(N, 2, device=DEV)
    ops.call("sbl_cls_head_fwd", _p(enc), _p(w1), _p(b1), _p(w2), _p(b2), _p(pooled), _p(pooled_t), _p(l1), _p(l2), N, T, 512,
             1500, 2, li, _s())
    d1, d2 = torch.randn(N, 1500, generator=g).to(DEV), torch.randn(N, 2, generator=g).to(DEV)
    shapes = ((1500, 512), (1500,), (2, 512), (2,))

    def bwd(d_enc, outs, acc):
        ops.call("sbl_cls_head_bwd", _p(enc), _p(pooled), _p(d1), _p(d2), _p(w1), _p(w2), _p(d_enc), *[_p(t) for t in outs], N,
                 T, 512, 1500, 2, li, acc, _s())
        torch.cuda.synchronize()

    fresh = [torch.full(s, float("nan"), device=DEV) for s in shapes]
    de = torch.full_like(enc, float("nan"))
    bwd(de, fresh, 0)
    prior = [torch.randn(s, generator=g).to(DEV) for s in shapes]
    acc = [t.clone() for t in prior]
    de2 = torch.full_like(enc, float("nan"))
    bwd(de2, acc, 1)
    for a, p, f in zip(acc, prior, fresh):
        assert torch.equal(a, p + f)                 # += of the same deterministic sums
    assert torch.equal(de2, de)                      # the input gradient is written, not accumulated
    # against fp64: the mean-over-time path on every frame, the language path on frame li only
    dp = (d1.double() @ w1.double()) / T
    ref = dp.unsqueeze(1).expand(N, T, 512).clone()
    ref[:, li] += d2.double() @ w2.double()
    assert relerr(de, ref) < 1e-5
    assert relerr(fresh[0], d1.double().t() @ pooled.double()) < 1e-5
    assert relerr(fresh[2], d2.double().t() @ enc[:, li].double()) < 1e-5
    # NULL outputs are skipped: the input gradient alone, then the language head's parameters alone
    de3 = torch.full_like(enc, float("nan"))
    bwd(de3, [None] * 4, 0)
    assert torch.equal(de3, de)
    only2 = [None, None, torch.zeros(2, 512, device=DEV), torch.zeros(2, device=DEV)]
    bwd(None, only2, 0)
    assert torch.equal(only2[2], fresh[2]) and torch.equal(only2[3], fresh[3])


# --------------------------------------------------------------------------- the whole model
def _fill(m):
    sd = m.state_dict()
    m.load_state_dict({k: (v if k.endswith(".pe") else torch.from_numpy(detfill.fill_value(k, tuple(v.shape)).copy()))
                       for k, v in sd.items()})
    for mm in m.modules():
        if isinstance(mm, torch.nn.Dropout):
            mm.p = 0.0
    m.visual_frontend.frontend_dropout_p = 0.0
    return m


def _cls_model(n_enc=1):
    from sbl_for_multilingual_lip_reading_amd.transformer.classifier import ClassifierTransformer
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    return _fill(ClassifierTransformer(Encoder(512, n_enc, 8, 64, 64, 512, 2048), None)).to(DEV).train()


def _targets(B, salt):
    g = torch.Generator().manual_seed(salt)
    return torch.randint(0, 1500, (B,), generator=g), torch.randint(0, 2, (B,), generator=g)


def _cls_step(m, salt, B=4, T=6, H=24, W=24):
    from sbl_for_multilingual_lip_reading_amd.transformer.classifier import cal_cls_loss
    x, _, _ = detfill.synthetic_batch(B, T, H, W, salt)
    t1, t2 = _targets(B, salt)
    v, lang = m(torch.from_numpy(x).to(DEV))
    loss, stats = cal_cls_loss(v, lang, t1.to(DEV), t2.to(DEV))
    loss.backward()
    return loss


def test_classifier_matches_cls_config1_golden(ops):
    """BASELINE config 1 through ClassifierTransformer itself (6 encoder layers, 2 clips of 29 frames + the zero frame the
    restated forward reads as its last row)."""
    g = load_golden("cls_config1.npz")
    m = _cls_model(6)
    seen = {}
    m.visual_frontend.register_forward_hook(lambda mod, i, o: seen.__setitem__("feats", o.detach()))
    m.encoder_v.register_forward_hook(lambda mod, i, o: seen.__setitem__("enc", o[0].detach()))
    x, _, _ = detfill.synthetic_batch(2, 29, 88, 88, int(g["salt"]))
    xt = torch.from_numpy(x)
    xt = torch.cat([xt, xt.new_zeros(2, 1, 88, 88)], 1).to(DEV)
    v, lang = m(xt)
    assert tuple(v.shape) == (2, 1500) and tuple(lang.shape) == (2, 2)
    assert maxdiff(seen["feats"], g["feats"]) < 1e-3 and maxdiff(seen["enc"], g["enc"]) < 1e-3
    assert maxdiff(v, g["v_t"]) < 1e-3 and maxdiff(lang, g["v_lang"]) < 1e-3


def test_training_step_matches_cpu_autograd(ops):
    """One stage-1 step (B=8, T=8 + the zero frame, 24x24, 1 encoder layer) against oracle.sbl_oracle.cls_forward + two
    F.cross_entropy calls under CPU autograd."""
    from oracle import sbl_oracle as O
    from sbl_for_multilingual_lip_reading_amd.transformer.classifier import cal_cls_loss
    from test_cls_cpu import _cls_shapes
    B, T, H, W = 8, 8, 24, 24
    m = _cls_model(1)
    sd = {}
    for k, v in detfill.fill_state_dict(_cls_shapes(1)).items():
        t = torch.from_numpy(v.copy())
        if t.is_floating_point() and "running_" not in k:
            t.requires_grad_(True)
        sd[k] = t
    x, _, _ = detfill.synthetic_batch(B, T, H, W, 31)
    t1, t2 = _targets(B, 31)
    t1[5] = IGN
    xt = torch.from_numpy(x)
    pre, ffn0 = {}, O.ffn

    def ffn_rec(sd_, prefix, h, drop=0.0):       # the oracle's feed-forward pre-activations, per FFN
        pre[prefix] = F.linear(h, sd_[prefix + ".w_1.weight"], sd_[prefix + ".w_1.bias"]).detach().reshape(-1, 2048)
        return ffn0(sd_, prefix, h, drop)
    O.ffn = ffn_rec
    try:
        feats, enc, rv, rlang = O.cls_forward(sd, xt, n_layers_enc=1)
    finally:
        O.ffn = ffn0
    rloss = F.cross_entropy(rv, t1, ignore_index=IGN) + 0.1 * F.cross_entropy(rlang, t2, ignore_index=IGN)
    rloss.backward()
    v, lang = m(torch.cat([xt, xt.new_zeros(B, 1, H, W)], 1).to(DEV))
    loss, stats = cal_cls_loss(v, lang, t1.to(DEV), t2.to(DEV))
    loss.backward()
    assert maxdiff(v, rv) < 1e-3 and maxdiff(lang, rlang) < 1e-3
    assert abs(loss.item() - rloss.item()) < 1e-4
    assert float(stats[1]) == B - 1 and float(stats[4]) == B
    # fc_* and encoder_v.*: 1e-3 of the tensor's largest entry with exact fp32 products; the split-bf16 trunk (bf16x6) feeds
    # the encoder through 17 train-mode BatchNorms at this small batch and gets the 2e-3 the end-to-end tests allow for
    # transformer gradients.  The absolute floor covers the analytically-zero key-projection bias gradients (rounding noise
    # of ~1e-9 on both sides).  visual_frontend.*: the end-to-end tests' frontend bound.
    # A hidden unit of a feed-forward whose pre-activation lies within rounding distance of 0 on some row can switch its ReLU
    # between two fp32-grade evaluations (test_hip_parity.py's check_transformer_grads tracks the same effect): its row of
    # w_1 / entry of b_1 / column of w_2 is held to the loose bound only.
    tol = 1e-3 if ops.get_matmul_precision() == "f32" else 2e-3
    near = {k: (h.abs() < 1e-4 * float(h.abs().max())).any(0) for k, h in pre.items()}
    assert all(int(v.sum()) < 64 for v in near.values())
    for n, p in m.named_parameters():
        ref, got = sd[n].grad, p.grad.detach().cpu()
        bound = tol * float(ref.abs().max()) + 1e-7
        if n.startswith("visual_frontend."):
            assert maxdiff(got, ref) < 3e-2 * float(ref.abs().max()) + 2e-6, n
            continue
        ffn = n.rsplit(".", 2)[0]
        if ffn in near and n.split(".")[-2] in ("w_1", "w_2"):
            j = near[ffn]
            keep = (~j if n.endswith("w_1.weight") or n.endswith("w_1.bias") else None)
            if keep is not None:
                assert maxdiff(got[keep], ref[keep]) < bound, (n, relerr(got, ref))
                assert maxdiff(got[j], ref[j]) < 3e-2 * float(ref.abs().max()) + 1e-7, n
                continue
            if n.endswith("w_2.weight"):
                assert maxdiff(got[:, ~j], ref[:, ~j]) < bound, (n, relerr(got, ref))
                assert maxdiff(got[:, j], ref[:, j]) < 3e-2 * float(ref.abs().max()) + 1e-7, n
                continue
        assert maxdiff(got, ref) < bound, (n, relerr(got, ref))


# --------------------------------------------------------------------------- data parallel, 2 ranks on the one GPU over gloo
def _dp_worker(rank, world, port, q, outdir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from sbl_for_multilingual_lip_reading_amd import dp
    torch.cuda.set_device(0)
    m = _cls_model()
    flat = dp.FlatModel(m)
    dp.broadcast_parameters(flat)
    ex = dp.GradientExchange(flat, world, overlap=True)
    hooks = len(ex._hooks)
    flat.zero_grad()
    _cls_step(m, 80 + rank)
    ex.finish()
    torch.cuda.synchronize()
    path = os.path.join(outdir, "grad%d.pt" % rank)
    torch.save(flat.flat_grad.detach().cpu(), path)
    q.put((rank, path, [s for s, _ in ex.launches], hooks))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_exchange_equals_mean_of_shard_gradients(tmp_path):
    import queue as _queue
    import time as _time
    from sbl_for_multilingual_lip_reading_amd import dp
    from sbl_for_multilingual_lip_reading_amd.transformer.classifier import ClassifierTransformer
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, 29651, q, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    got, t_end = {}, _time.time() + 300
    while len(got) < len(procs):                    # fail fast if a rank dies
        try:
            r, pth, order, hooks = q.get(timeout=2)
            got[r] = (torch.load(pth, weights_only=True), order, hooks)
        except _queue.Empty:
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            assert not dead, "a rank exited with %s" % dead
            assert _time.time() < t_end, "ranks did not finish in time"
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for r in range(2):
        order = got[r][1]
        assert got[r][2] == 5
        # hooks fired the segments in reverse-autograd order: heads, encoder_v, ResNet stages 4..2, then layer1 + stem
        assert [s for i, s in enumerate(order) if i == 0 or order[i - 1] != s] == list(ClassifierTransformer.FLAT_SEGMENTS)
    shard = []
    for r in range(2):
        m = _cls_model()
        flat = dp.FlatModel(m)
        flat.zero_grad()
        _cls_step(m, 80 + r)
        torch.cuda.synchronize()
        shard.append(flat.flat_grad.detach().cpu().double())
        ranges = dict(flat.ranges)
    mean = (shard[0] + shard[1]) / 2
    assert torch.equal(got[0][0], got[1][0])
    for seg, (a, b) in ranges.items():
        d = float((got[0][0][a:b].double() - mean[a:b]).norm() / mean[a:b].norm())
        assert d < (3e-2 if seg.startswith("visual") else 2e-3), (seg, d)


# --------------------------------------------------------------------------- checkpoints
def _trainer():
    from sbl_for_multilingual_lip_reading_amd import dp
    from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import FusedAdam, TransformerOptimizer
    m = _cls_model()
    flat = dp.FlatModel(m)
    return m, flat, TransformerOptimizer(FusedAdam(flat), warmup_steps=1)     # lr ~ 9e-3: three steps move every weight


def _train_step(m, opt, s):
    opt.zero_grad()
    _cls_step(m, 90 + s)
    opt.step()


def test_save_and_resume_equals_uninterrupted_training(tmp_path):
    from sbl_for_multilingual_lip_reading_amd import checkpoint
    m, flat, opt = _trainer()
    start = flat.flat_param.detach().cpu().double()
    for s in range(2):
        _train_step(m, opt, s)
    checkpoint.save_checkpoint(tmp_path / "ck.pt", m, opt, epoch=1)
    saved = [t.detach().cpu().clone() for t in (flat.flat_param, opt.optimizer.exp_avg, opt.optimizer.exp_avg_sq)]
    _train_step(m, opt, 2)
    torch.cuda.synchronize()
    a = flat.flat_param.detach().cpu().double()
    bufs_a = {k: v.detach().cpu().double() for k, v in m.named_buffers()}
    m2, flat2, opt2 = _trainer()
    meta = checkpoint.load_checkpoint(tmp_path / "ck.pt", m2, opt2)
    assert meta["epoch"] == 1 and opt2.step_num == 2 and opt2.optimizer.step_count == 2
    # the resumed state is the saved one, bit for bit: weights (flat buffer) and both Adam moments
    for x, y in zip(saved, (flat2.flat_param, opt2.optimizer.exp_avg, opt2.optimizer.exp_avg_sq)):
        assert torch.equal(x, y.detach().cpu())
    _train_step(m2, opt2, 2)
    torch.cuda.synchronize()
    b = flat2.flat_param.detach().cpu().double()
    assert float((a - start).abs().max()) > 1e-3                   # the steps did train
    # the third step itself is not bit-reproducible: the trunk's weight gradients and the BatchNorm / LayerNorm parameter
    # gradients are sums of float atomics, and Adam normalises every element's update, so a near-zero gradient whose last
    # bits differ moves its weight by a visible fraction of the learning rate (measured 2.5e-5 of the largest weight)
    assert float((a - b).abs().max() / a.abs().max()) < 1e-4
    # the heads' gradients are deterministic (sbl_cls_head_bwd): there the resumed step equals the uninterrupted one
    lo, hi = flat.ranges["fc_"]
    assert float((a[lo:hi] - b[lo:hi]).abs().max() / a[lo:hi].abs().max()) < 1e-6
    for k, v in m2.named_buffers():
        assert float((v.detach().cpu().double() - bufs_a[k]).abs().max()) <= 1e-6 * max(1.0, float(bufs_a[k].abs().max())), k


def test_stage1_frontend_and_encoder_carry_into_the_sbl_model(tmp_path):
    """A trained classifier's checkpoint loaded into the SBL Transformer (prefix_map for the encoder) gives the same frontend
    features and encoder output in eval BatchNorm."""
    from sbl_for_multilingual_lip_reading_amd import checkpoint
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    from sbl_for_multilingual_lip_reading_amd.transformer.transformer import Transformer
    m, flat, opt = _trainer()
    _train_step(m, opt, 0)
    checkpoint.save_checkpoint(tmp_path / "cls.pt", m)
    sbl = Transformer(Encoder(512, 1, 8, 64, 64, 512, 2048), Decoder(0, 1, 58, 512, 1, 8, 64, 64, 512, 2048), None).to(DEV)
    fe_before = sbl.visual_frontend.frontend3D[0].weight.detach().clone()
    checkpoint.load_checkpoint(tmp_path / "cls.pt", sbl, strict=False, prefix_map={"encoder_v.": "encoder."})
    assert not torch.equal(fe_before, sbl.visual_frontend.frontend3D[0].weight)
    m.eval()
    sbl.eval()
    for mod in (m, sbl):
        mod.visual_frontend.frontend_dropout_p = 0.0
    x = torch.from_numpy(detfill.synthetic_batch(3, 5, 24, 24, 41)[0]).to(DEV).unsqueeze(1)
    with torch.no_grad():
        f1, f2 = m.visual_frontend(x), sbl.visual_frontend(x)
        e1, e2 = m.encoder_v(f1, [5] * 3)[0], sbl.encoder(f2, [5] * 3)[0]
    assert float((f1 - f2).abs().max()) <= 1e-6 * max(1.0, float(f1.abs().max()))
    assert float((e1 - e2).abs().max()) <= 1e-6 * max(1.0, float(e1.abs().max()))
