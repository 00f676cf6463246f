"""float64 reference of the train-mode compositions under the GPU's own dropout masks.

The arithmetic is oracle/sbl_oracle.py (and tests/seq2seq_oracle.py for the single-direction decoder) on float64 copies of
the state dict and the inputs; nothing here restates a transformer.  The oracle funnels every dropout decision through one
function, `_dropout(x, p, on)`, in a fixed call order: the encoder's PE dropout, then per layer the attention probabilities,
the attention output and the FFN output; in the SBL decoder per step the embedding of l2r, of r2l, then per layer l2r's five
sites (self probabilities, self output, cross probabilities, cross output, FFN output) and r2l's five.  masked_dropout()
replaces that function for the duration of a call by one that multiplies by the next mask of a PLAN and by the keep scale.

A plan is a list of (offset, base, p): the call's tensor x, flattened in C order, draws elements base .. base + x.numel() of
stream `offset` (dropout_sites.mask_range).  That is enough for every site of this project, because each oracle tensor is one
contiguous run of the kernel's index layout:
  * a tape launch over one segment (encoder, module tests, single-direction decoder): (B, L, D) rows are element m * D + c,
    the oracle's head-major (H*B, Lq, Lk) probabilities are ((h * B + b) * Lq + i) * Lk + j - the kernel's own order; base 0;
  * a decoder stage over the segments segL: step t is segment s of its stage; its rows start at B * sum(segL[:s]) * D, its
    self-attention block at H * B * sum(L^2 of the earlier segments), its cross-attention block at H * B * T * sum(L of the
    earlier segments) (include/sbl_hip.h; attention_routes.p_offsets, decoder_rows_reference.stage_rows);
  * the stage-batched decoder's sites are indexed by the element's place in the FULL 16-segment layout whatever stage (or
    compact "ends" row) computed it: the same three formulas over segL = 1..16, under the site's own un-folded offset.
The layouts are written down here from the header and those two restatements, not imported from decoder_stages.py.
"""
import contextlib

import numpy as np
import torch

import dropout_sites as DS
from oracle import sbl_oracle as O

H, D, ML = 8, 512, O.MAXLEN
LOGIT_BAR, LOSS_BAR = 1e-3, 1e-3
MARGIN = 1e-2                          # top-2 margin every own-argmax step of the reference must exceed: 10 x the logit bar


def grad_bound(ref):
    """check_transformer_grads' element-wise bound for a gradient with reference `ref`."""
    return 2e-3 * float(ref.abs().max()) + 2e-6


# --------------------------------------------------------------------------- the oracle under given masks
@contextlib.contextmanager
def masked_dropout(seed, plan):
    """Replace O._dropout by the plan's masks; on exit every entry must have been used."""
    state = {"k": 0}
    orig = O._dropout

    def _dropout(x, p, on):
        if not on:
            return x
        assert state["k"] < len(plan), "the oracle asks for more dropout sites than the plan has (%d)" % len(plan)
        off, base, pp = plan[state["k"]][:3]
        if len(plan[state["k"]]) > 3:
            assert plan[state["k"]][3] == x.numel(), (state["k"], plan[state["k"]], tuple(x.shape))
        state["k"] += 1
        assert abs(pp - p) < 1e-6, (pp, p)
        keep = DS.mask_range(seed, off, base, x.numel(), pp).reshape(tuple(x.shape))
        return x * torch.from_numpy(keep).to(x.dtype) * float(DS.keep_scale(pp))

    O._dropout = _dropout
    try:
        yield state
        assert state["k"] == len(plan), "the oracle used %d of the plan's %d sites" % (state["k"], len(plan))
    finally:
        O._dropout = orig


def to64(sd, requires_grad=True):
    """float64 leaf copies of the floating tensors of a state dict."""
    out = {}
    for k, v in sd.items():
        if v.is_floating_point():
            t = v.detach().double().clone()
            out[k] = t.requires_grad_(True) if requires_grad and "running_" not in k else t
        else:
            out[k] = v.clone()
    return out


def det_state(shapes, salt=0, gains=None, prefix=""):
    """{prefix + key: float32 tensor} by the deterministic fill (sbl_for_multilingual_lip_reading_amd.detfill)."""
    from sbl_for_multilingual_lip_reading_amd import detfill
    return {prefix + k: torch.from_numpy(detfill.fill_value(prefix + k, tuple(s), salt, gains).copy()) for k, s in shapes.items()}


def load_det(module, prefix, p, salt=0, gains=None):
    """Fill a HIP-backed module like det_state(prefix=...) and set every nn.Dropout of it to p -> the float32 state dict
    under the oracle's key names."""
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items() if not k.endswith("pe")}
    sd = det_state(shapes, salt, gains, prefix)
    own = module.state_dict()
    module.load_state_dict({k: (v if k.endswith("pe") else sd[prefix + k]) for k, v in own.items()})
    for mm in module.modules():
        if isinstance(mm, torch.nn.Dropout):
            mm.p = p
    return sd


# --------------------------------------------------------------------------- plans
def plan_in_order(records):
    """Single-segment tape launches: the k-th oracle site is the k-th forward record with p > 0, from element 0."""
    return [(r.offset, 0, r.p, r.count()) for r in records]


def stages_of(coins):
    """(first, last) step of every stage: a stage ends with the first own-argmax step (or the last step)."""
    out, i = [], 0
    for j in range(ML):
        if coins[j] or j == ML - 1:
            out.append((i, j))
            i = j + 1
    return out


def seg_bases(N, T, segL):
    """Per segment of a stage: (first row element, first self-attention probability, first cross-attention probability)."""
    out, r, ps, pe = [], 0, 0, 0
    for L in segL:
        out.append((r * D, ps, pe))
        r, ps, pe = r + N * L, ps + H * N * L * L, pe + H * N * L * T
    return out


def _site_base(bases, k):
    """Index base of site kind k (-1 = embedding, 0 self probabilities, 1 self output, 2 cross probabilities, 3 cross
    output, 4 FFN output) from a seg_bases() entry."""
    return bases[1] if k == 0 else bases[2] if k == 2 else bases[0]


def _site_count(N, T, L, k):
    return H * N * L * L if k == 0 else H * N * L * T if k == 2 else N * L * D


def site_order(nl):
    """The oracle's call order inside one decoder step: (direction, layer, kind); the two embeddings have layer -1."""
    return [(0, -1, -1), (1, -1, -1)] + [(d, n, k) for n in range(nl) for d in (0, 1) for k in range(5)]


_TAPE_NAMES = ("sbl_attention_seg_fwd", "sbl_add_layernorm_fwd", "sbl_attention_seg_fwd", "sbl_add_layernorm_fwd", "sbl_add_layernorm_fwd")


def tape_decoder_plan(records, N, T, nl, coins):
    """Per-stage tape (Decoder._run): every stage draws fresh offsets, in the oracle's own order (both embeddings, then per
    layer l2r's five launches and r2l's); step t is a segment of its stage's launches."""
    order = site_order(nl)
    recs = list(records)
    plan = [None] * ML
    for i0, i1 in stages_of(coins):
        segL = tuple(range(i0 + 1, i1 + 2))
        mine, recs = recs[:len(order)], recs[len(order):]
        assert len(mine) == len(order), "stage (%d, %d): %d dropout launches, expected %d" % (i0, i1, len(mine), len(order))
        for (d, n, k), r in zip(order, mine):
            want = "sbl_dropout" if k < 0 else _TAPE_NAMES[k]
            assert r.name == want, ((i0, i1), (d, n, k), r)
            assert r.count() == sum(_site_count(N, T, L, k) for L in segL), ((i0, i1), (d, n, k), r)
        bases = seg_bases(N, T, segL)
        for t in range(i0, i1 + 1):
            plan[t] = [(r.offset, _site_base(bases[t - i0], k), r.p, _site_count(N, T, t + 1, k)) for (d, n, k), r in zip(order, mine)]
    assert not recs, "%d dropout launches left over after the last stage" % len(recs)
    return [e for step in plan for e in step]


def batched_site_offsets(records, N, T, nl, coins):
    """Stage-batched decoder (decoder_stages.py): every stage's launches carry the site's offset folded with the stage's base
    in the FULL layout.  Un-fold each with the base written down here; a site's offset must come out the same from every
    stage and be a plain small counter value -> {(direction, layer, kind): offset}."""
    full = seg_bases(N, T, tuple(range(1, ML + 1)))
    recs = list(records)
    per_stage = 2 + 2 * 5 * nl
    raw = {}
    for i0, i1 in stages_of(coins):
        mine, recs = recs[:per_stage], recs[per_stage:]
        assert len(mine) == per_stage, "stage (%d, %d): %d offsets, expected %d" % (i0, i1, len(mine), per_stage)
        sites = [(0, -1, -1), (1, -1, -1)] + [(d, n, k) for n in range(nl) for k in range(5) for d in (0, 1)]      # slot pairs
        for (d, n, k), r in zip(sites, mine):
            assert r.slot == d and (r.name == "sbl_embed_pe_drop2_fwd") == (k < 0) and ("attention" in r.name) == (k in (0, 2)), ((d, n, k), r)
            off = DS.unfold(r.offset, _site_base(full[i0], k))
            assert off < (1 << 32), "stage (%d, %d), site %s: offset %d does not un-fold with the stage's base in the full layout" \
                % (i0, i1, (d, n, k), r.offset)
            assert raw.setdefault((d, n, k), off) == off, "site %s: stage (%d, %d) un-folds to offset %d, an earlier stage to %d" \
                % ((d, n, k), i0, i1, off, raw[(d, n, k)])
    assert not recs, "%d offsets left over after the last stage" % len(recs)
    return raw


def batched_decoder_plan(raw, N, T, nl, p):
    """The plan of the whole-buffer layout under the sites' own offsets `raw` (batched_site_offsets, or a synthetic table)."""
    full = seg_bases(N, T, tuple(range(1, ML + 1)))
    return [(raw[(d, n, k)], _site_base(full[t], k), p, _site_count(N, T, t + 1, k)) for t in range(ML) for (d, n, k) in site_order(nl)]


# --------------------------------------------------------------------------- SBL step
def sbl_step(sd, feats, tgt_l2r, tgt_r2l, coins, ne, nd, p, seed, plan, fed=None):
    """Encoder + SBL decoder + loss in the dtype of `sd` / `feats` under the plan's masks (encoder sites first).
    fed = (tokens_l2r, tokens_r2l), each (N, 16) int64: the tokens fed back at the own-argmax steps (the GPU's); None = the
    reference's own argmax.  Returns dict(enc, pred_l2r, pred_r2l, loss, argmax = the reference's own tokens at the
    own-argmax steps [(step, l2r (N,), r2l (N,))], margin = its smallest top-2 margin there)."""
    _, gold_l = O.preprocess(tgt_l2r)
    _, gold_r = O.preprocess(tgt_r2l)
    own, margins = [], []

    def nxt(i, pl, pr):
        if not coins[i]:
            return gold_l[:, i], gold_r[:, i]
        al, ar = pl.argmax(-1), pr.argmax(-1)
        own.append((i, al.clone(), ar.clone()))
        for pred in (pl, pr):
            top = pred.detach().topk(2, dim=-1).values
            margins.append(float((top[:, 0] - top[:, 1]).min()))
        return (al, ar) if fed is None else (fed[0][:, i], fed[1][:, i])

    with masked_dropout(seed, plan):
        enc = O.encoder(sd, feats, ne, drop=p)
        pl, pr, _, _ = O._decoder_steps(sd, enc, nd, H, nxt, p)
    out = {"enc": enc, "pred_l2r": pl, "gold_l2r": gold_l, "pred_r2l": pr, "gold_r2l": gold_r}
    out["loss"] = O.train_step_loss(out)
    out["argmax"], out["margin"] = own, (min(margins) if margins else float("inf"))
    return out


def synthetic_batched_plan(N, T, ne, nd, p, swap=None):
    """A made-up ledger for the CPU tests: distinct offsets in no particular order for the encoder's 1 + 3 * ne sites and the
    decoder's 2 + 10 * nd; swap = (site a, site b) of the decoder lets a draw b's stream."""
    enc_sites = [N * T * D] + [c for _ in range(ne) for c in (H * N * T * T, N * T * D, N * T * D)]
    enc_plan = [(1000 - 7 * i, 0, p, c) for i, c in enumerate(enc_sites)]
    raw = {s: 17 + 5 * ((11 * i) % 31) for i, s in enumerate(site_order(nd))}
    assert len(set(raw.values())) == len(raw) and 2 + 10 * nd <= 31
    if swap is not None:
        raw[swap[0]] = raw[swap[1]]
    return enc_plan + batched_decoder_plan(raw, N, T, nd, p)
