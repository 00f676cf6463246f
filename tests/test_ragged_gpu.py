"""GPU tests of ragged clips at inference: sbl_attention_seg_len_fwd on its three kernels against the float64
restatement of tests/ragged_reference.py within the bounds of tests/attention_routes.py, bit-identity with the grouped entry
on K/V cut to the count, poisoned rows behind the count, the model against the reference's own clip-by-clip decode
(tests/golden/ragged_*.npz, tools/make_ragged_goldens.py), full lengths against no lengths, every decode path of the Decoder,
and one hipGraph whose lengths tensor is overwritten in place between capture and replay."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

import attention_routes as A
import lexicon_cases as LC
import ragged_reference as R
import sbl_beam_oracle as PB
from conftest import load_golden, maxdiff
from sbl_for_multilingual_lip_reading_amd import detfill

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 777.25
SEED, OFFSET = 1234567, 7
V, SOS, EOS = 58, 0, 1


@pytest.fixture(scope="module", params=["f32", "bf16x6"])
def ops(request):
    from sbl_for_multilingual_lip_reading_amd import _lib, ops as _ops
    _lib.load()
    assert torch.cuda.is_available()
    _ops.set_matmul_precision(request.param)
    yield _ops
    _ops.set_matmul_precision("f32")


# --------------------------------------------------------------------------- the kernels
# (case, kv_len): the routes of the issue's table, then counts of 0, below 0 and above Lk on every route
KCASES = [
    (R.case("small_cross", 6, 3, (1, 2, 5), 29), (29, 1, 16, 17, 28, 2)),           # 54 problems: the last workgroup has idle wavefronts
    (R.case("small_cross_g3", 12, 3, (1, 2, 5), 29, 3), (29, 1, 16, 17)),           # B = 12 in groups of 3: four K/V entries
    (R.case("small_cross_g3x6", 18, 3, (1, 2, 5), 29, 3), (29, 1, 16, 17, 28, 2)),
    (R.case("small_self16", 3, 2, (16,), 0), (16, 1, 9)),
    (R.case("qtile_self29", 4, 2, (29,), 0), (1, 16, 17, 29)),
    (R.case("qtile_self32", 4, 2, (32,), 0), (1, 16, 17, 32)),
    (R.case("wg_cross33", 3, 2, (5,), 33), (32, 33, 1)),
    (R.case("wg_cross64", 3, 2, (5,), 64), (32, 33, 64)),
    (R.case("wg_self33", 3, 2, (33,), 0), (33, 1, 32)),
    (R.case("small_cross_clamp", 6, 3, (1, 2, 5), 29), (0, -3, 40, 29, 16, 1)),
    (R.case("small_self_clamp", 4, 2, (16,), 0), (0, 99, -1, 7)),
    (R.case("qtile_self_clamp", 4, 2, (29,), 0), (0, 99, -1, 17)),
    (R.case("wg_cross_clamp", 4, 2, (5,), 64), (0, 70, -2, 33)),
    (R.case("wg_self_clamp", 3, 2, (33,), 0), (0, 64, -5)),
]
ROUTES = {"small_cross": "small", "small_cross_g3": "small", "small_cross_g3x6": "small", "small_self16": "small", "qtile_self29": "qtile",
          "qtile_self32": "qtile", "wg_cross33": "workgroup", "wg_cross64": "workgroup", "wg_self33": "workgroup",
          "small_cross_clamp": "small", "small_self_clamp": "small", "qtile_self_clamp": "qtile", "wg_cross_clamp": "workgroup",
          "wg_self_clamp": "workgroup"}
KC = {c.name: (c, kv) for c, kv in KCASES}
_id = lambda v: v.name if hasattr(v, "name") else None      # noqa: E731


class Buf:
    """(rows + 2, nslots * HD) floats filled with `fill`; slot i is the column block [i * HD, (i + 1) * HD) of the first `rows`
    rows (the layout of the q/k/v and [K|V] projection buffers)."""

    def __init__(self, rows, nslots, HD, fill):
        self.rows, self.HD, self.ld, self.fill = rows, HD, nslots * HD, fill
        self.mat = torch.full((rows + 2, self.ld), fill, dtype=torch.float32, device=DEV)

    def slot(self, i):
        return self.mat[:self.rows, i * self.HD:(i + 1) * self.HD]

    def put(self, i, arr):
        self.slot(i).copy_(torch.from_numpy(np.ascontiguousarray(arr)))
        return self

    def untouched_outside(self, i):
        m = self.mat.clone()
        m[:self.rows, i * self.HD:(i + 1) * self.HD] = self.fill
        return bool((m == self.fill).all())


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return R.make_inputs(KC[name][0])


@functools.lru_cache(maxsize=None)
def _reference(name, drop_p):
    c, kv_len = KC[name]
    return R.reference(c, _inputs(name), kv_len, drop_p, SEED, OFFSET)


def _seed():
    return torch.tensor([SEED], dtype=torch.int64, device=DEV)


def _operands(c, inp, layout):
    """((buffer, slot) of q, k, v, o): contiguous buffers of their own, or the production packing - self-attention: q, k, v the
    three column blocks of one buffer; cross-attention: q a block of such a buffer, K / V the two blocks of another; o the
    middle block of a three-block buffer.  Input padding is NaN, o is pre-filled with a sentinel."""
    HD, Rq, Rk, nan = c.H * 64, A.rows_q(c), A.rows_k(c), float("nan")
    if layout == "contig":
        q, k, v = ((Buf(r, 1, HD, nan).put(0, inp[n]), 0) for n, r in (("q", Rq), ("k", Rk), ("v", Rk)))
        return q, k, v, (Buf(Rq, 1, HD, SENT), 0)
    qb = Buf(Rq, 3, HD, nan).put(0, inp["q"])
    if c.Lk:
        kvb = Buf(Rk, 2, HD, nan).put(0, inp["k"]).put(1, inp["v"])
        k, v = (kvb, 0), (kvb, 1)
    else:
        qb.put(1, inp["k"]).put(2, inp["v"])
        k, v = (qb, 1), (qb, 2)
    return (qb, 0), k, v, (Buf(Rq, 3, HD, SENT), 1)


def _call(ops, c, operands, kv_len=None, drop_p=0.0):
    """sbl_attention_seg_len_fwd (kv_len given) or sbl_attention_seg_grouped_fwd -> o as numpy, after the sentinel check"""
    args = []
    for b, i in operands:
        args += [b.slot(i).data_ptr(), b.ld]
    seed = _seed()
    tail = (A.SCALE, drop_p, seed.data_ptr() if drop_p else None, OFFSET, ops._s())
    seg = (ctypes.c_int * len(c.segL))(*c.segL)
    if kv_len is None:
        ops.call("sbl_attention_seg_grouped_fwd", *args, c.B, c.H, seg, len(c.segL), c.Lk, c.kvg, *tail)
    else:
        lens = torch.tensor(list(kv_len), dtype=torch.int32, device=DEV)
        ops.call("sbl_attention_seg_len_fwd", *args, c.B, c.H, seg, len(c.segL), c.Lk, c.kvg, lens.data_ptr(), *tail)
    torch.cuda.synchronize()
    ob, oi = operands[3]
    assert ob.untouched_outside(oi), "a store outside the output rows / columns"
    return ob.slot(oi).cpu().numpy()


@pytest.mark.parametrize("layout", ["contig", "packed"])
@pytest.mark.parametrize("c,kv_len", KCASES, ids=_id)
def test_every_route_against_float64(ops, c, kv_len, layout):
    """o within the bounds of attention_routes.py of the float64 restatement, without dropout and with it (the keep mask drawn
    at the indices of the call without counts); a sequence with count 0 (or below) gets exact zeros, a count above Lk clamps;
    the sentinels around o hold; the input padding is NaN."""
    assert R.route(c) == ROUTES[c.name]
    for drop_p in (0.0, 0.3):
        o = _call(ops, c, _operands(c, _inputs(c.name), layout), kv_len, drop_p)
        ref, bound = _reference(c.name, drop_p)
        ratio = A.compare({"o": (ref, bound)}, {"o": o}, ("o",))["o"]
        print("%s %s p=%.1f: o %.3g of the bound" % (c.name, layout, drop_p, ratio))
        assert ratio <= 1.0, (c.name, layout, drop_p, ratio)
        for pr in A.problems(c):
            if R.clamp(kv_len, c, pr) == 0:
                assert not o[pr["qrows"], pr["h"] * 64:pr["h"] * 64 + 64].any()


@pytest.mark.parametrize("name", ["small_cross", "small_cross_g3", "small_self16", "qtile_self29", "qtile_self32", "small_cross_clamp",
                                  "qtile_self_clamp"])
def test_trimmed_identity_on_the_one_wavefront_routes(ops, name):
    """Sequence by sequence, the ragged call is bit-identical to sbl_attention_seg_grouped_fwd on that entry's K/V cut to its
    count: masked keys contribute exact zeros and the key tiles are those of the count."""
    c, kv_len = KC[name]
    inp = _inputs(name)
    o = _call(ops, c, _operands(c, inp, "packed"), kv_len)
    for e in range(R.n_entries(c)):
        if min(max(kv_len[e], 0), c.Lk or c.segL[0]) == 0:
            continue
        sub, sinp, rows = R.trimmed(c, inp, kv_len, e)
        assert R.route(sub) in ("small", "qtile")
        want = _call(ops, sub, _operands(sub, sinp, "contig"))
        diff = np.flatnonzero(o[rows].view(np.uint32) != want.view(np.uint32))
        assert diff.size == 0, (name, e, diff[:8], o[rows].reshape(-1)[diff[:8]], want.reshape(-1)[diff[:8]])


@pytest.mark.parametrize("poison", [float("nan"), 1e30])
@pytest.mark.parametrize("name", ["small_cross", "small_cross_g3", "small_self16", "qtile_self29", "wg_cross33", "wg_cross64", "wg_self33",
                                  "small_cross_clamp", "wg_self_clamp"])
def test_poison_behind_the_count_never_reaches_o(ops, name, poison):
    """K/V rows >= count filled with NaN / 1e30 (self-attention: the K and V column blocks of those rows of the fused qkv buffer,
    Q left alone): o is bit-identical to the run with zeros there, on all three kernels."""
    c, kv_len = KC[name]
    outs = []
    for fill in (0.0, poison):
        inp = {n: a.copy() for n, a in _inputs(name).items()}
        for pr in A.problems(c):
            cols = slice(pr["h"] * 64, pr["h"] * 64 + 64)
            n = R.clamp(kv_len, c, pr)
            inp["k"][pr["krows"][n:], cols] = fill
            inp["v"][pr["krows"][n:], cols] = fill
        outs.append(_call(ops, c, _operands(c, inp, "packed"), kv_len))
    assert np.all(np.isfinite(outs[1])) and np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


# --------------------------------------------------------------------------- the model
_MODELS = {}


def _model(name):
    """The Transformer of a ragged fixture with the fixture's detfill weights, dropout off, eval mode; and the fixture."""
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    from sbl_for_multilingual_lip_reading_amd.transformer.transformer import Transformer
    if name not in _MODELS:
        g = load_golden(name + ".npz")
        ne, nd, B, T, H, W, salt = (int(v) for v in g["meta"])
        m = Transformer(Encoder(512, ne, 8, 64, 64, 512, 2048), Decoder(SOS, EOS, V, 512, nd, 8, 64, 64, 512, 2048), None)
        gains = json.loads(str(g["gains"]))
        m.load_state_dict({k: (v if k.endswith(".pe") else torch.from_numpy(detfill.fill_value(k, tuple(v.shape), salt, gains).copy()))
                           for k, v in m.state_dict().items()})
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        m.visual_frontend.frontend_dropout_p = 0.0
        _MODELS[name] = (m.to(DEV).eval(), g)
    return _MODELS[name]


def _decode(m, x, lens):
    """(tokens (N, 2, 17), logits (N, 2, 16, 58), encoder output) of the greedy decode under `lens` (None, list or tensor)."""
    with torch.no_grad():
        ys = m.recognize(x, lens)
        dev_lens = m._lengths(x, lens)
        enc, _ = m._encode(x, dev_lens)
        outs, ys2 = m.decoder._run(enc, None, None, teacher_mode=False, kv_len=dev_lens)
    assert torch.equal(ys[0], ys2[0]) and torch.equal(ys[1], ys2[1])
    logits = torch.stack([torch.stack(outs[d], 1) for d in (0, 1)], 1)
    return torch.stack(ys, 1).cpu().numpy(), logits.cpu().numpy(), enc.cpu().numpy()


@pytest.mark.parametrize("name", ["ragged_small", "ragged_full"])
def test_model_decodes_every_clip_as_the_reference_decodes_it_alone(ops, name):
    """Transformer.recognize(x, input_lengths) on the padded batch against the reference run clip by clip on the cut clip:
    the tokens exactly, every step's logits and the encoder rows < l within the project's 1e-3, the encoder rows >= l exactly
    0.  The host list and the CUDA tensor give bit-identical results.  Without lengths a short clip decodes differently."""
    m, g = _model(name)
    x = torch.from_numpy(g["clips"]).to(DEV)
    lengths = g["lengths"].tolist()
    tok, logits, enc = _decode(m, x, lengths)
    d_logit, d_enc = maxdiff(logits, g["logits"]), maxdiff(enc, g["enc"])
    print("%s: max|dlogit| %.2e, max|denc| %.2e" % (name, d_logit, d_enc))
    for n, l in enumerate(lengths):
        assert not enc[n, l:].any(), "an encoder row behind the clip's end is not zero"
    assert d_enc < 1e-3 and d_logit < 1e-3
    assert np.array_equal(tok, g["tokens"])
    tok_t, logits_t, enc_t = _decode(m, x, torch.tensor(lengths, dtype=torch.int32, device=DEV))
    assert np.array_equal(tok, tok_t) and np.array_equal(logits.view(np.uint32), logits_t.view(np.uint32))
    assert np.array_equal(enc.view(np.uint32), enc_t.view(np.uint32))
    tok_pad, _, _ = _decode(m, x, None)
    T = x.size(1)
    assert any(l < T and not np.array_equal(tok_pad[n], g["tokens"][n]) for n, l in enumerate(lengths))
    assert np.array_equal(tok_pad, g["tokens_padded"])


def test_full_lengths_equal_no_lengths(ops):
    """input_lengths = [T] * N as a CUDA tensor: tokens, pair-beam scores and encoder output bit-identical to None."""
    m, g = _model("ragged_small")
    x = torch.from_numpy(detfill.normal("ragged.full.clips", tuple(g["clips"].shape), 3)).to(DEV)
    full = torch.full((x.size(0),), x.size(1), dtype=torch.int32, device=DEV)
    a, b = _decode(m, x, None), _decode(m, x, full)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    with torch.no_grad():
        ra, rb = m.recognize_nbest(x, 3, 3), m.recognize_nbest(x, 3, 3, input_lengths=full)
    for k in ("ys_l2r", "ys_r2l", "scores", "scores_dir"):
        assert torch.equal(getattr(ra, k), getattr(rb, k)), k
    for ha, hb in zip(ra.history, rb.history):
        assert torch.equal(ha, hb)


_DECODERS = {}


def _decoder(salt):
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    if salt not in _DECODERS:
        sd = PB.decoder_state_dict(2, salt)
        dec = Decoder(SOS, EOS, V, 512, 2, 8, 64, 64, 512, 2048, dropout=0.0)
        own = dec.state_dict()
        dec.load_state_dict({k: (v if k.endswith("pe") else sd["decoder." + k]) for k, v in own.items()})
        _DECODERS[salt] = dec.to(DEV).eval()
    return _DECODERS[salt]


def _flat(res):
    """every tensor of a (nested) result tuple, on the host"""
    if isinstance(res, torch.Tensor):
        return [res.cpu().numpy().copy()]
    return [a for r in res for a in _flat(r)]


def test_every_decode_path_carries_the_lengths(ops, monkeypatch):
    """Decoder level, N = 4 clips of 8 encoder rows with lengths (8, 5, 1, 3): the rows >= l replaced by 1e4 x noise against zeros
    there.  recognize_beam, beam_search (W = 3), score_pairs (two chunks), recognize_words (K = 4) and beam_search_lex (W = 3, a
    12-word lexicon) return every field bit-identical; without the lengths the noise changes the result; beam_search(W = 1)
    is recognize_beam token for token under lengths."""
    from sbl_for_multilingual_lip_reading_amd.transformer import decoder as D
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    dec = _decoder(7)
    N, T, lengths = 4, 8, (8, 5, 1, 3)
    lens = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    clean = PB.encoder_output(N, T, 61)
    noisy = clean.clone()
    noise = PB.encoder_output(N, T, 62) * 1e4
    for n, l in enumerate(lengths):
        clean[n, l:] = 0.0
        noisy[n, l:] = noise[n, l:]
    lex = Lexicon(LC.make_lexicon(12, 5), device=DEV, vocab=V, sos_id=SOS, eos_id=EOS)
    monkeypatch.setattr(D, "SCORE_PAIRS_MAX_ROWS", 136 * 2 * 2)      # two clips of two slots per chunk: two chunks
    with torch.no_grad():
        pairs = dec.beam_search(clean.to(DEV), 3, 2, lens)
        n_pos = torch.tensor([16, 3, 9, 1, 16, 16, 5, 2], dtype=torch.int32, device=DEV)
        paths = {
            "recognize_beam": lambda e, l: dec.recognize_beam(e, l),
            "beam_search": lambda e, l: dec.beam_search(e, 3, 3, l),
            "score_pairs": lambda e, l: dec.score_pairs(e, pairs.ys_l2r, pairs.ys_r2l, n_pos, group=2, encoder_input_lengths=l),
            "recognize_words": lambda e, l: dec.recognize_words(e, lex, shortlist=4, encoder_input_lengths=l),
            "recognize_words_beam": lambda e, l: dec.recognize_words(e, lex, beam_size=3, nbest=2, shortlist=4, encoder_input_lengths=l),
            "beam_search_lex": lambda e, l: dec.beam_search_lex(e, lex, 3, 2, l),
        }
        for name, f in paths.items():
            a, b = _flat(f(clean.to(DEV), lens)), _flat(f(noisy.to(DEV), lens))
            assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), name
            assert not any(np.isnan(x).any() for x in a if x.dtype.kind == "f"), name
            if name != "recognize_beam":      # (tokens alone may survive the noise; every other path returns scores)
                free = _flat(f(noisy.to(DEV), None))
                assert not all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, free)), name + ": the rows behind the end change nothing"
        greedy = dec.recognize_beam(noisy.to(DEV), lens)
        one = dec.beam_search(noisy.to(DEV), 1, 1, lens)
    assert torch.equal(one.ys_l2r[:, 0], greedy[0]) and torch.equal(one.ys_r2l[:, 0], greedy[1])


def test_lengths_overwritten_in_place_under_one_hipgraph(ops):
    """validate and validate_words_lex captured once with a static lengths tensor; the lengths are overwritten in place; after
    the one replay the tokens, words and both meters' counters equal an eager run with the new lengths."""
    from sbl_for_multilingual_lip_reading_amd.transformer.lexicon import Lexicon
    from sbl_for_multilingual_lip_reading_amd.transformer.metrics import ErrorRateMeter, WordAccuracyMeter
    m, g = _model("ragged_small")
    x = torch.from_numpy(g["clips"]).to(DEV)
    N, T = x.shape[:2]
    _, l2r, r2l = (torch.from_numpy(a).to(DEV) for a in detfill.synthetic_batch(N, T, 2, 2, 17))
    lex = Lexicon(LC.make_lexicon(12, 5), device=DEV, vocab=V, sos_id=SOS, eos_id=EOS)
    gold = torch.tensor([0, 3, 7, 11], dtype=torch.int64, device=DEV)
    first, second = g["lengths"].tolist(), [3, 8, 6, 2]

    def run(lens, em, wm):
        return _flat((m.validate(x, l2r, r2l, em, input_lengths=lens),
                      m.validate_words_lex(x, gold, lex, wm, beam_size=3, nbest=2, input_lengths=lens)))
    with torch.no_grad():
        want = {}
        for key, ll in (("first", first), ("second", second)):
            em, wm = ErrorRateMeter(device=DEV), WordAccuracyMeter(device=DEV)
            want[key] = (run(torch.tensor(ll, dtype=torch.int32, device=DEV), em, wm), em.acc.tolist(), wm.acc.tolist())
        assert not all(np.array_equal(a, b) for a, b in zip(want["first"][0], want["second"][0])), "the lengths change nothing"
        static = torch.tensor(first, dtype=torch.int32, device=DEV)
        em, wm = ErrorRateMeter(device=DEV), WordAccuracyMeter(device=DEV)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            run(static, em, wm)                                   # warm-up on the capture stream
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            res = (m.validate(x, l2r, r2l, em, input_lengths=static),
                   m.validate_words_lex(x, gold, lex, wm, beam_size=3, nbest=2, input_lengths=static))
        em.reset()
        wm.reset()
        static.copy_(torch.tensor(second, dtype=torch.int32, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert em.acc.tolist() == want["second"][1] and wm.acc.tolist() == want["second"][2]
        got = _flat(res)
        assert len(got) == len(want["second"][0]) and all(np.array_equal(a, b) for a, b in zip(got, want["second"][0]))
