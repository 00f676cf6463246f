"""Plain numpy / float64 restatement of the four stage-1 classification entry points (sbl_cls_head_fwd, sbl_cls_loss_fwd,
sbl_cls_loss_bwd, sbl_cls_head_bwd) as include/sbl_hip.h documents them, the derived float32 error bound of every output,
the case tables of tests/test_cls_edges_gpu.py and the two comparison functions (exact, check) that module uses.  No GPU,
nothing of the package; tests/test_cls_reference_cpu.py holds this file to float64 torch autograd, to a float32
restatement of the loss rows, and shows that exact() / check() flag the one-line mistakes a kernel could make.

The tiles of csrc/cls_head.hip the tables are laid against: 8 classes per workgroup (CB), 4 clips per input-gradient
workgroup (RC), 512 classes per LDS chunk of those workgroups (KC; each of the four wavefronts takes a 128-class quarter, so
a chunk of <= 128 classes leaves quarters empty), 64 clips per pass of the logits kernel, 256 clips per LDS chunk of the
dW1 / db1 workgroups, 16 wavefronts over the rows of the loss forward, 4 rows per workgroup of the loss backward.

Exact cases.  Operands drawn from the integers -3..3 and T in {1, 2, 4}: every product, every partial sum and the division by
T of every linear output is a multiple of 1/T below 2^24 / T in magnitude, hence a float32, whatever the summation order.
The float64 result IS the float32 result, bit for bit.  exact_head_case() asserts that regime for every case it makes.

Bounds (U = 2^-24).  A float32 sum of n FMA terms in any order is within (n + 2) U sum|terms|.
    pooled    (T + 1) U sum_t|enc| / T
    logits1   (512 + T + 6) U (sum_d mean_t|enc| |W1| + |b1|)
    logits2   (512 + 2) U (sum_d |enc[:, li]| |W2| + |b2|)
    dW1, db1, dW2, db2   (N + 2) U sum_n|terms|; with accumulate the preset is one more term
    d_enc     (C1 + C2 + 3 + 2) U (sum_c|dlogits1 W1| / T + [t == li] sum_j|dlogits2 W2|)
    row loss  t_c = mx - x_c, p the float64 softmax, lse = log sum e^-t, A = sum_c (t_c + 2) p_c:
              B_loss = U (A + ceil(C/64) + 6 + 2|lse| + |lse + mx| + |loss_row|)
              (v - mx rounded and amplified through exp; two for expf; the lane-strided sum and its butterfly; two for
              logf; the two final adds)
    stats[0], stats[3]   sum of the rows' B_loss + (ceil(N/16) + 17) U sum|loss_row|
    loss      the two means' bounds + four roundings of its own value
    dlogits   B_d[c] = |scale| U (p_c (t_c + ceil(C/64) + A + 9) + |p_c - [c == g]| (3 + [c == g])) + 2^-120
              (scale the exact factor.  The softmax term carries t_c + 2 for its exponential, A + ceil(C/64) + 6 for the sum
              and 1 for the division; the subtraction of the one-hot, the at most two roundings of scale and the product
              act on the value they produce, |p_c - [c == g]|.  Away from the target that is p_c (t_c + ceil(C/64) + A +
              12); at a target with a small p_c it is 4, where charging those roundings to p_c alone leaves 1, which the
              float32 restatement of tests/test_cls_reference_cpu.py exceeds.  The last term covers float32 underflow of
              exp)
The GPU module allows 2x these bounds (the GPU's expf / logf against the host's), the float32 restatement on the CPU 1x.
"""
import numpy as np

U = 2.0 ** -24
D = 512
CB, RC, KC, LOGITS_PASS, DW_CHUNK, MAX_C2 = 8, 4, 512, 64, 256, 16
LOSS_WAVES, LOSS_BWD_ROWS = 16, 4
IGN = -100
TINY = 2.0 ** -120
OUT_FWD = ("pooled", "pooled_t", "logits1", "logits2")
OUT_BWD = ("d_enc", "dW1", "db1", "dW2", "db2")


def f64(a):
    return np.asarray(a, dtype=np.float64)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def cdiv(a, b):
    return (a + b - 1) // b


# --------------------------------------------------------------------------- heads
def head_fwd(enc, w1, b1, w2, b2, li):
    """float64 {pooled (N, D), pooled_t (D, N), logits1 (N, C1), logits2 (N, C2)} of float32 operands."""
    enc, w1, b1, w2, b2 = (f64(a) for a in (enc, w1, b1, w2, b2))
    pooled = enc.sum(1) / enc.shape[1]
    return {"pooled": pooled, "pooled_t": pooled.T.copy(), "logits1": pooled @ w1.T + b1, "logits2": enc[:, li] @ w2.T + b2}


def head_fwd_bounds(enc, w1, b1, w2, b2, li):
    a, w1, b1, w2, b2 = (np.abs(f64(x)) for x in (enc, w1, b1, w2, b2))
    T = a.shape[1]
    mean = a.sum(1) / T
    pooled = (T + 1) * U * mean
    return {"pooled": pooled, "pooled_t": pooled.T.copy(), "logits1": (D + T + 6) * U * (mean @ w1.T + b1),
            "logits2": (D + 2) * U * (a[:, li] @ w2.T + b2)}


def head_bwd(enc, pooled, d1, d2, w1, w2, li, want=OUT_BWD, accumulate=0, preset=None):
    """float64 outputs of sbl_cls_head_bwd for the names in `want` (a NULL output is absent from the result).  pooled is the
    float32 buffer the kernel is handed.  accumulate = 1 adds the four parameter gradients to preset[name]; d_enc is
    written, never added to."""
    enc, pooled, d1, d2, w1, w2 = (f64(a) for a in (enc, pooled, d1, d2, w1, w2))
    N, T, _ = enc.shape
    out = {}
    if "d_enc" in want:
        de = np.repeat((d1 @ w1 / T)[:, None, :], T, axis=1)
        de[:, li] = de[:, li] + d2 @ w2
        out["d_enc"] = de
    full = {"dW1": lambda: d1.T @ pooled, "db1": lambda: d1.sum(0), "dW2": lambda: d2.T @ enc[:, li], "db2": lambda: d2.sum(0)}
    for k, fn in full.items():
        if k in want:
            out[k] = fn() + (f64(preset[k]) if accumulate else 0.0)
    return out


def head_bwd_bounds(enc, pooled, d1, d2, w1, w2, li, want=OUT_BWD, accumulate=0, preset=None):
    enc, pooled, d1, d2, w1, w2 = (np.abs(f64(a)) for a in (enc, pooled, d1, d2, w1, w2))
    N, T, _ = enc.shape
    C1, C2 = w1.shape[0], w2.shape[0]
    out = {}
    if "d_enc" in want:
        s = np.repeat((d1 @ w1 / T)[:, None, :], T, axis=1)
        s[:, li] = s[:, li] + d2 @ w2
        out["d_enc"] = (C1 + C2 + 3 + 2) * U * s
    full = {"dW1": lambda: d1.T @ pooled, "db1": lambda: d1.sum(0), "dW2": lambda: d2.T @ enc[:, li], "db2": lambda: d2.sum(0)}
    acc = 1 if accumulate else 0
    for k, fn in full.items():
        if k in want:
            out[k] = (N + 2 + acc) * U * (fn() + (np.abs(f64(preset[k])) if acc else 0.0))
    return out


# --------------------------------------------------------------------------- loss
def ce_rows(x, tgt, ignore_id=IGN):
    """Per row of the float32 logits x (N, C): everything the loss and its bounds are made of, in float64.
    valid = target is not ignore_id; row = logsumexp(x) - x[g] (NaN for a target outside [0, C), 0 on ignored rows);
    correct = valid and the FIRST maximal index equals the target."""
    x, tgt = f64(x), np.asarray(tgt, dtype=np.int64)
    N, C = x.shape
    mx = x.max(1)
    t = mx[:, None] - x
    e = np.exp(-t)
    se = e.sum(1)
    p = e / se[:, None]
    lse = np.log(se)
    valid = tgt != ignore_id
    inside = (tgt >= 0) & (tgt < C)
    g = np.where(inside, tgt, 0)
    row = (lse + mx) - x[np.arange(N), g]
    row = np.where(inside, row, np.nan)
    row = np.where(valid, row, 0.0)
    correct = valid & (x.argmax(1) == tgt)                      # np.argmax: first occurrence
    A = ((t + 2.0) * p).sum(1)
    passes = cdiv(C, 64)
    b_row = np.where(valid, U * (A + passes + 6 + 2 * np.abs(lse) + np.abs(lse + mx) + np.abs(row)), 0.0)
    onehot = np.zeros((N, C))
    onehot[np.arange(N)[inside], g[inside]] = 1.0
    return {"t": t, "p": p, "lse": lse, "mx": mx, "A": A, "passes": passes, "valid": valid, "inside": inside, "row": row,
            "correct": correct, "b_row": b_row, "onehot": onehot}


def loss_fwd(l1, l2, t1, t2, lw, ignore_id=IGN):
    """{"loss", "stats" (6), "b_loss", "b_stats" (6: 0 for the counts)} of sbl_cls_loss_fwd.  lang_weight crosses the ABI as
    a float, so the reference takes its float32 value."""
    lw = float(np.float32(lw))
    N = np.asarray(l1).shape[0]
    stats, b_stats, means, b_means = np.zeros(6), np.zeros(6), [], []
    for h, (x, t) in enumerate(((l1, t1), (l2, t2))):
        r = ce_rows(x, t, ignore_id)
        s, v = r["row"].sum(), float(r["valid"].sum())
        b = r["b_row"].sum() + (cdiv(N, LOSS_WAVES) + 17) * U * np.abs(r["row"]).sum()
        stats[3 * h:3 * h + 3] = (s, v, float(r["correct"].sum()))
        b_stats[3 * h] = b
        with np.errstate(divide="ignore", invalid="ignore"):
            means.append(np.float64(s) / np.float64(v))
            b_means.append(np.float64(b) / np.float64(v))
    loss = means[0] + lw * means[1]
    # four more roundings (two divisions, the product, the sum) of its own value: |a| + |b| = |loss| for lang_weight >= 0
    b_loss = b_means[0] + abs(lw) * b_means[1] + 4 * U * (abs(means[0]) + abs(lw * means[1]))
    return {"loss": loss, "stats": stats, "b_loss": b_loss, "b_stats": b_stats}


def loss_bwd(l1, l2, t1, t2, lw, gscale, ignore_id=IGN):
    """{"d1", "d2", "b_d1", "b_d2", "rows1", "rows2"} of sbl_cls_loss_bwd: dlogits = gscale / valid * (softmax - onehot),
    times lang_weight for head 2, 0 on ignored rows.  rows* marks the rows the contract defines (a row whose target is
    neither ignore_id nor inside [0, C) has a NaN loss and no documented gradient)."""
    lw, gscale = float(np.float32(lw)), float(np.float32(gscale))
    out = {}
    for h, (x, t) in enumerate(((l1, t1), (l2, t2))):
        r = ce_rows(x, t, ignore_id)
        v = float(r["valid"].sum())
        scale = (gscale * (lw if h else 1.0)) / v if v else 0.0
        keep = r["valid"][:, None]
        d = np.where(keep, scale * (r["p"] - r["onehot"]), 0.0)
        b = abs(scale) * U * (r["p"] * (r["t"] + r["passes"] + r["A"][:, None] + 9) +
                              np.abs(r["p"] - r["onehot"]) * (3 + r["onehot"])) + TINY
        out["d%d" % (h + 1)] = d
        out["b_d%d" % (h + 1)] = np.where(keep, b, 0.0)
        out["rows%d" % (h + 1)] = ~r["valid"] | r["inside"]
    return out


# --------------------------------------------------------------------------- comparisons (shared with the GPU module)
def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def exact(what, got, ref):
    """torch.equal(got, ref) as float32: the same shape and every element equal (a NaN equals nothing)."""
    import torch
    got, ref = _host(got), _host(ref)
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    r32 = f32(ref)
    assert np.array_equal(f64(r32), f64(ref)), what + ": the expected values are not float32"
    if not torch.equal(torch.from_numpy(np.ascontiguousarray(got)), torch.from_numpy(r32)):
        bad = got != r32
        first = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, expected %r" %
                             (what, int(bad.sum()), bad.size, first, got[first], r32[first]))


def check(what, got, ref, bound, factor=1.0, rows=None):
    """|got - ref| <= factor * bound for every element (bound == 0: equal).  rows: boolean mask over the first axis of the
    rows that are compared.  Prints and returns the worst error / bound ratio (against 1x the bound)."""
    got, ref = f64(_host(got)), f64(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound = np.broadcast_to(f64(bound), ref.shape)
    if rows is not None:
        got, ref, bound = got[rows], ref[rows], bound[rows]
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(bound)), what + ": non-finite reference"
    assert np.all(np.isfinite(got)), what + ": non-finite output"
    err = np.abs(got - ref)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    worst = float(ratio.max()) if ratio.size else 0.0
    print("RATIO %-62s %.3f  (max err %.3e)" % (what, worst, float(err.max()) if err.size else 0.0))
    assert worst <= factor, "%s: err/bound %.3f > %g at %s" % (what, worst, factor,
                                                             np.unravel_index(int(ratio.argmax()), ratio.shape))
    return worst


# --------------------------------------------------------------------------- case tables
def _hc(edge, N=5, C1=9, C2=2, T=2, li=1):
    return {"id": "N%d-C1_%d-C2_%d-T%d-li%d-%s" % (N, C1, C2, T, li, edge), "N": N, "C1": C1, "C2": C2, "T": T, "li": li}


# exact cases: one axis at an edge, the others small (N = 5: two input-gradient groups, the second with one clip)
HEAD_EXACT = [
    _hc("one-clip", N=1), _hc("rc-group-short", N=3), _hc("rc-group-full", N=4), _hc("rc-group-plus-one", N=5),
    _hc("logits-pass-short", N=63), _hc("logits-pass-full", N=64), _hc("logits-second-pass", N=65),
    _hc("dw1-chunk-full", N=256), _hc("dw1-second-256-clip-chunk", N=257), _hc("dw1-second-chunk-44-clips", N=300),
    _hc("one-class-empty-quarters", C1=1), _hc("slice-short-empty-quarters", C1=7), _hc("slice-full-empty-quarters", C1=8),
    _hc("quarter-short-empty-quarters", C1=127), _hc("quarter-full-empty-quarters", C1=128), _hc("second-quarter-one-class", C1=129),
    _hc("chunk-short", C1=511), _hc("chunk-full", C1=512), _hc("second-chunk-one-class-empty-quarters", C1=513),
    _hc("model-width", C1=1500),
    _hc("one-language", C2=1), _hc("three-languages", C2=3), _hc("max-c2", C2=16),
    _hc("single-frame", T=1, li=0), _hc("first-frame", T=2, li=0), _hc("first-of-four", T=4, li=0),
    _hc("middle-frame", T=4, li=2), _hc("last-of-four", T=4, li=3),
    _hc("all-edges-at-once", N=300, C1=1500, C2=16, T=4, li=2),
]
HEAD_NULL = [_hc("null-outputs", N=5), _hc("null-outputs-second-256-clip-chunk", N=257)]
NULL_COMBOS = {"d_enc-only": ("d_enc",), "head1-pair-only": ("dW1", "db1"), "head2-pair-only": ("dW2", "db2"),
               "all-but-d_enc": ("dW1", "db1", "dW2", "db2")}

# bounded cases: the same edges where the mean over time is not exact
HEAD_REAL = [
    _hc("one-clip-model-width", N=1, C1=1500, C2=2, T=31, li=30), _hc("small", N=5, C1=9, C2=3, T=3, li=1),
    _hc("full-tiles-one-language", N=4, C1=8, C2=1, T=3, li=0), _hc("short-tiles-max-c2", N=3, C1=7, C2=16, T=31, li=0),
    _hc("short-pass-short-quarter", N=63, C1=127, C2=2, T=3, li=1), _hc("full-pass-full-quarter", N=64, C1=128, C2=2, T=3, li=1),
    _hc("second-pass-second-quarter", N=65, C1=129, C2=16, T=3, li=2), _hc("long-clips-short-chunk", N=33, C1=511, C2=2, T=31, li=15),
    _hc("dw1-chunk-full-chunk-full", N=256, C1=512, C2=3, T=3, li=0),
    _hc("dw1-second-256-clip-chunk-second-class-chunk", N=257, C1=513, C2=2, T=3, li=2),
    _hc("all-edges-at-once", N=300, C1=1500, C2=16, T=3, li=1),
]


def _lc(edge, N, C1, C2, spread=3, gscale=1.0, lw=0.1, ignore=False):
    return {"id": "N%d-C%dx%d-spread%d-g%g-lw%g%s-%s" % (N, C1, C2, spread, gscale, lw, "-ign" if ignore else "", edge),
            "N": N, "C1": C1, "C2": C2, "spread": spread, "gscale": gscale, "lw": lw, "ignore": ignore}


LOSS_CASES = [
    _lc("one-row", 1, 63, 2), _lc("bwd-group-full", 4, 64, 3), _lc("loss-bwd-fifth-row", 5, 65, 64, ignore=True),
    _lc("fwd-waves-short", 15, 2, 16, spread=30), _lc("fwd-waves-full", 16, 129, 65, ignore=True),
    _lc("loss-fwd-17th-row", 17, 1500, 2, ignore=True), _lc("fwd-third-round", 33, 129, 65, spread=30, ignore=True),
    _lc("one-class-each", 5, 1, 1), _lc("two-classes-wide-head2", 5, 2, 16, spread=80), _lc("lanes-short", 5, 63, 2, spread=30),
    _lc("lanes-full", 5, 64, 3, spread=80), _lc("second-lane-pass", 5, 65, 64, spread=30),
    _lc("third-lane-pass", 5, 129, 65, spread=80), _lc("model-width", 5, 1500, 2, spread=30),
    _lc("model-width-underflow", 17, 1500, 2, spread=80), _lc("gscale-fraction", 5, 65, 64, gscale=0.37),
    _lc("gscale-negative", 17, 129, 65, gscale=-2.0, ignore=True), _lc("gscale-zero", 5, 64, 3, gscale=0.0, ignore=True),
    _lc("lang-weight-zero", 5, 63, 2, lw=0.0), _lc("lang-weight-other", 17, 1500, 2, gscale=0.37, lw=1.5, ignore=True),
    _lc("lang-weight-other-negative-gscale", 33, 2, 16, spread=30, gscale=-2.0, lw=1.5),
    _lc("one-class-each-full-waves", 16, 1, 1, ignore=True), _lc("everything-scaled", 4, 1500, 2, spread=80, gscale=0.37, lw=1.5),
    _lc("short-waves-ignored", 15, 65, 64, ignore=True), _lc("one-row-model-width", 1, 1500, 2, spread=30),
]
LOSS_BY_ID = {c["id"]: c for c in LOSS_CASES}

# equal maxima at (lower, higher): neighbours; one lane in two passes; the lower index in the higher lane; first and last
TIE_PAIRS = {1500: ((5, 6), (5, 69), (64, 1), (0, 1499)), 65: ((5, 6), (64, 1), (0, 64))}


def _rng(case, salt):
    return np.random.default_rng([salt] + [ord(ch) for ch in case["id"]])


def _ints(rng, *shape):
    return rng.integers(-3, 4, size=shape).astype(np.float32)


def exact_head_case(case):
    """Integer operands, gradients and accumulate presets of an exact case.  Asserts the exact regime: every sum of |terms|
    of every output, in units of 1/T, stays below 2^24 (returned as "grid_max")."""
    N, C1, C2, T, li = (case[k] for k in ("N", "C1", "C2", "T", "li"))
    assert T in (1, 2, 4) and 0 <= li < T and 1 <= C2 <= MAX_C2
    g = _rng(case, 1)
    o = {"enc": _ints(g, N, T, D), "w1": _ints(g, C1, D), "b1": _ints(g, C1), "w2": _ints(g, C2, D), "b2": _ints(g, C2),
         "d1": _ints(g, N, C1), "d2": _ints(g, N, C2),
         "preset": {"d_enc": _ints(g, N, T, D), "dW1": _ints(g, C1, D), "db1": _ints(g, C1), "dW2": _ints(g, C2, D),
                    "db2": _ints(g, C2)}}
    a = {k: np.abs(f64(v)) for k, v in o.items() if k != "preset"}
    pre = {k: np.abs(f64(v)) for k, v in o["preset"].items()}
    st = a["enc"].sum(1)                                   # T * mean|enc|: pooled in units of 1/T
    sums = [st, st @ a["w1"].T + T * a["b1"], T * (a["enc"][:, li] @ a["w2"].T + a["b2"]),
            a["d1"].T @ st + T * pre["dW1"], T * (a["d1"].sum(0) + pre["db1"]),
            T * (a["d2"].T @ a["enc"][:, li] + pre["dW2"]), T * (a["d2"].sum(0) + pre["db2"]),
            a["d1"] @ a["w1"] + T * (a["d2"] @ a["w2"])]
    o["grid_max"] = float(max(s.max() for s in sums))
    assert o["grid_max"] < 2.0 ** 24, (case["id"], o["grid_max"])
    return o


def real_head_case(case):
    """randn operands whose rows are scaled by powers of two across 2^-6 .. 2^6 (clips of enc and of the gradients, classes
    of the weights, biases and gradients), so that small and large outputs sit in one tensor."""
    N, C1, C2, T = (case[k] for k in ("N", "C1", "C2", "T"))
    g = _rng(case, 2)
    rn = lambda *s: g.standard_normal(s)
    p2 = lambda n, step: 2.0 ** (((np.arange(n) * step) % 13) - 6)
    sn, s1, s2 = p2(N, 5), p2(C1, 7), p2(C2, 3)
    o = {"enc": rn(N, T, D) * sn[:, None, None], "w1": rn(C1, D) * s1[:, None], "b1": rn(C1) * s1,
         "w2": rn(C2, D) * s2[:, None], "b2": rn(C2) * s2,
         "d1": rn(N, C1) * p2(N, 3)[:, None] * p2(C1, 11), "d2": rn(N, C2) * p2(N, 3)[:, None] * p2(C2, 5),
         "preset": {"d_enc": rn(N, T, D), "dW1": rn(C1, D) * s1[:, None], "db1": rn(C1) * s1, "dW2": rn(C2, D), "db2": rn(C2)}}
    o["preset"] = {k: f32(v) for k, v in o["preset"].items()}
    return {k: (v if k == "preset" else f32(v)) for k, v in o.items()}


def loss_case(case):
    """Logits of the given spread and targets of a loss case.  ignore: rows 1, 4, .. of head 1 and rows 2, 6, .. of head 2
    carry ignore_id (N >= 4 keeps valid rows in both heads).  Every head has an all-equal row (row 0) and a row with a +60
    peak (its last valid row; with one row: head 1 all equal, head 2 peaked)."""
    N, C1, C2 = case["N"], case["C1"], case["C2"]
    g = _rng(case, 3)
    out = {}
    for h, C in ((1, C1), (2, C2)):
        x = f32(g.standard_normal((N, C)) * case["spread"])
        t = g.integers(0, C, size=N).astype(np.int64)
        if case["ignore"]:
            assert N >= 4
            t[(1 if h == 1 else 2)::(3 if h == 1 else 4)] = IGN
        if N > 1 or h == 1:
            x[0] = x[0, 0]
        if N > 1 or h == 2:
            r = max(i for i in range(N) if t[i] != IGN and (i > 0 or N == 1))
            k = int(g.integers(0, C))
            x[r, k] = x[r].max() + np.float32(60.0)
            if h == 1:
                t[r] = k                          # head 1: the target is the peak (softmax - onehot cancels); head 2: it is not
        out["l%d" % h], out["t%d" % h] = x, t
    return out


def tie_case(C1, C2, target):
    """One row per pair of TIE_PAIRS: both classes of the pair hold the row's maximum; target = "lower" or "higher"."""
    g = np.random.default_rng([4, C1, C2])
    n = max(len(TIE_PAIRS[C1]), len(TIE_PAIRS[C2]))
    out = {}
    for h, C in ((1, C1), (2, C2)):
        pairs = [TIE_PAIRS[C][i % len(TIE_PAIRS[C])] for i in range(n)]
        x = f32(g.standard_normal((n, C)))
        t = np.zeros(n, dtype=np.int64)
        for r, (a, b) in enumerate(pairs):
            x[r, a] = x[r, b] = x[r].max() + np.float32(1.0)
            t[r] = min(a, b) if target == "lower" else max(a, b)
        out["l%d" % h], out["t%d" % h] = x, t
    return out
