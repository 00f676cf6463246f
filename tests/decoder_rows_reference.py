"""Plain numpy references of the decoder kernels that index rows through a SegDesc (csrc/sbl_common.h): the ragged stage
layout and the compact "ends" layout of the last decoder layer.  No torch, no GPU, nothing of the package: the tables below
are written from the prose of sbl_common.h and include/sbl_hip.h, and tests/test_decoder_rows_reference_cpu.py holds them
to torch (flip, F.embedding, argmax, autograd), to a brute-force triple loop and to the golden fixtures.

Layouts
    A stage (B, seg_L): segment s holds B sequences of length seg_L[s]; its B * seg_L[s] rows follow segment s-1's rows in
    (b, l) order.  stage_rows() gives (segment, b, l) of every row, flip_rows() the row of the time-flipped position of
    the same sequence, first_rows() / last_rows() the rows of position 0 / L-1 of sequence (s, b) in (s, b) order.
    Its ends layout keeps min(2, L) rows per sequence in (b, k) order, k = 0 -> position 0, k = Lc-1 -> position L-1;
    ends_table() gives (segment, b, k, full row) of every compact row.

Every float64 formula takes the fp32 inputs the kernel gets; the *32 functions return the fp32 result bit for bit where the
formula is one rounded operation (the factor 2 of the fusion is exact).
"""
import numpy as np

U = 2.0 ** -24
EW_BLOCK, EW_MAX_BLOCKS = 256, 8192            # ew_grid() of misc.hip / norm.hip, dec_grid() of decode_step.hip
D = 512

EDGE, SMALL, FULL, WIDE = (1,), (1, 2, 3), tuple(range(1, 17)), (16,) * 8
STAGE_B, WIDE_B = 32, 129


def f64(a):
    return np.asarray(a, dtype=np.float64)


def f32(a):
    return np.asarray(a, dtype=np.float32)


def cdiv(a, b):
    return (a + b - 1) // b


def ew_passes(n):
    """Trips of the grid-stride loop of a kernel launched with ew_grid(n) workgroups of 256 over n work items."""
    grid = min(max(cdiv(n, EW_BLOCK), 1), EW_MAX_BLOCKS)
    return cdiv(n, grid * EW_BLOCK)


# --------------------------------------------------------------------------- layouts
def stage_rows(B, seg_L):
    """(seg, b, l) int arrays over the rows of the stage, and row_off per segment."""
    seg, bb, ll, off, r = [], [], [], [], 0
    for s, L in enumerate(seg_L):
        off.append(r)
        j = np.arange(B * L)
        seg.append(np.full(B * L, s))
        bb.append(j // L)
        ll.append(j % L)
        r += B * L
    return np.concatenate(seg), np.concatenate(bb), np.concatenate(ll), np.asarray(off)


def n_rows(B, seg_L):
    return B * int(sum(seg_L))


def flip_rows(B, seg_L):
    """Row of position L-1-l of the same sequence, for every row."""
    seg, b, l, off = stage_rows(B, seg_L)
    L = np.asarray(seg_L)[seg]
    return off[seg] + b * L + (L - 1 - l)


def first_rows(B, seg_L):
    """Row of position 0 of sequence (s, b), in (s, b) order."""
    off = stage_rows(B, seg_L)[3]
    return np.concatenate([off[s] + np.arange(B) * L for s, L in enumerate(seg_L)])


def last_rows(B, seg_L):
    """Row of position L-1 of sequence (s, b), in (s, b) order: the rows the output heads read."""
    off = stage_rows(B, seg_L)[3]
    return np.concatenate([off[s] + np.arange(B) * L + L - 1 for s, L in enumerate(seg_L)])


def ends_table(B, seg_L):
    """(seg, b, k, full row) int arrays over the compact rows of the ends layout."""
    lc = [min(2, L) for L in seg_L]
    seg, b, k, _ = stage_rows(B, lc)
    off = stage_rows(B, seg_L)[3]
    L = np.asarray(seg_L)[seg]
    return seg, b, k, off[seg] + b * L + k * (L - 1)


def ends_full_rows(B, seg_L):
    return ends_table(B, seg_L)[3]


# --------------------------------------------------------------------------- embedding + positional encoding
def embed_index(tok, B, seg_L, V):
    """(vocabulary row, position) of every row of the stage: every segment reads tok[b, l]; ids are clamped to [0, V-1]."""
    _, b, l, _ = stage_rows(B, seg_L)
    return np.clip(np.asarray(tok)[b, l], 0, V - 1), l


def embed_index_flat(tok, B, L, V, pos0=0):
    """The same for the single-direction decoder's (B, L) rows, which read tok[b, pos0 + l] and pe[pos0 + l]."""
    j = np.arange(B * L)
    pos = j % L + pos0
    return np.clip(np.asarray(tok)[j // L, pos], 0, V - 1), pos


def embed_pe64(emb, pe, t, pos, scale=None):
    e = f64(emb)[t]
    return (e if scale is None else e * float(np.float32(scale))) + f64(pe)[pos]


def embed_pe32(emb, pe, t, pos):
    """emb[t] + pe[pos]: one fp32 add."""
    return f32(emb)[t] + f32(pe)[pos]


def fma32(a, b, c):
    """round_fp32(a * b + c) of fp32 arrays with ONE rounding.  a * b is exact in double (48 bits); the double sum s is
    rounded to 53 bits, which is monotone and keeps every fp32 midpoint, so narrowing s can only go wrong when s sits exactly
    on a midpoint and the true sum (s + err, err from the error-free TwoSum) does not: then err decides the direction."""
    p = f64(a) * f64(b)
    c = f64(c)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    d = s - f64(r)
    other = np.nextafter(r, np.where(d > 0, np.inf, -np.inf).astype(np.float32))
    tie = (d != 0) & (np.abs(d) == np.abs(f64(other) - s))
    return np.where(tie & (err != 0) & (np.sign(err) == np.sign(d)), other, r)


def embed_scale_pe32(emb, pe, t, pos, scale):
    """emb[t] * scale + pe[pos] both ways the compiler may emit it: (rounded product, then add) and (one fused multiply-add)."""
    e, p, s = f32(emb)[t], f32(pe)[pos], np.float32(scale)
    return (e * s) + p, fma32(e, np.broadcast_to(s, e.shape), p)


def embed_grad64(dy, t, V, scale=1.0):
    """(demb, sum of |terms|, rows per vocabulary row): demb[v] = sum over the rows with t == v of dy[row] * scale."""
    g = f64(dy) * float(np.float32(scale))
    demb, mag = np.zeros((V, g.shape[1])), np.zeros((V, g.shape[1]))
    np.add.at(demb, t, g)
    np.add.at(mag, t, np.abs(g))
    return demb, mag, np.bincount(t, minlength=V)


# --------------------------------------------------------------------------- fusion, gather-last
def fusion64(a, b, flip):
    """A' = A + flip(B), B' = 2 B + flip(A)."""
    a, b = f64(a), f64(b)
    return a + b[flip], 2.0 * b + a[flip]


def fusion_bwd64(da2, db2, flip):
    """The adjoint: dA = dA' + flip(dB'), dB = flip(dA') + 2 dB'."""
    da2, db2 = f64(da2), f64(db2)
    return da2 + db2[flip], da2[flip] + 2.0 * db2


def fusion32(a, b, flip):
    a, b = f32(a), f32(b)
    return a + b[flip], np.float32(2) * b + a[flip]


def fusion_bwd32(da2, db2, flip):
    da2, db2 = f32(da2), f32(db2)
    return da2 + db2[flip], da2[flip] + np.float32(2) * db2


def gather_last(x, last):
    return np.asarray(x)[last]


def gather_last_bwd(dy, last, rows):
    dy = np.asarray(dy)
    dx = np.zeros((rows, dy.shape[1]), dy.dtype)
    dx[last] = dy
    return dx


# --------------------------------------------------------------------------- stage tail
def tail_last64(yf0, yf1, first, last):
    """last_0 = A[L-1] + B[0], last_1 = 2 B[L-1] + A[0] per sequence (s, b)."""
    a, b = f64(yf0), f64(yf1)
    return a[last] + b[first], 2.0 * b[last] + a[first]


def tail_last32(yf0, yf1, first, last):
    a, b = f32(yf0), f32(yf1)
    return a[last] + b[first], np.float32(2) * b[last] + a[first]


def tail_logits64(last, w):
    """(logits, sum_k |last_k| |w_k|): the bias-free Linear(512, V) head."""
    return f64(last) @ f64(w).T, np.abs(f64(last)) @ np.abs(f64(w)).T


def first_argmax(x):
    """First maximal index along the last axis; a row of all -inf gives 0."""
    x = np.asarray(x)
    m = x.max(-1, keepdims=True)
    return np.argmax(x == m, -1).astype(np.int64)


def tail_tokens(ys, logits, B, nseg, step):
    """ys[b, step + 1] = first maximal index of the LAST segment's rows; everything else untouched."""
    out = np.array(ys, copy=True)
    out[:, step + 1] = first_argmax(logits[(nseg - 1) * B:nseg * B])
    return out


def argmax_select(pred, gold, ys, step, own):
    """ys[b, step + 1] = own ? first maximal index of pred[b] : gold[b, step]."""
    out = np.array(ys, copy=True)
    out[:, step + 1] = first_argmax(pred) if own else np.asarray(gold)[:, step]
    return out
