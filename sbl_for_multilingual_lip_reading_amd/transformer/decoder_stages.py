"""The SBL decoder's 16 steps as ONE autograd node with a stage-batched backward.

Forward has to run stage by stage: a stage (a maximal run of teacher-forced steps, decoder.stages_of) needs the
previous stage's argmax token (decoder.py:173-186).  Backward has no such dependency - tokens are not differentiable -
so the backward of ALL 16 steps is one ragged batch: per layer and direction one LayerNorm / attention / GEMM launch
over the N*136 rows of every step (the N*31 end rows behind the last layer's self-attention, see below), instead of one per
stage.  The dependent chain shrinks from
11 kernels x 6 layers x (1 + #own-argmax coins) to 11 x 6, and its GEMMs are 4352-row products instead of 100-1500.

To make that possible every stage's forward writes its activations into row ranges of per-layer buffers laid out
as the 16-segment ragged batch (segment t = the step with prefix length t+1, rows N*t*(t+1)/2 ...), with the raw
C-ABI kernels (no per-op tape).  There is one launch sequence: per stage one launch for the embeddings of both directions,
per layer the sbl_*2_* entry points that serve both directions at once (the last LayerNorm of a layer also makes the
cross-direction fusion that feeds the next one), and one stage-tail launch (last fusion at the last positions, both heads,
next token); the cross-attention K/V of all 12 layers come from one GEMM before the first stage.  Dropout masks are functions of (seed, stream offset, element index); a stage passes
an offset that folds its row base in (the generator is affine in both, see _fold), so the batched backward
regenerates exactly the masks of the forward with plain whole-buffer indices.

The backward of a layer is ops.ffn_bwd / ops.attn_bwd (what the per-stage tape's MHAFn / FFNFn run) over these buffers, with a
sink that collects the weight gradients for one grouped launch; only the paired forward is a launch sequence of this file.

The last layer runs on its "ends" rows (Decoder.last_layer_ends_only).  Of its output a step reads two rows per sequence:
the stage tail forms A'[L-1] = A[L-1] + B[0] and B'[L-1] = 2 B[L-1] + A[0] (decoder.py:160-167), so every other row has a
gradient of exactly zero.  Its QKV product and self-attention core still cover all rows (the two surviving queries attend to
every key); one gather then takes positions 0 and L-1 of att and of the residual x into a compact layout - segment t keeps
min(2, t+1) rows per sequence in (b, k) order, N*31 rows instead of N*136 (decoder.ends_rows is the map) - and the
out-projection, the cross-attention sub-layer and the feed-forward sub-layer run on those rows through the same entry points
with a smaller M (sbl_*_ends_* for the LayerNorm and attention kernels, which draw every dropout decision from the element's
place in the FULL layout: masks, and so results, are those of the full-row computation).  Backward mirrors it: a tail adjoint
writes the compact dy from the heads' gradients, the sub-layer adjoints run compact, one scatter writes the full-size datt and residual
gradient (their end rows, zero everywhere else: no separate zero fill), and the self-attention core and QKV adjoints run on all rows.
Off, or with more than 32 encoder frames (the compact cross-attention is built on the one-wavefront kernels) = every launch of
the last layer covers all rows, as in the other layers.

Used by Decoder.forward when gradients accumulate into persistent buffers (dp.FlatModel) and the coins are known on
the host (supported() has the full list); every other case keeps the per-stage tape (Decoder._run).  Same numbers as that
path (tests compare them).
"""
import torch

from . import decoder as _decoder
from ._env import config, ops

_C1 = 0x9E3779B97F4A7C15
_C2 = 0xD1B54A32D192ED03
_K = (_C2 * pow(_C1, -1, 1 << 64)) % (1 << 64)
_MASK = (1 << 64) - 1


def _fold(offset, base):
    """Stream offset that makes element i of a sub-tensor draw what element base+i of the whole tensor draws:
    sbl_rand_u32 hashes seed + C1*(offset+1) + C2*idx in wrap-around 64-bit arithmetic and C1 is odd."""
    return ((offset + 1 + base * _K) & _MASK) - 1 & _MASK


def supported(dec, encoder_outputs):
    """The parameter handles ([direction][layer] of _layer) the fast path runs on, or None when it does not apply.  It needs
    persistent gradient buffers for every decoder parameter (kernels accumulate there), host coins, CUDA, the 512-wide /
    at-most-64-token geometry the fused stage head and tail are built for, the 2 * n_layers cross-attention [W_k; W_v]
    pairs (biases and gradient buffers too) as rows of one matrix in (direction, layer) order - dp.FlatModel lays a whole
    Transformer out like that - and, per layer, the same dropout probabilities and LayerNorm eps in both directions
    (they share launches)."""
    if not (dec.batched_backward and encoder_outputs.is_cuda and torch.is_grad_enabled() and dec.coins_dev is None):
        return None
    if dec.d_model != 512 or encoder_outputs.size(-1) != 512 or dec.tgt_word_emb.weight.size(0) > 64 or not dec.batch_teacher_runs:
        return None
    if any(ops._gbuf(p) is None for p in dec.parameters()):
        return None
    ws, bs = ops.kv_block([l.enc_attn for d in (0, 1) for l in dec._layers(d)])
    if not all(ops._adjacent(*ts) and ops._adjacent(*map(ops._gbuf, ts)) for ts in (ws, bs)):
        return None
    layers = [[_layer(l) for l in dec._layers(d)] for d in (0, 1)]
    if any((h0.drop_p, h0.ln[4]) != (h1.drop_p, h1.ln[4]) for L0, L1 in zip(*layers) for h0, h1 in zip(L0, L1)):      # one value per launch
        return None
    return layers


def _layer(lay):
    """The (self-attention, cross-attention, feed-forward) parameter handles (ops.SubLayer) of one DecoderLayer."""
    hs = (lay.slf_attn.handle(), lay.enc_attn.handle(cross=True), lay.pos_ffn.handle())
    assert all(lin.gw is not None for h in hs for lin in (h.inp, h.out)), "fused gradient buffers are not adjacent"
    return hs


class DecoderStagesFn(torch.autograd.Function):
    """(encoder_outputs, anchor parameter) -> (pred_l2r, pred_r2l), each (N, 16, 58).  `anchor` is any decoder
    parameter: it only makes the outputs require grad when the encoder is frozen."""

    @staticmethod
    def forward(ctx, enc_out, anchor, dec, layers, gold_l2r, gold_r2l, coins):
        """layers: what supported() returned."""
        call, segs, _p = ops.call, ops._segs, ops._p
        dev = enc_out.device
        N, T, D = enc_out.shape
        H, HD, F_, V = 8, 512, dec.layer_first_l2r.pos_ffn.w_1.weight.size(0), dec.tgt_word_emb.weight.size(0)
        ML = config.MAX_DECODE_LEN
        nl = dec.n_layers
        R = N * ML * (ML + 1) // 2
        rowoff = [N * t * (t + 1) // 2 for t in range(ML + 1)]                        # segment t = prefix length t+1
        ps_off = [H * N * sum((u + 1) ** 2 for u in range(t)) for t in range(ML + 1)]  # self-attention probabilities
        pe_off = [H * N * T * sum(u + 1 for u in range(t)) for t in range(ML + 1)]     # cross-attention probabilities
        enc2 = enc_out.contiguous().view(N * T, D)
        main = torch.cuda.current_stream(dev)
        side = ops.side_stream(dev) if dec.two_streams else None
        ops.set_main_stream(main)
        streams = (main, side if side is not None else main)
        st = ops.dropout_state(dev)
        training = dec.training
        p_emb = dec.dropout.p if training else 0.0

        # the last layer's "ends" layout: behind its self-attention core only positions 0 and L-1 of every sequence are computed
        # (module docstring); segment t keeps min(2, t+1) rows per sequence.  (The compact cross-attention is built on the
        # one-wavefront kernels: at most 32 key rows.)
        ends = bool(dec.last_layer_ends_only) and T <= 32
        crow = [len(_decoder.ends_rows(N, range(1, t + 1))) for t in range(ML + 1)]    # compact row offsets
        pec_off = [H * T * c for c in crow]                                            # compact cross-attention probabilities
        Rc = crow[ML]

        E = lambda *shape: ops._new(enc_out, *shape)      # noqa: E731
        # ---- all-stage buffers
        B_ = [[None] * nl for _ in (0, 1)]
        for d in (0, 1):
            for n in range(nl):
                e = ends and n == nl - 1
                Z, Zp = (Rc, pec_off[ML]) if e else (R, pe_off[ML])      # rows behind the self-attention core
                B_[d][n] = dict(x=E(R, D), qkv=E(R, 3 * HD), att=E(R, HD), ps=E(ps_off[ML]), o_s=E(Z, D), mu_s=E(Z), rs_s=E(Z), y_s=E(Z, D),
                                q=E(Z, HD), att2=E(Z, HD), pe=E(Zp), o_e=E(Z, D), mu_e=E(Z), rs_e=E(Z), y_e=E(Z, D),
                                h=E(Z, F_), o_f=E(Z, D), mu_f=E(Z), rs_f=E(Z), y_f=E(Z, D), kv=None,
                                off=[st.next_offset() for _ in range(5)] if training else [0] * 5)
                if e:
                    B_[d][n].update(x_c=E(Rc, D), att_c=E(Rc, HD))      # the end rows of x and att
        off_emb = [st.next_offset() if p_emb > 0 else 0 for _ in (0, 1)]
        last = [E(ML * N, D), E(ML * N, D)]
        pred = [E(ML * N, V), E(ML * N, V)]
        heads = (dec.tgt_word_prj_l2r.weight, dec.tgt_word_prj_r2l.weight)
        emb, pe_tab = dec.tgt_word_emb.weight, dec.positional_encoding.pe[0]
        # token buffers: <sos> followed by the teacher tokens of every step (decoder.py:176-186 feeds gold[:, i] when coin i says
        # so); the slots of the own-arg-max steps are overwritten by the stage tail before any later step reads them.  One
        # concatenation per direction instead of a fill, a column store and one select launch per teacher-forced step.
        sos_col = torch.full((N, 1), dec.sos_id, dtype=torch.long, device=dev)
        ys = [torch.cat([sos_col, golds_[:, :ML].to(torch.long)], 1).contiguous() for golds_ in (gold_l2r, gold_r2l)]
        seed = st.seed

        # ---- hoisted cross-attention K/V (attention.py:42-43 for every layer and direction; step-invariant).  The 12
        # [W_k; W_v] pairs are rows of ONE (12*1024, 512) matrix (supported()): one GEMM writes KV_all (N*T, 12*1024), layer
        # (d, n) reads its column block in place (row stride ldkv).
        kv_lin, kv_all, blocks = ops.project_kv_block(enc2, [l.enc_attn for d in (0, 1) for l in dec._layers(d)])
        ldkv = kv_lin.N
        for d in (0, 1):
            for n in range(nl):
                B_[d][n]["kv"] = blocks[d * nl + n]

        def layer_fwd(n, r0, r1, i0, segL):
            """Both directions of layer n in shared launches (same shapes, their own operands): kernel boundaries cost
            ~5 us each and small launches on two streams do not overlap, so the directions share launches, not streams."""
            b0, b1 = B_[0][n], B_[1][n]
            (s0, e0, f0), (s1, e1, f1) = layers[0][n], layers[1][n]
            M = r1 - r0
            seg_arr, nseg = segs(segL)
            sl = lambda b, k: b[k][r0:r1]
            sp = _p(seed) if training else None
            # self-attention sub-layer
            q0, q1 = sl(b0, "qkv"), sl(b1, "qkv")
            ops.gemm2(M, 3 * HD, D, sl(b0, "x"), sl(b1, "x"), D, s0.inp.w, s1.inp.w, D, q0, q1, 3 * HD, s0.inp.b, s1.inp.b)
            call("sbl_attention_seg2_fwd", _p(q0), _p(q1), 3 * HD, _p(q0[:, HD:]), _p(q1[:, HD:]), 3 * HD, _p(q0[:, 2 * HD:]), _p(q1[:, 2 * HD:]),
                 3 * HD, _p(sl(b0, "att")), _p(sl(b1, "att")), HD, b0["ps"].data_ptr() + 4 * ps_off[i0], b1["ps"].data_ptr() + 4 * ps_off[i0],
                 1 if n == 0 else 0, N, H, seg_arr, nseg, 0, 0.125, s0.drop_p, sp if s0.drop_p > 0 else None,
                 _fold(b0["off"][0], ps_off[i0]), _fold(b1["off"][0], ps_off[i0]), ops._s())
            # from here on the last layer runs on its end rows: one gather of att and of the residual x, both directions
            e = ends and n == nl - 1
            att_k, x_k = "att", "x"
            if e:
                c0, c1 = crow[i0], crow[i0 + nseg]
                M = c1 - c0
                call("sbl_ends_gather4", _p(sl(b0, "att")), _p(sl(b1, "att")), _p(sl(b0, "x")), _p(sl(b1, "x")), _p(b0["att_c"][c0:c1]),
                     _p(b1["att_c"][c0:c1]), _p(b0["x_c"][c0:c1]), _p(b1["x_c"][c0:c1]), N, seg_arr, nseg, D, ops._s())
                sl = lambda b, k: b[k][c0:c1]      # noqa: E731
                att_k, x_k = "att_c", "x_c"
            ops.gemm2(M, D, HD, sl(b0, att_k), sl(b1, att_k), HD, s0.out.w, s1.out.w, HD, sl(b0, "o_s"), sl(b1, "o_s"), D, s0.out.b, s1.out.b)

            def ln2(o, res, y, mu, rs, ln0, ln1, drop_p, k):
                # (masks are indexed by the full layout either way: the ends kernel maps its rows back, same folded offset)
                call("sbl_add_layernorm2_ends_fwd" if e else "sbl_add_layernorm2_fwd",
                     _p(sl(b0, o)), _p(sl(b1, o)), _p(sl(b0, res)), _p(sl(b1, res)), _p(ln0[0]), _p(ln1[0]),
                     _p(ln0[1]), _p(ln1[1]), _p(sl(b0, y)), _p(sl(b1, y)), _p(sl(b0, mu)), _p(sl(b1, mu)), _p(sl(b0, rs)), _p(sl(b1, rs)),
                     *((N, seg_arr, nseg) if e else (M,)), D, ln0[4], drop_p, sp if drop_p > 0 else None, _fold(b0["off"][k], r0 * D),
                     _fold(b1["off"][k], r0 * D), ops._s())

            ln2("o_s", x_k, "y_s", "mu_s", "rs_s", s0.ln, s1.ln, s0.drop_p, 1)
            # cross-attention sub-layer
            ops.gemm2(M, HD, D, sl(b0, "y_s"), sl(b1, "y_s"), D, e0.inp.w, e1.inp.w, D, sl(b0, "q"), sl(b1, "q"), HD, e0.inp.b, e1.inp.b)
            kv0, kv1 = b0["kv"], b1["kv"]
            if e:
                call("sbl_attention_ends2_fwd", _p(sl(b0, "q")), _p(sl(b1, "q")), HD, _p(kv0), _p(kv1), ldkv, _p(kv0[:, HD:]), _p(kv1[:, HD:]), ldkv,
                     _p(sl(b0, "att2")), _p(sl(b1, "att2")), HD, b0["pe"].data_ptr() + 4 * pec_off[i0], b1["pe"].data_ptr() + 4 * pec_off[i0],
                     N, H, seg_arr, nseg, T, 0.125, e0.drop_p, sp if e0.drop_p > 0 else None,
                     _fold(b0["off"][2], pe_off[i0]), _fold(b1["off"][2], pe_off[i0]), ops._s())
            else:
                call("sbl_attention_seg2_fwd", _p(sl(b0, "q")), _p(sl(b1, "q")), HD, _p(kv0), _p(kv1), ldkv, _p(kv0[:, HD:]), _p(kv1[:, HD:]), ldkv,
                     _p(sl(b0, "att2")), _p(sl(b1, "att2")), HD, b0["pe"].data_ptr() + 4 * pe_off[i0], b1["pe"].data_ptr() + 4 * pe_off[i0],
                     0, N, H, seg_arr, nseg, T, 0.125, e0.drop_p, sp if e0.drop_p > 0 else None,
                     _fold(b0["off"][2], pe_off[i0]), _fold(b1["off"][2], pe_off[i0]), ops._s())
            ops.gemm2(M, D, HD, sl(b0, "att2"), sl(b1, "att2"), HD, e0.out.w, e1.out.w, HD, sl(b0, "o_e"), sl(b1, "o_e"), D, e0.out.b, e1.out.b)
            ln2("o_e", "y_s", "y_e", "mu_e", "rs_e", e0.ln, e1.ln, e0.drop_p, 3)
            # position-wise feed-forward sub-layer
            ops.gemm2(M, F_, D, sl(b0, "y_e"), sl(b1, "y_e"), D, f0.inp.w, f1.inp.w, D, sl(b0, "h"), sl(b1, "h"), F_, f0.inp.b, f1.inp.b, relu=1)
            ops.gemm2(M, D, F_, sl(b0, "h"), sl(b1, "h"), F_, f0.out.w, f1.out.w, F_, sl(b0, "o_f"), sl(b1, "o_f"), D, f0.out.b, f1.out.b)
            if n + 1 < nl:
                # the sub-layer's LayerNorm and the cross-direction fusion that feeds layer n + 1, one launch; y_f is not stored
                nb0, nb1 = B_[0][n + 1]["x"][r0:r1], B_[1][n + 1]["x"][r0:r1]
                call("sbl_add_layernorm2_fusion_fwd", _p(sl(b0, "o_f")), _p(sl(b1, "o_f")), _p(sl(b0, "y_e")), _p(sl(b1, "y_e")),
                     _p(f0.ln[0]), _p(f1.ln[0]), _p(f0.ln[1]), _p(f1.ln[1]), _p(nb0), _p(nb1), _p(sl(b0, "mu_f")), _p(sl(b1, "mu_f")),
                     _p(sl(b0, "rs_f")), _p(sl(b1, "rs_f")), N, seg_arr, nseg, D, f0.ln[4], f0.drop_p, sp if f0.drop_p > 0 else None,
                     _fold(b0["off"][4], r0 * D), _fold(b1["off"][4], r0 * D), ops._s())
            else:
                # (the last fusion is only ever read at the last positions: stage tail, which is why this layer ran on its end rows)
                ln2("o_f", "y_e", "y_f", "mu_f", "rs_f", f0.ln, f1.ln, f0.drop_p, 4)

        for (i0, i1) in _decoder.stages_of(coins, ML):
            segL = tuple(range(i0 + 1, i1 + 2))
            seg_arr, nseg = segs(segL)
            r0, r1 = rowoff[i0], rowoff[i1 + 1]
            # stage head: embedding + PE + dropout of both directions in one launch (the pre-dropout embeddings are not
            # needed afterwards: backward regenerates the mask)
            call("sbl_embed_pe_drop2_fwd", _p(ys[0]), _p(ys[1]), ys[0].stride(0), _p(emb), _p(pe_tab), _p(B_[0][0]["x"][r0:r1]),
                 _p(B_[1][0]["x"][r0:r1]), N, seg_arr, nseg, D, V, p_emb, _p(seed) if p_emb > 0 else None,
                 _fold(off_emb[0], r0 * D), _fold(off_emb[1], r0 * D), ops._s())
            for n in range(nl):
                layer_fwd(n, r0, r1, i0, segL)
            # stage tail: last fusion at the last positions + both heads + the token fed to the next stage, one launch
            lrows = slice(i0 * N, (i1 + 1) * N)
            if ends:      # the compact y_f IS a ragged batch of min(2, L)-row sequences whose first / last rows the tail wants
                seg_arr, nseg = segs(tuple(min(2, L) for L in segL))
                r0, r1 = crow[i0], crow[i1 + 1]
            call("sbl_decoder_tail_fwd", _p(B_[0][nl - 1]["y_f"][r0:r1]), _p(B_[1][nl - 1]["y_f"][r0:r1]), _p(heads[0]), _p(heads[1]),
                 _p(last[0][lrows]), _p(last[1][lrows]), _p(pred[0][lrows]), _p(pred[1][lrows]), V, _p(ys[0]), _p(ys[1]),
                 ys[0].stride(0), i1, int(bool(coins[i1])), N, seg_arr, nseg, D, V, ops._s())

        ctx.state = dict(N=N, T=T, D=D, HD=HD, V=V, ML=ML, nl=nl, R=R, layers=layers, B=B_, last=last, ys=ys,
                         heads=heads, g_heads=(ops._gbuf(heads[0]), ops._gbuf(heads[1])), g_emb=ops._gbuf(emb), seed=seed,
                         p_emb=p_emb, off_emb=off_emb, streams=streams, two=side is not None, enc2=enc2, training=training,
                         kv_lin=kv_lin, ends=ends, Rc=Rc)
        ctx.set_materialize_grads(False)
        dec.last_ys = ys
        # (ML*N, V) step-major -> (N, ML, V) views
        return pred[0].view(ML, N, V).transpose(0, 1), pred[1].view(ML, N, V).transpose(0, 1)

    @staticmethod
    @ops._bw
    def backward(ctx, dpl, dpr):
        S = ctx.state
        call, gemm, segs, _p = ops.call, ops.gemm, ops._segs, ops._p
        N, T, D, HD, V, ML, nl, R = (S[k] for k in ("N", "T", "D", "HD", "V", "ML", "nl", "R"))
        layers, B_, streams, ends, Rc = S["layers"], S["B"], S["streams"], S["ends"], S["Rc"]
        main, side = streams[0], (streams[1] if S["two"] else None)
        dev = S["enc2"].device
        seed = S["seed"]
        segL = tuple(range(1, ML + 1))
        seg_arr, nseg = segs(segL)
        ldkv = S["kv_lin"].N

        E = lambda *shape: ops._new(S["enc2"], *shape)      # noqa: E731
        wg = {}           # deferred weight gradients by row count: (C, ldc, colsum, [A], lda, [B], ldb, M, N), see ops.wgrad_group

        def dW(lin, dY, X):      # the weight-gradient sink of ops.attn_bwd / ops.ffn_bwd
            wg.setdefault(X.size(0), []).append((lin.gw, lin.K, lin.gb, [dY], lin.N, [X], lin.K, lin.N, lin.K))

        if side is not None:
            side.wait_stream(main)
        # ---- heads and the gather of the last positions
        dx, dlasts = [None, None], [None, None]
        for d, dp in ((0, dpl), (1, dpr)):
            with torch.cuda.stream(streams[d]):
                if dp is None:
                    if not ends:
                        dx[d] = torch.zeros(R, D, device=dev, dtype=torch.float32)
                    continue
                dpred = dp.transpose(0, 1).contiguous().view(ML * N, V)
                dlast = dlasts[d] = E(ML * N, D)
                gemm(0, 0, ML * N, D, V, dpred, V, S["heads"][d], D, dlast, D)
                gemm(1, 0, V, D, ML * N, dpred, V, S["last"][d], D, S["g_heads"][d], D, accumulate=1)
                if not ends:      # (ends: the tail adjoint below goes from dlast straight to the compact rows)
                    dx[d] = E(R, D)
                    call("sbl_gather_last_bwd", _p(dlast), _p(dx[d]), N, seg_arr, nseg, D, ops._s())

        def layer_bwd(d, n, dy):
            """The sub-layers' adjoints over the rows of all steps, with the forward's offsets; always a separate pre-dropout
            gradient (the grouped launch below reads it after the input gradient has been accumulated into dz)."""
            (slf, enc, ffn), b = layers[d][n], B_[d][n]
            off = b["off"]
            if ends and n == nl - 1:
                # compact rows down to the self-attention's out-projection, then its two results go back to their end rows of
                # full-size buffers (zero elsewhere) for the core, which needs every key and value row
                en = (N, segL)
                dy = ops.ffn_bwd(ffn, dy, b["y_e"], (b["h"], b["o_f"], b["mu_f"], b["rs_f"]), seed, off[4], True, dW, ends=en)
                dy, _ = ops.attn_bwd(enc, dy, b["y_s"], (b["q"], b["att2"], b["pe"], b["o_e"], b["mu_e"], b["rs_e"]), N, segL, b["kv"],
                                     seed, off[2], off[3], True, dW, dkv=dkv_blocks[d * nl + n], ends=True)
                dz_c, datt_c = ops._out_ln_bwd(slf, dy, b["att_c"], b["o_s"], b["x_c"], b["mu_s"], b["rs_s"], seed, off[1], True, dW, ends=en)
                dz, datt = E(R, D), E(R, HD)
                call("sbl_ends_scatter2", _p(dz_c), _p(datt_c), _p(dz), _p(datt), N, seg_arr, nseg, D, ops._s())
                return ops.attn_core_bwd(slf, dz, datt, b["x"], b["qkv"], b["ps"], N, segL, None, seed, off[0], dW)[0]
            dy = ops.ffn_bwd(ffn, dy, b["y_e"], (b["h"], b["o_f"], b["mu_f"], b["rs_f"]), seed, off[4], True, dW)
            dy, _ = ops.attn_bwd(enc, dy, b["y_s"], (b["q"], b["att2"], b["pe"], b["o_e"], b["mu_e"], b["rs_e"]), N, segL, b["kv"],
                                 seed, off[2], off[3], True, dW, dkv=dkv_blocks[d * nl + n])
            dy, _ = ops.attn_bwd(slf, dy, b["x"], (b["qkv"], b["att"], b["ps"], b["o_s"], b["mu_s"], b["rs_s"]), N, segL, None,
                                 seed, off[0], off[1], True, dW)
            return dy

        # gradient of the hoisted K/V: column block (direction, layer) of one (N*T, 12*1024) buffer, so that its input gradient
        # is ONE product over K = 12*1024 below
        dkv_all = E(N * T, ldkv)
        dkv_blocks = dkv_all.split(2 * HD, 1)
        for n in range(nl - 1, -1, -1):
            if side is not None:
                main.wait_stream(side)
            if ends and n == nl - 1:
                dy = [E(Rc, D), E(Rc, D)]
                call("sbl_ends_tail_bwd", _p(dlasts[0]), _p(dlasts[1]), _p(dy[0]), _p(dy[1]), N, seg_arr, nseg, D, ops._s())
                if side is not None and dlasts[1] is not None:
                    dlasts[1].record_stream(main)
            else:
                dy = [E(R, D), E(R, D)]
                call("sbl_fusion_seg_bwd", _p(dx[0]), _p(dx[1]), _p(dy[0]), _p(dy[1]), N, seg_arr, nseg, D, ops._s())
            if side is not None:
                side.wait_stream(main)
            for d in (0, 1):
                with torch.cuda.stream(streams[d]):
                    dx[d] = layer_bwd(d, n, dy[d])
        # ---- embeddings (shared table: float atomics) and the hoisted K/V projections
        denc = E(N * T, D)
        for d in (0, 1):
            with torch.cuda.stream(streams[d]):
                g = dx[d]
                if S["p_emb"] > 0:
                    g2 = E(R, D)
                    call("sbl_dropout", _p(g), _p(g2), R * D, S["p_emb"], _p(seed), S["off_emb"][d], ops._s())
                    g = g2
                call("sbl_embed_seg_bwd", _p(S["ys"][d]), S["ys"][d].stride(0), _p(g), _p(S["g_emb"]), N, seg_arr, nseg, D, V, ops._s())
        if side is not None:
            main.wait_stream(side)
        # dEnc = [dKV_0 | ... | dKV_11] (N*T, 12*1024) x [Wkv_0; ...; Wkv_11] (12*1024, 512): ONE product instead of 12
        # launches plus the adds of their partial results; its weight gradient is one (12*1024, 512) problem too
        gemm(0, 0, N * T, D, ldkv, dkv_all, ldkv, S["kv_lin"].w, D, denc, D)
        dW(S["kv_lin"], dkv_all, S["enc2"])
        # ---- every weight gradient of the decoder: one grouped launch over the R rows of all steps (and the K/V problem over
        # its N*T rows) on the side stream, issued right here: it then runs beside the encoder backward, a dependent chain of
        # 928-row products that cannot fill the chip.  (Issuing it after backward has passed the encoder measured slower for the
        # whole step, 31.95 against 31.46 ms in a same-box A/B: the encoder's own launches get 2-3x faster without 2688 tiles
        # beside them, but the chip idles under them and the grouped launch then competes with the throughput-bound frontend
        # backward.  Capping its grid to 128 / 192 workgroups, 33.69 / 32.01 ms.)
        run = side if side is not None else main
        if run is not main:
            run.wait_stream(main)
        with torch.cuda.stream(run):
            for rows, problems in wg.items():
                ops.wgrad_group(problems, (rows,), run, ops._wgrad_splitk)
        if run is not main:
            # nothing downstream reads these gradients before the step ends (dp.GradientExchange.launch waits for the side
            # stream itself): join at the end of backward instead of stalling the main stream for the 4.5 ms grouped launch
            # (a kernel trace showed the encoder backward waiting for it)
            ops._arm_side_join()
        ctx.state = None
        return denc.view(N, T, D), None, None, None, None, None, None

