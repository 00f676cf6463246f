"""Decoder (the SBL bidirectional decoder) and DecoderLayer with the constructor / forward signatures and state-dict
keys of the reference's transformer/decoder.py."""
import collections
import random

import torch
import torch.nn as nn

from ._env import _lib, config, ops
from . import decoder_stages
from .attention import MultiHeadAttention
from .module import PositionalEncoding, PositionwiseFeedForward, mask_rows
from .utils import device_lengths

IGNORE_ID = config.IGNORE_ID
MAX_PAIR_BEAM = 16          # slots per clip of Decoder.beam_search (csrc/pair_beam.hip)

PairBeamResult = collections.namedtuple("PairBeamResult", ("ys_l2r", "ys_r2l", "scores", "scores_dir", "history"))
PairScore = collections.namedtuple("PairScore", ("score", "score_dir", "logp", "best"))
WordResult = collections.namedtuple("WordResult", ("word", "cand", "cand_dist", "cand_hyp", "score", "score_dir"))
PairWordBeamResult = collections.namedtuple("PairWordBeamResult", ("word", "cand", "score", "score_dir", "ys_l2r", "ys_r2l", "history"))
SCORE_PAIRS_MAX_ROWS = 1 << 16      # rows of one score_pairs stage (136 per slot): 128 MiB of activations per 512 columns


def stages_of(coins, maxlen):
    """(first step, last step) of every stage: a stage is a maximal run of steps whose input tokens are known when it
    starts, i.e. it ends with the first step whose coin says "feed back the own argmax" (or with the last step)."""
    stages, i = [], 0
    while i < maxlen:
        j = i
        while j < maxlen - 1 and not coins[j]:
            j += 1
        stages.append((i, j))
        i = j + 1
    return stages


def ends_rows(n_seq, seg_lens, row0=0):
    """Compact-to-full row map of the last decoder layer's "ends" layout (decoder_stages.py): for the ragged batch whose
    segment s holds n_seq sequences of length seg_lens[s] (full rows from row0 on, (b, l) order) the full row of every compact
    row.  Segment s keeps min(2, L) rows per sequence in (b, k) order: k = 0 is position 0, k = 1 is position L-1 - the two
    rows the heads read after the last fusion - and the L = 1 row is both."""
    rows = []
    for L in seg_lens:
        for b in range(n_seq):
            rows.extend(row0 + b * L + k * (L - 1) for k in range(min(2, L)))
        row0 += n_seq * L
    return rows


class Decoder(nn.Module):
    ''' Two n_layers-deep decoders, left-to-right and right-to-left, that attend to the same encoder output and swap
    information after every layer; 16 greedy / teacher-forced steps each (decoder.py:16-191, 301-385).

    Same constructor / forward / recognize_beam signatures and state-dict keys as the reference.  What differs
    is how the same numbers are produced:
      * the cross-attention K/V projections of the encoder output are computed once per layer per forward, not
        once per step (step-invariant; exact algebra);
      * the aliased in-place fusion loops are one kernel, A' = A + flip(B), B' = 2B + flip(A);
      * tokens, argmax and the teacher-forcing select stay on the device (no host sync in the 16-step loop);
      * the coins are still `random.random() > 0.5`, 16 draws in the reference's order (so `random.seed(k)`
        reproduces its choices), but they are drawn up front: step i+1 depends on step i only when coin i says
        "feed back the own argmax" (decoder.py:176-186).  A run of steps whose inputs are all teacher-forced is
        therefore processed as ONE ragged batch (rows of all its prefixes concatenated; weights are shared by the
        steps), which turns 16 sequential stages into 1 + (#own-argmax coins) ~ 8.5 on average.  The per-step
        results are identical: every row-wise op is unchanged and attention / fusion / embedding work per segment.
        `batch_teacher_runs = False` restores the one-stage-per-step schedule (also used by greedy inference,
        where every coin is "own argmax").
    A training forward takes one of two paths that compute the same numbers.  With persistent gradient buffers
    (dp.FlatModel) and host coins, the 16 steps are ONE autograd node with a single fixed launch sequence and a backward
    batched over all steps (decoder_stages.py; its supported() lists the conditions).  Otherwise, and for inference, `_run`
    builds the per-stage tape of ops.* Functions.
    Set `self.coins_dev` to a device int32[16] tensor to take the coins from device memory (one captured hipGraph
    for every coin pattern; implies the per-step schedule), or `self.coins_host` to a list of 16 bools to fix them.
    '''

    def __init__(
            self, sos_id, eos_id,
            n_tgt_vocab, d_word_vec,
            n_layers, n_head, d_k, d_v,
            d_model, d_inner, dropout=0.1,
            tgt_emb_prj_weight_sharing=True,
            pe_maxlen=5000):
        super(Decoder, self).__init__()
        self.sos_id = sos_id
        self.eos_id = eos_id
        self.n_tgt_vocab = n_tgt_vocab
        self.d_word_vec = d_word_vec
        self.n_layers = n_layers
        self.n_head = n_head
        self.d_k = d_k
        self.d_v = d_v
        self.d_model = d_model
        self.d_inner = d_inner
        self.tgt_emb_prj_weight_sharing = tgt_emb_prj_weight_sharing   # stored, ignored (decoder.py:40)
        self.pe_maxlen = pe_maxlen

        self.tgt_word_emb = nn.Embedding(n_tgt_vocab, d_word_vec)
        self.positional_encoding = PositionalEncoding(d_model, max_len=pe_maxlen)
        self.dropout = nn.Dropout(dropout)

        def direction():        # one direction's layers: the first one, then the remaining n_layers - 1
            layer = lambda: DecoderLayer(d_model, d_inner, n_head, d_k, d_v, dropout)      # noqa: E731
            return layer(), nn.ModuleList(layer() for _ in range(n_layers - 1))

        self.layer_first_l2r, self.layer_stack_l2r = direction()
        self.layer_first_r2l, self.layer_stack_r2l = direction()

        self.x_logit_scale = 1.0
        # output heads: 512 features -> 58 classes (56 tokens, <sos>, <eos>), fixed sizes as in decoder.py:59-60
        self.tgt_word_prj_l2r = nn.Linear(512, 58, bias=False)
        self.tgt_word_prj_r2l = nn.Linear(512, 58, bias=False)

        self.batched_backward = True     # one stage-batched backward over all 16 steps (decoder_stages.py) when possible
        self.last_layer_ends_only = True # the last layer computes, behind its self-attention, only the two rows per sequence the heads read
        self.two_streams = True          # run the two directions' layers on two HIP streams (joined before each fusion)
        self.batch_teacher_runs = True   # batch the steps of a teacher-forced run (see class docstring)
        self.coins_dev = None            # optional device int32[16]: 1 = feed own argmax (graph replay, per-step schedule)
        self.coins_host = None           # optional list of 16 bools overriding the python `random` draws
        self.last_coins = None           # the coins of the last forward (host list), for inspection / parity tests

    def preprocess(self, padded_input):
        """Generate decoder input and output label from padded_input (decoder.py:62-77): strip IGNORE_ID,
        add <sos> / <eos>, pad both to 16 with *eos*.  Vectorised on the input's device, no host sync."""
        N, To = padded_input.shape
        maxlen = config.MAX_DECODE_LEN
        if padded_input.is_cuda:
            return self._preprocess_device(padded_input)
        valid = padded_input.ne(IGNORE_ID)
        # stable compaction of the valid ids to the left (the reference's y[y != IGNORE_ID])
        order = torch.argsort((~valid).to(torch.int8), dim=1, stable=True)
        comp = torch.gather(padded_input, 1, order)
        n_valid = valid.sum(1, keepdim=True)
        pos = torch.arange(To, device=padded_input.device).unsqueeze(0)
        comp = torch.where(pos < n_valid, comp, torch.full_like(comp, self.eos_id))
        ys_in = padded_input.new_full((N, maxlen), self.eos_id)
        ys_out = padded_input.new_full((N, maxlen), self.eos_id)
        ys_in[:, 0] = self.sos_id
        w = min(To, maxlen - 1)
        ys_in[:, 1:1 + w] = comp[:, :w]
        ys_out[:, :min(To, maxlen)] = comp[:, :maxlen]
        return ys_in, ys_out

    def _preprocess_device(self, a, b=None):
        """preprocess on the GPU: one launch of sbl_decoder_preprocess for one target tensor or for both directions (instead
        of ~20 torch launches each).  Returns (ys_in, ys_out) or (ys_in_a, ys_out_a, ys_in_b, ys_out_b)."""
        maxlen = config.MAX_DECODE_LEN
        a = a.contiguous().long()
        N, To = a.shape
        outs = [a.new_empty((N, maxlen)) for _ in range(4 if b is not None else 2)]
        if b is not None:
            b = b.contiguous().long()
            assert b.shape == a.shape
        ops.call("sbl_decoder_preprocess", a.data_ptr(), b.data_ptr() if b is not None else None, outs[0].data_ptr(),
                 outs[1].data_ptr(), outs[2].data_ptr() if b is not None else None, outs[3].data_ptr() if b is not None else None,
                 N, To, maxlen, self.sos_id, self.eos_id, IGNORE_ID, torch.cuda.current_stream(a.device).cuda_stream)
        return tuple(outs)

    def _layers(self, direction):
        first = self.layer_first_l2r if direction == 0 else self.layer_first_r2l
        stack = self.layer_stack_l2r if direction == 0 else self.layer_stack_r2l
        return [first] + list(stack)

    def _draw_coins(self, teacher_mode):
        """The coins of one forward, True = feed back the own argmax after that step (kept in last_coins): all True for
        greedy inference; None when they live on the device (coins_dev); coins_host if set; else one draw per step in the
        order of decoder.py:176."""
        if not teacher_mode:
            coins = [True] * config.MAX_DECODE_LEN
        elif self.coins_dev is not None:
            coins = None
        elif self.coins_host is not None:
            coins = [bool(c) for c in self.coins_host]
        else:
            coins = [random.random() > config.TEACHER_COIN_THRESHOLD for _ in range(config.MAX_DECODE_LEN)]
        self.last_coins = coins
        return coins

    def _begin(self, encoder_outputs):
        """What every decode loop starts with -> (layers[direction], main stream, side stream or None, kv[direction][layer]):
        the parameters fused, the two streams, and the hoisted cross-attention K/V of the encoder output."""
        dev = encoder_outputs.device
        layers = (self._layers(0), self._layers(1))
        for d in (0, 1):            # parameter fusing (first call only) happens here, on the caller's stream
            for lay in layers[d]:
                lay.slf_attn._fuse()
                lay.enc_attn._fuse()
        side = main = None
        if self.two_streams and dev.type == "cuda":
            main = torch.cuda.current_stream(dev)
            side = ops.side_stream(dev)
            ops.set_main_stream(main)
        # hoisted cross-attention K/V (one GEMM per layer per direction per forward).  The r2l projections are made on
        # the side stream: autograd accumulates the per-stage K/V gradients on the stream of the node that consumes
        # them, so a main-stream node here would make every main-stream backward step wait for the side stream.
        kv = [[lay.enc_attn.project_kv(encoder_outputs) for lay in layers[0]], None]
        if side is None:
            kv[1] = [lay.enc_attn.project_kv(encoder_outputs) for lay in layers[1]]
        else:
            side.wait_stream(main)
            with torch.cuda.stream(side):
                kv[1] = [lay.enc_attn.project_kv(encoder_outputs) for lay in layers[1]]
        return layers, main, side, kv

    _kv_len = staticmethod(device_lengths)

    def _stage(self, ys, B, segL, layers, main, side, kv, kv_group=None, kv_len=None):
        """One stage on B sequences per segment: embedding + PE of the token tables ys[direction], the n_layers layers of
        both directions with the fusion after each -> x[direction], the rows (B * sum(segL), d_model) behind the last
        fusion.  kv_group = W: kv belongs to B / W clips whose W beam slots share it (DecoderLayer.forward_rows).
        kv_len: the clips' frame counts (`_kv_len`), the keys of every cross-attention."""
        emb = self.tgt_word_emb.weight
        pe = self.positional_encoding.pe[0]
        x = [ops.dropout(ops.EmbedPEFn.apply(ys[d], B, segL, emb, pe), self.dropout.p, self.training) for d in (0, 1)]
        for n in range(self.n_layers):
            slf_mask = 'causal' if n == 0 else None       # decoder.py:123-125 vs :150,:157
            if side is None:
                for d in (0, 1):
                    x[d] = layers[d][n].forward_rows(x[d], B, segL, slf_mask, kv[d][n], kv_group, kv_len)
            else:
                # the l2r and r2l layers are independent until the fusion: run them on two HIP streams so their
                # small kernels overlap on the 256 CUs (fork / join is captured as parallel hipGraph branches;
                # autograd replays backward on the same two streams)
                side.wait_stream(main)
                x[0] = layers[0][n].forward_rows(x[0], B, segL, slf_mask, kv[0][n], kv_group, kv_len)
                with torch.cuda.stream(side):
                    x[1] = layers[1][n].forward_rows(x[1], B, segL, slf_mask, kv[1][n], kv_group, kv_len)
                main.wait_stream(side)
            x[0], x[1] = ops.FusionFn.apply(x[0], x[1], B, segL)
        return x

    def _stage_last(self, ys, B, segL, layers, main, side, kv, kv_group=None, kv_len=None):
        """`_stage`, then position -1 of every prefix: per direction the (len(segL) * B, d_model) rows the heads read."""
        x = self._stage(ys, B, segL, layers, main, side, kv, kv_group, kv_len)
        return [ops.GatherLastFn.apply(x[d], B, segL) for d in (0, 1)]

    def _run(self, encoder_outputs, gold_l2r, gold_r2l, teacher_mode, kv_len=None):
        """The 16 decoding steps shared by forward (decoder.py:106-186) and recognize_beam (:310-383).  kv_len (inference
        only): the clips' frame counts (`_stage`)."""
        maxlen = config.MAX_DECODE_LEN
        N = encoder_outputs.size(0)
        dev = encoder_outputs.device
        layers, main, side, kv = self._begin(encoder_outputs)
        ys = [torch.full((N, maxlen + 1), self.eos_id, dtype=torch.long, device=dev) for _ in (0, 1)]
        for y in ys:
            y[:, 0] = self.sos_id
        heads = (self.tgt_word_prj_l2r.weight, self.tgt_word_prj_r2l.weight)
        golds = (gold_l2r, gold_r2l)
        outs = ([None] * maxlen, [None] * maxlen)

        coins = self._draw_coins(teacher_mode)
        if coins is None or not self.batch_teacher_runs:
            stages = [(i, i) for i in range(maxlen)]
        else:
            stages = stages_of(coins, maxlen)
            for k in range(maxlen):              # teacher-forced tokens are known up front
                if not coins[k]:
                    for d in (0, 1):
                        ops.argmax_select(None, golds[d], ys[d], k, 0)

        if encoder_outputs.requires_grad and torch.is_grad_enabled():
            # d(loss)/d(encoder_outputs) is complete only after every decoder tape node has run: issue the merged
            # weight-gradient GEMMs then (side stream), beside the encoder / frontend backward.  (Flushing when backward
            # reaches the encoder INPUT instead measured equal within noise: the chip is throughput-bound either way.)
            encoder_outputs.register_hook(lambda g: ops.flush_deferred())
        with ops.deferring():      # decoder weights are used once per stage: their dW GEMMs are deferred and merged
            for (i0, i1) in stages:
                segL = tuple(range(i0 + 1, i1 + 2))            # prefix lengths of the steps in this stage
                last = self._stage_last(ys, N, segL, layers, main, side, kv, kv_len=kv_len)     # (nseg*N, 512) per direction
                for d in (0, 1):
                    pred = ops.linear(last[d], heads[d])                   # (nseg*N, 58)
                    # unbind (one stack in backward) instead of row slices (a zero-filled (nseg*N, 58) buffer, a copy and
                    # an add per step in backward)
                    for step, pr in zip(range(i0, i1 + 1), pred.view(len(segL), N, -1).unbind(0)):
                        outs[d][step] = pr
                # token fed to the next stage
                if coins is None:
                    for d in (0, 1):
                        ops.argmax_select(outs[d][i1].detach(), golds[d], ys[d], i1, 0, self.coins_dev)
                elif coins[i1]:
                    for d in (0, 1):
                        ops.argmax_select(outs[d][i1].detach(), golds[d], ys[d], i1, 1)
                elif not self.batch_teacher_runs:
                    for d in (0, 1):
                        ops.argmax_select(outs[d][i1].detach(), golds[d], ys[d], i1, 0)
        return outs, ys

    def forward(self, padded_input_l2r, padded_input_r2l, encoder_outputs,
                encoder_input_lengths, return_attns=False):
        """padded_input_l2r / _r2l (N, To) IGNORE_ID-padded targets, encoder_outputs (N, Ti, d_model).
        Returns (pred_l2r (N,16,58), gold_l2r (N,16), pred_r2l, gold_r2l)."""
        dev = encoder_outputs.device
        if dev.type == "cuda" and padded_input_l2r.shape == padded_input_r2l.shape:
            ys_in_pad_l2r, ys_out_pad_l2r, ys_in_pad_r2l, ys_out_pad_r2l = self._preprocess_device(
                padded_input_l2r.to(dev), padded_input_r2l.to(dev))
        else:
            ys_in_pad_l2r, ys_out_pad_l2r = self.preprocess(padded_input_l2r.to(dev))
            ys_in_pad_r2l, ys_out_pad_r2l = self.preprocess(padded_input_r2l.to(dev))
        layers = decoder_stages.supported(self, encoder_outputs)
        if layers is not None:
            pl, pr = decoder_stages.DecoderStagesFn.apply(encoder_outputs, self.tgt_word_emb.weight, self, layers, ys_out_pad_l2r,
                                                          ys_out_pad_r2l, self._draw_coins(True))
            return pl, ys_out_pad_l2r, pr, ys_out_pad_r2l
        outs, _ = self._run(encoder_outputs, ys_out_pad_l2r, ys_out_pad_r2l, teacher_mode=True)
        return torch.stack(outs[0], 1), ys_out_pad_l2r, torch.stack(outs[1], 1), ys_out_pad_r2l

    def recognize_beam(self, encoder_outputs, encoder_input_lengths=None):
        """Greedy decode, always own argmax (decoder.py:301-385).  Returns (ys_l2r, ys_r2l) (N,17) int64.
        encoder_input_lengths (here and in every decode method below): None, or the clips' frame counts - N ints or a device
        int32 (N,) tensor, which is never read on the host.  Clip n then attends to the encoder rows t < lengths[n] only, so
        whatever the rows behind hold does not matter and the clip decodes as it would alone at its length."""
        with torch.no_grad():
            _, ys = self._run(encoder_outputs, None, None, teacher_mode=False,
                              kv_len=self._kv_len(encoder_input_lengths, encoder_outputs))
        return ys[0], ys[1]

    def beam_search(self, encoder_outputs, beam_size, nbest=1, encoder_input_lengths=None):
        """Beam search over PAIRS of an l2r and an r2l prefix - the search that recognize_beam's name and the reference's
        beam_size / nbest arguments promise (decoder.py:301-385 is greedy).  A pair is fused exactly as row b of the two
        directions is in `_run`; every clip keeps W = beam_size pairs, the batch is S = N * W rows, and because the upper
        layers are not causal and the fusion flips positions the whole prefix is recomputed at every step with `_run`'s own
        kernels (no KV cache).  After the stage of step i the tail kernel (ops.pair_beam_tail) adds, for every live slot s and
        every (a, b) in V x V, score[s] + (log_softmax(head_l2r)[a] + log_softmax(head_r2l)[b]) in fp32 and keeps the clip's
        best W in descending total (ties: lower parent slot, then lower rank of a in (log-prob descending, token ascending)
        order, then lower rank of b).  Nothing ends early and there is no length penalty: all 16 positions are decoded, as
        the model is trained (<eos> is fed and predicted behind the end), so the totals are sequence log-likelihoods and
        the slots after step 15 are the n-best list in order.  beam_size = 1 is the greedy decode token for token.
        The cross-attention K/V are hoisted once for the N clips and shared by a clip's W slots
        (sbl_attention_seg_grouped_fwd); two streams as in `_run`; module mode is used as recognize_beam uses it; no host
        read, so the call is capturable as one hipGraph.
        Returns PairBeamResult(ys_l2r, ys_r2l (N, nbest, 17) int64, scores (N, nbest), scores_dir (N, nbest, 2), history =
        (l2r token, r2l token, parent rank, total score), each (N, 16, W) at [n][step][rank])."""
        enc = encoder_outputs
        W, nbest = self._search_args("Decoder.beam_search", enc, beam_size, nbest)
        with torch.no_grad():
            kv_len = self._kv_len(encoder_input_lengths, enc)
            st = self._beam_steps(enc, W, config.MAX_DECODE_LEN, kv_len, ops.pair_beam_tail)
        N, L = enc.size(0), config.MAX_DECODE_LEN + 1
        ys_l, ys_r = (y.view(N, W, L)[:, :nbest] for y in st.prefixes(config.MAX_DECODE_LEN))
        return PairBeamResult(ys_l, ys_r, st.score[:, :nbest], st.score_dir[:, :nbest], st.history())

    @staticmethod
    def _search_args(who, enc, beam_size, nbest):
        """(W, nbest) of a pair beam search as ints, after the refusals both searches share (`who`: the method, for the message)."""
        W, nbest = int(beam_size), int(nbest)
        if not 1 <= W <= MAX_PAIR_BEAM:
            raise _lib.SblHipError("%s: beam_size = %d outside 1..%d" % (who, W, MAX_PAIR_BEAM))
        if not 1 <= nbest <= W:
            raise _lib.SblHipError("%s: nbest = %d outside 1..beam_size = %d" % (who, nbest, W))
        Decoder._need_gpu(who, enc)
        return W, nbest

    @staticmethod
    def _need_gpu(who, enc):
        if not enc.is_cuda:
            raise _lib.SblHipError("%s needs the encoder output on the GPU (got a %s tensor); there is no CPU path" % (who, enc.device))

    def _check_lexicon(self, who, lexicon):
        if lexicon.vocab > self.n_tgt_vocab or (lexicon.sos_id, lexicon.eos_id) != (self.sos_id, self.eos_id):
            raise _lib.SblHipError("%s: the lexicon (vocab %d, sos %d, eos %d) is not this decoder's (%d, %d, %d)"
                                   % (who, lexicon.vocab, lexicon.sos_id, lexicon.eos_id, self.n_tgt_vocab, self.sos_id, self.eos_id))

    def _beam_steps(self, enc, W, steps, kv_len, tail, lex=False):
        """The step loop of beam_search and beam_search_lex -> the final ops.PairBeamState (lex: with node buffers), on the
        17-entry prefix rows the stage reads.  The stage is `_run`'s, at batch N * W; tail(last_l, last_r, head_l, head_r, st, i)
        ends step i."""
        N = enc.size(0)
        layers, main, side, kv = self._begin(enc)
        st = ops.PairBeamState(N, W, steps, self.sos_id, self.eos_id, enc.device, lex=lex, row_len=config.MAX_DECODE_LEN + 1)
        heads = (self.tgt_word_prj_l2r.weight, self.tgt_word_prj_r2l.weight)
        for i in range(steps):
            last = self._stage_last(st.prefixes(i), N * W, (i + 1,), layers, main, side, kv, kv_group=W, kv_len=kv_len)
            tail(last[0], last[1], heads[0], heads[1], st, i)
        return st

    def score_pairs(self, encoder_outputs, ys_l2r, ys_r2l, n_pos=None, group=1, encoder_input_lengths=None):
        """Pair scores of S given token rows (include/sbl_hip.h, sbl_pair_score_tail): with lpL_i / lpR_i the two heads'
        log-softmax at the last position of prefix length i + 1 of slot s - the pair fused exactly as `_run` and beam_search
        fuse it - taken at ys_l2r[s][i+1] / ys_r2l[s][i+1]: logp[s, i] = (lpL_i, lpR_i) for i < n_pos[s], else 0; score_dir
        their sums; score[s] = the sum of (lpL_i + lpR_i), both in ascending i in fp32 (the order of the beam search's totals:
        with n_pos = 16 on beam_search's rows it is that search's score).  No length penalty, no prior.
        ys_l2r / ys_r2l: int64 (S, 17) (or (N, group, 17)); encoder_outputs holds S / group clips and slot s belongs to clip
        s // group; n_pos: None (16 positions) or int32 (S,).  All 16 prefixes of every slot go through ONE ragged stage
        (segL = 1..16, 136 rows per slot and direction; cross-attention K/V shared by a clip's slots), then GatherLastFn, then
        the tail kernel; beyond SCORE_PAIRS_MAX_ROWS rows the clips are taken in chunks of whole clips (the last one may be
        shorter), whose size depends on the shapes alone.  Module mode is used as recognize_beam uses it; no host read, so the call is capturable as one hipGraph.
        Returns PairScore(score (S,), score_dir (S, 2), logp (S, 16, 2), best (S / group,) int32 = the rank of the largest
        score in every group, the lower rank on an exact tie)."""
        enc = encoder_outputs
        G = int(group)
        self._need_gpu("Decoder.score_pairs", enc)
        maxlen = config.MAX_DECODE_LEN
        ys = [y.reshape(-1, maxlen + 1).contiguous() for y in (ys_l2r, ys_r2l)]
        S, N = ys[0].size(0), enc.size(0)
        if not 1 <= G <= MAX_PAIR_BEAM or S != N * G or ys[1].size(0) != S:
            raise _lib.SblHipError("Decoder.score_pairs: %d and %d token rows for %d clips in groups of %d (1..%d)"
                                   % (S, ys[1].size(0), N, G, MAX_PAIR_BEAM))
        dev = enc.device
        kv_len = self._kv_len(encoder_input_lengths, enc)
        out = PairScore(torch.empty(S, device=dev), torch.empty(S, 2, device=dev), torch.empty(S, maxlen, 2, device=dev),
                        torch.empty(N, dtype=torch.int32, device=dev))
        segL = tuple(range(1, maxlen + 1))
        clips = max(1, SCORE_PAIRS_MAX_ROWS // (sum(segL) * G))      # clips per chunk
        heads = (self.tgt_word_prj_l2r.weight, self.tgt_word_prj_r2l.weight)
        with torch.no_grad():
            for c0 in range(0, N, clips):
                c1 = min(N, c0 + clips)
                s0, s1 = c0 * G, c1 * G
                layers, main, side, kv = self._begin(enc[c0:c1])
                tok = [y[s0:s1] for y in ys]
                last = self._stage_last(tok, s1 - s0, segL, layers, main, side, kv, kv_group=G,
                                        kv_len=None if kv_len is None else kv_len[c0:c1])
                ops.pair_score_tail(last[0], last[1], heads[0], heads[1], tok[0], tok[1], None if n_pos is None else n_pos[s0:s1], G,
                                    out.logp[s0:s1], out.score_dir[s0:s1], out.score[s0:s1], out.best[c0:c1])
        return out

    def recognize_words(self, encoder_outputs, lexicon, beam_size=None, nbest=1, shortlist=8, encoder_input_lengths=None):
        """Closed-vocabulary decode: the word of `lexicon` (transformer.lexicon.Lexicon) for every clip, in two passes on the
        device.  Hypotheses: the greedy pair of recognize_beam (beam_size = None, H = 1) or the nbest pairs of
        beam_search(beam_size, nbest) (H = nbest).  Shortlist (sbl_lexicon_shortlist): D(h, w) = lev(p_l, w) +
        lev(p_r, reversed(w)) with p_l / p_r the hypothesis rows cut before the first eos; a word's key is its smallest (D, h)
        and the K = shortlist words with the smallest (D, h, w) are kept.  Rescoring: score_pairs(group = K) on the candidates'
        token rows over their c_w + 1 trained positions; the word is the candidate with the largest score (the lower rank on
        an exact tie).  No host read: capturable as one hipGraph.
        Returns WordResult(word (N,) int64, cand, cand_dist, cand_hyp (N, K) int32, score (N, K), score_dir (N, K, 2))."""
        enc = encoder_outputs
        K = int(shortlist)
        self._need_gpu("Decoder.recognize_words", enc)
        if not 1 <= K <= min(len(lexicon), ops.LEXICON_MAX_SHORTLIST):
            raise _lib.SblHipError("Decoder.recognize_words: shortlist = %d outside 1..min(%d words, %d)"
                                   % (K, len(lexicon), ops.LEXICON_MAX_SHORTLIST))
        self._check_lexicon("Decoder.recognize_words", lexicon)
        kv_len = self._kv_len(encoder_input_lengths, enc)
        if beam_size is None:
            ys_l, ys_r = self.recognize_beam(enc, kv_len)
        else:
            res = self.beam_search(enc, beam_size, nbest, kv_len)
            ys_l, ys_r = res.ys_l2r, res.ys_r2l
        N = enc.size(0)
        sl = ops.lexicon_shortlist(ys_l, ys_r, lexicon.packed, K, self.sos_id, self.eos_id, IGNORE_ID)
        ps = self.score_pairs(enc, sl.cand_ys_l2r, sl.cand_ys_r2l, sl.n_pos, group=K, encoder_input_lengths=kv_len)
        word = sl.cand.gather(1, ps.best.long().unsqueeze(1)).squeeze(1).long()
        return WordResult(word, sl.cand, sl.cand_dist, sl.cand_hyp, ps.score.view(N, K), ps.score_dir.view(N, K, 2))

    def beam_search_lex(self, encoder_outputs, lexicon, beam_size, nbest=1, encoder_input_lengths=None):
        """Closed-vocabulary decode in ONE pass: beam_search restricted to the words of `lexicon` (transformer.lexicon.Lexicon)
        through its pair trie (Lexicon.pair_trie; include/sbl_hip.h, sbl_pair_beam_tail_lex).  Every hypothesis pair is one
        word - the l2r row spells w, the r2l row reversed(w), which is what the model was trained on - so the n-best are
        distinct words.  The stage, the K/V hoist and the two streams are beam_search's; the tail keeps, of the trie edges
        of every live slot, the clip's best W by score[s] + (lpL[a] + lpR[b]) (ties: lower slot, then lower key), and a pair
        that has emitted (eos, eos) is carried with its score unchanged.  The log-softmax is not renormalised and there is no
        length normalisation or prior, so a word's total is score_pairs(..., n_pos = c_w + 1) on its rows, the quantity
        recognize_words ranks by.  steps = lexicon.max_len + 1 iterations (host-known): after the last one every live slot
        sits on a terminal node.  No host read: capturable as one hipGraph.
        Returns PairWordBeamResult(word (N,) int64, cand (N, nbest) int32 = the n-best words, best first, -1 at dead ranks,
        score (N, nbest), score_dir (N, nbest, 2), ys_l2r, ys_r2l (N, nbest, 17) int64 = sos, w, eos fill and sos,
        reversed(w), eos fill, history = (l2r token, r2l token, parent rank, total score, node), each (N, steps, W))."""
        enc = encoder_outputs
        W, nbest = self._search_args("Decoder.beam_search_lex", enc, beam_size, nbest)
        self._check_lexicon("Decoder.beam_search_lex", lexicon)
        N, L = enc.size(0), config.MAX_DECODE_LEN + 1
        steps = lexicon.max_len + 1
        trie = lexicon.pair_trie()
        kv_len = self._kv_len(encoder_input_lengths, enc)
        with torch.no_grad():
            st = self._beam_steps(enc, W, steps, kv_len, lambda *a: ops.pair_beam_tail_lex(*a, trie), lex=True)
            cand = trie[2][st.nodes(steps)[:, :nbest].long()]      # a dead rank sits on node 0, whose word is -1
        ys_l, ys_r = (y.view(N, W, L)[:, :nbest] for y in st.prefixes(steps))
        return PairWordBeamResult(cand[:, 0].long(), cand, st.score[:, :nbest], st.score_dir[:, :nbest], ys_l, ys_r,
                                  st.history() + (st.hist_node,))


class DecoderLayer(nn.Module):
    ''' Causal self-attention, attention to the encoder output, position-wise FFN (decoder.py:387-408) '''

    def __init__(self, d_model, d_inner, n_head, d_k, d_v, dropout=0.1):
        super(DecoderLayer, self).__init__()
        self.slf_attn = MultiHeadAttention(n_head, d_model, d_k, d_v, dropout=dropout)
        self.enc_attn = MultiHeadAttention(n_head, d_model, d_k, d_v, dropout=dropout)
        self.pos_ffn = PositionwiseFeedForward(d_model, d_inner, dropout=dropout)

    def forward_rows(self, x2, B, segL, slf_attn_mask, enc_kv, kv_group=None, kv_len=None):
        """The layer on a ragged batch of rows (see MultiHeadAttention.forward_rows); non_pad_mask is all ones on
        this path (decoder.py:109,112).  kv_group = W: enc_kv belongs to B / W clips whose W beam slots share it.
        kv_len: device int32 key counts of the enc_kv entries (cross-attention only)."""
        x2, _ = self.slf_attn.forward_rows(x2, B, segL, mask=slf_attn_mask)
        x2, _ = self.enc_attn.forward_rows(x2, B, segL, mask=None, kv_proj=enc_kv, kv_group=kv_group, kv_len=kv_len)
        return self.pos_ffn(x2)

    def forward(self, dec_input, enc_output, non_pad_mask=None, slf_attn_mask=None, dec_enc_attn_mask=None,
                enc_kv=None):
        h, self_attn = self.slf_attn(dec_input, dec_input, dec_input, mask=slf_attn_mask)
        h = mask_rows(h, non_pad_mask)
        h, cross_attn = self.enc_attn(h, enc_output, enc_output, mask=dec_enc_attn_mask, kv_proj=enc_kv)
        h = mask_rows(h, non_pad_mask)
        return mask_rows(self.pos_ffn(h), non_pad_mask), self_attn, cross_attn
