"""The single-direction phoneme seq2seq model: the reference's VSR_seq2seq_Transformer_with_phonemes_LRW/ ("LRW/" below; the
LRW1000 directory has the same classes with a 48-token vocabulary), the baseline the SBL model is measured against.

Seq2SeqDecoder / Seq2SeqTransformer keep the constructor and forward signatures and the state-dict keys of
LRW/transformer/decoder.py:Decoder and LRW/transformer/transformer.py:Transformer.  The teacher-forced pass is built from the
entry points the SBL model uses; the greedy decode keeps a K/V cache per layer and processes one new row per clip and step
(csrc/decode_step.hip; the GEMM / LayerNorm launches around that one-row attention core are the shared sub-layer functions
of ops.py) instead of re-running the whole prefix at every step as LRW/transformer/decoder.py:146-164 does: every
layer of this decoder is causal, so row i of every sub-layer depends on rows <= i only."""
import collections

import torch
import torch.nn as nn

from ._env import _lib, config, ops
from .decoder import DecoderLayer
from .module import PositionalEncoding
from .transformer import Transformer
from .utils import device_lengths, get_attn_pad_mask
from .video_frontend import Lipreading

IGNORE_ID = config.IGNORE_ID
MAX_TGT_LEN = 14          # pad_list's fixed max_len (LRW/transformer/utils.py:5): <sos> + at most 13 tokens
MAX_KEYS = 64             # one key per lane in the decode-step attention; the teacher-forced kernels share the bound
MAX_BEAM = 16             # slots per clip in the beam tail (csrc/decode_head.h); nbest has the same bound

# beam_search's result: yseq (N, nbest, maxlen+2) int64 (<sos>, tokens, eos-filled behind the end), lengths (N, nbest) int32,
# scores (N, nbest) fp32, n_hyps (N) int32 (ranks beyond it: length 0, score -inf), history = the per-(clip, step, rank)
# kept (token, parent rank, score, flag) tensors, each (N, maxlen, W)
BeamResult = collections.namedtuple("BeamResult", ("yseq", "lengths", "scores", "n_hyps", "history"))
# recognize_words' result: word (N,) int64, the lexicon word of the best hypothesis (-1: no hypothesis ended); cand (N, nbest)
# int32, the distinct words of the n-best, best first (-1 beyond n_hyps); score (N, nbest) fp32 = log P(word, eos | clip) of
# the teacher-forced model (+ priors), -inf beyond n_hyps; n_hyps (N) int32; yseq (N, nbest, Cmax + 3) int64 as in BeamResult.
# `word` and `cand` are what metrics.WordAccuracyMeter.update reads.
WordBeamResult = collections.namedtuple("WordBeamResult", ("word", "cand", "score", "n_hyps", "yseq"))


class Seq2SeqDecoder(nn.Module):
    """n_layers causal decoder layers over one target direction (LRW/transformer/decoder.py:19-176).

    With tgt_emb_prj_weight_sharing the output projection and the embedding are ONE parameter and the embedding is scaled
    by x_logit_scale = d_model ** -0.5 (decoder.py:57-62); otherwise they are separate and the scale is 1."""

    def __init__(
            self, sos_id, eos_id,
            n_tgt_vocab, d_word_vec,
            n_layers, n_head, d_k, d_v,
            d_model, d_inner, dropout=0.1,
            tgt_emb_prj_weight_sharing=True,
            pe_maxlen=5000):
        super(Seq2SeqDecoder, self).__init__()
        if d_model != 512 or d_word_vec != d_model or d_k != 64 or d_v != 64:
            raise _lib.SblHipError("Seq2SeqDecoder: the HIP kernels are built for d_model = d_word_vec = 512 and d_k = d_v = 64 "
                                   "(got %d, %d, %d, %d)" % (d_model, d_word_vec, d_k, d_v))
        if not 1 <= n_tgt_vocab <= 64:
            raise _lib.SblHipError("Seq2SeqDecoder: n_tgt_vocab = %d outside 1..64 (the decode tail keeps one class per lane)"
                                   % n_tgt_vocab)
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
        self.tgt_emb_prj_weight_sharing = tgt_emb_prj_weight_sharing
        self.pe_maxlen = pe_maxlen

        self.tgt_word_emb = nn.Embedding(n_tgt_vocab, d_word_vec)
        self.positional_encoding = PositionalEncoding(d_model, max_len=pe_maxlen)
        self.dropout = nn.Dropout(dropout)
        self.layer_stack = nn.ModuleList(DecoderLayer(d_model, d_inner, n_head, d_k, d_v, dropout=dropout)
                                         for _ in range(n_layers))
        self.tgt_word_prj = nn.Linear(d_model, n_tgt_vocab, bias=False)
        nn.init.xavier_normal_(self.tgt_word_prj.weight)
        if tgt_emb_prj_weight_sharing:
            self.tgt_word_prj.weight = self.tgt_word_emb.weight
            self.x_logit_scale = d_model ** -0.5
        else:
            self.x_logit_scale = 1.

    # ------------------------------------------------------------------ parameter layout
    def cross_attention_modules(self):
        """The layers' cross-attention modules, in layer order.  Their [w_ks; w_vs] rows (and biases) form one block
        [K_0; V_0; K_1; ...] so that the encoder output's K / V for ALL layers are one GEMM in recognize_beam;
        dp.FlatModel lays the block out itself, otherwise _fuse() does."""
        return [lay.enc_attn for lay in self.layer_stack]

    def _fuse(self):
        """Idempotent (pointer checks): q/k/v of every self-attention adjacent, the cross-attention K/V block adjacent."""
        for lay in self.layer_stack:
            lay.slf_attn._fuse()
        mods = self.cross_attention_modules()
        ws, bs = ops.kv_block(mods)
        for m in mods:
            m.kv_in_block = True
        if ops._adjacent(*ws) and ops._adjacent(*bs):
            return
        if getattr(ws[0], "_sbl_flat", None) is not None:
            raise _lib.SblHipError("Seq2SeqDecoder: the flat model's cross-attention K/V block is not contiguous")
        ops.fuse_rows(ws, bs)

    # ------------------------------------------------------------------ teacher-forced pass
    def preprocess(self, padded_input):
        """decoder.py:64-79: strip IGNORE_ID; ys_in = <sos> + y padded with eos, ys_out = y + <eos> padded with IGNORE_ID,
        both (N, 14).  Vectorised on the input's device: no per-row loop, no host sync."""
        N, To = padded_input.shape
        if To > MAX_TGT_LEN - 1:
            raise _lib.SblHipError("Seq2SeqDecoder: targets of width %d; at most %d tokens fit the fixed length %d "
                                   "(LRW/transformer/utils.py:5)" % (To, MAX_TGT_LEN - 1, MAX_TGT_LEN))
        y = padded_input.long()
        valid = y.ne(IGNORE_ID)
        order = torch.argsort((~valid).to(torch.int8), dim=1, stable=True)      # stable compaction of the valid ids to the left
        comp = torch.gather(y, 1, order)
        n_valid = valid.sum(1, keepdim=True)
        inside = torch.arange(To, device=y.device).unsqueeze(0) < n_valid
        ys_in = y.new_full((N, MAX_TGT_LEN), self.eos_id)
        ys_in[:, 0] = self.sos_id
        ys_in[:, 1:1 + To] = torch.where(inside, comp, torch.full_like(comp, self.eos_id))
        ys_out = y.new_full((N, MAX_TGT_LEN), IGNORE_ID)
        ys_out[:, :To] = torch.where(inside, comp, torch.full_like(comp, IGNORE_ID))
        ys_out.scatter_(1, n_valid, self.eos_id)
        return ys_in, ys_out

    def _check_encoder(self, enc):
        if enc.dim() != 3 or enc.size(-1) != self.d_model:
            raise _lib.SblHipError("Seq2SeqDecoder: encoder output of shape %s, expected (N, T, %d)" % (tuple(enc.shape), self.d_model))
        if enc.size(1) > MAX_KEYS:
            raise _lib.SblHipError("Seq2SeqDecoder: %d encoder frames; the attention kernels hold at most %d keys" % (enc.size(1), MAX_KEYS))
        if not enc.is_cuda:
            raise _lib.SblHipError("Seq2SeqDecoder needs CUDA/HIP tensors (got a %s tensor); there is no CPU path" % enc.device)

    def forward(self, padded_input, encoder_padded_outputs, encoder_input_lengths, return_attns=False):
        """padded_input (N, To <= 13) IGNORE_ID-padded targets, encoder_padded_outputs (N, Ti, 512).  The one-shot
        teacher-forced pass of decoder.py:81-136.  Returns (pred (N, 14, V), gold (N, 14)) [+ the attention lists]."""
        enc = encoder_padded_outputs
        self._check_encoder(enc)
        self._fuse()
        N, Ti, _ = enc.shape
        ys_in, ys_out = self.preprocess(padded_input.to(enc.device))
        L = ys_in.size(1)
        # the K / V projections of the encoder output come first: the backward of every other decoder node then outranks
        # theirs in autograd's ready queue, so the decoder's gradients are complete when the encoder-output gradient is
        # (dp.GradientExchange launches the decoder segment there)
        kv = [lay.enc_attn.project_kv(enc) for lay in self.layer_stack]
        pad = ys_in.eq(self.eos_id)
        non_pad_mask = (~pad).float().unsqueeze(-1)
        future = torch.ones((L, L), dtype=torch.bool, device=enc.device).triu(1)
        slf_attn_mask = pad.unsqueeze(1) | future.unsqueeze(0)                   # key-pad OR causal, (N, L, L)
        on_device = isinstance(encoder_input_lengths, torch.Tensor) and encoder_input_lengths.is_cuda      # never read back
        if not on_device and all(int(n) >= Ti for n in encoder_input_lengths):
            dec_enc_attn_mask = None                                              # full lengths: the mask is a no-op
        else:
            dec_enc_attn_mask = get_attn_pad_mask(enc, encoder_input_lengths, L)
        x = ops.EmbedScalePEFn.apply(ys_in, self.tgt_word_emb.weight, self.positional_encoding.pe[0], float(self.x_logit_scale))
        x = ops.dropout(x, self.dropout.p, self.training)
        slf_list, enc_list = [], []
        for lay, kv_l in zip(self.layer_stack, kv):
            x, slf, cross = lay(x, enc, non_pad_mask=non_pad_mask, slf_attn_mask=slf_attn_mask,
                                dec_enc_attn_mask=dec_enc_attn_mask, enc_kv=kv_l)
            if return_attns:
                slf_list.append(slf)
                enc_list.append(cross)
        pred = ops.linear(x, self.tgt_word_prj.weight)
        if return_attns:
            return pred, ys_out, slf_list, enc_list
        return pred, ys_out

    # ------------------------------------------------------------------ greedy decode
    def recognize_beam(self, encoder_outputs, char_list=None, args=None, cached=True, encoder_input_lengths=None):
        """Greedy decode of maxlen = Ti steps (decoder.py:138-176; char_list / args are accepted and unused, as there).
        Returns ys int64 (N, Ti + 1), column 0 is <sos>.  cached=True: one new row per clip and step against per-layer K/V
        caches; cached=False: the reference's loop, the whole prefix re-run at every step through the teacher-forced building
        blocks (the statement the cached path is tested against).  No host sync either way.
        encoder_input_lengths (here and in every decode method below): None, or the clips' frame counts l - N ints or a device
        int32 (N,) tensor, which is never read on the host.  Clip n then attends to the encoder rows t < l_n only and decodes
        as the reference decodes it alone, cut to l_n frames: ys[n, 1..l_n] are its l_n tokens and ys[n, l_n+1..] is eos_id
        (all Ti steps are still issued; the columns behind l_n are overwritten by one masked fill on the device)."""
        self._check_encoder(encoder_outputs)
        lens = self._kv_len(encoder_input_lengths, encoder_outputs)
        self._fuse()
        with torch.no_grad():
            ys = self._greedy_cached(encoder_outputs, lens) if cached else self._greedy_recompute(encoder_outputs, lens)
            if lens is not None:
                T = encoder_outputs.size(1)
                behind = torch.arange(T + 1, device=ys.device).unsqueeze(0) > lens.clamp(1, T).unsqueeze(1)
                ys.masked_fill_(behind, self.eos_id)
            return ys

    _kv_len = staticmethod(device_lengths)

    def _new_ys(self, enc):
        return torch.full((enc.size(0), enc.size(1) + 1), self.sos_id, dtype=torch.long, device=enc.device)

    def _greedy_recompute(self, enc, lens=None):
        N, T, _ = enc.shape
        kv = [lay.enc_attn.project_kv(enc) for lay in self.layer_stack]       # step-invariant
        ys = self._new_ys(enc)
        emb, pe, w = self.tgt_word_emb.weight, self.positional_encoding.pe[0], self.tgt_word_prj.weight
        for i in range(T):
            x = ops.EmbedScalePEFn.apply(ys[:, :i + 1], emb, pe, float(self.x_logit_scale))
            x = ops.dropout(x, self.dropout.p, self.training)
            # ragged clips: the explicit key mask of the teacher-forced pass, built on the device from the lengths tensor
            cross_mask = None if lens is None else get_attn_pad_mask(enc, lens, i + 1)
            for lay, kv_l in zip(self.layer_stack, kv):
                x, _, _ = lay(x, enc, non_pad_mask=None, slf_attn_mask='causal', dec_enc_attn_mask=cross_mask, enc_kv=kv_l)
            ops.argmax_select(ops.linear(x[:, -1], w), None, ys, i, 1)
        return ys

    def _cached_steps(self, enc, rows, steps, tok0, attn, tail, kv_len=None):
        """The KV-cached step loop under the greedy decode and the beam search: `rows` rows per step (the clips, or their
        beam slots) for `steps` steps.  One GEMM for the cross-attention K / V of all layers, the first input row from the
        (rows, >= 1) token table tok0, then per step and layer the 11 launches of DESIGN.md section 4.4 and the tail;
        nothing is read back.  attn(step, ...) takes the arguments of ops.decode_attn_step; tail(y, w, step, emb, pe, scale,
        x_next) ends a step (x_next: the next step's input rows, None at the last one).  kv_len: None, or the clips' device
        int32 key counts for every cross-attention (attn's kv_len=)."""
        N, T, D = enc.shape
        layers = [(lay.slf_attn.handle(), lay.enc_attn.handle(cross=True), lay.pos_ffn.handle()) for lay in self.layer_stack]
        nl, H = len(layers), self.n_head
        HD, F_ = H * 64, self.d_inner
        new = lambda *shape: torch.empty(*shape, device=enc.device, dtype=torch.float32)      # noqa: E731

        # the K / V of the encoder output for all layers: one GEMM against the [K_0; V_0; K_1; ...] block, over the N clips
        kv = [blk.view(N, T, 2 * HD) for blk in ops.project_kv_block(enc.contiguous().view(N * T, D), self.cross_attention_modules())[2]]
        cache = new(nl, 2, rows, steps, HD)   # self-attention K / V rows of every layer; row i of a cache is written at step i
        emb, pe, w = self.tgt_word_emb.weight, self.positional_encoding.pe[0], self.tgt_word_prj.weight
        V, scale = emb.size(0), float(self.x_logit_scale)
        x = new(rows, D)
        ops.call("sbl_embed_scale_pe_fwd", ops._p(tok0), tok0.stride(0), ops._p(emb), ops._p(pe), ops._p(x), rows, 1, D, V, scale, 0, ops._s())
        qkv, q, att, o, h = new(rows, 3 * HD), new(rows, HD), new(rows, HD), new(rows, D), new(rows, F_)
        ya, yb, yc = new(rows, D), new(rows, D), new(rows, D)
        mean, rstd = new(rows), new(rows)

        for i in range(steps):
            cur = x
            for l, (sa, ca, ff) in enumerate(layers):
                ops.lin_fwd(sa.inp, cur, qkv)
                attn(i, qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:], cache[l, 0], cache[l, 1], steps, att, H, i, True)
                ops.out_ln_fwd(sa, att, cur, None, 0, (o, ya, mean, rstd))
                ops.lin_fwd(ca.inp, ya, q)
                attn(i, q, None, None, kv[l][:, :, :HD], kv[l][:, :, HD:], T, att, H, T, False, kv_len=kv_len)
                ops.out_ln_fwd(ca, att, ya, None, 0, (o, yb, mean, rstd))
                ops.ffn_fwd(ff, yb, None, 0, h, (o, yc, mean, rstd))
                cur = yc
            tail(cur, w, i, emb, pe, scale, x if i + 1 < steps else None)

    def _require_eval(self):
        if self.training and self.dropout.p > 0:
            raise _lib.SblHipError("Seq2SeqDecoder: the cached decode has no dropout; call eval() (or recognize_beam(cached=False))")

    def _greedy_cached(self, enc, lens=None):
        self._require_eval()
        ys = self._new_ys(enc)
        self._cached_steps(enc, enc.size(0), enc.size(1), ys, lambda i, *a, **kw: ops.decode_attn_step(*a, **kw),
                           lambda y, w, i, *head: ops.decode_tail(y, w, ys, i, *head), kv_len=lens)
        return ys

    # ------------------------------------------------------------------ beam search
    def beam_search(self, encoder_outputs, beam_size, nbest=1, decode_max_len=0, log_prior=None):
        """Beam search of LRW1000/transformer/decoder.py:131-245 for all N clips at once: each clip keeps beam_size
        hypotheses, every step adds log_softmax(logits) + log_prior[last token] (log_prior: None or the (V, V) fp32 table
        torch.log(bigram_freq), -inf allowed) in fp32, hypotheses that emit <eos> move to the ended list, at step
        maxlen - 1 (maxlen = decode_max_len or Ti) every kept hypothesis ends with an appended <eos>, and the nbest best
        ended hypotheses come back, best first, without length normalisation -> BeamResult.  Exact ties, which the
        reference leaves to torch.topk: the lower parent slot first, then the lower token id.  A candidate of score -inf
        is never kept.  The step is KV-cached like the greedy decode (one new row per slot and step; the slots' caches are
        followed through an ancestry table, never copied), eval-only, with no host read: capturable as one hipGraph.
        Ragged clips: beam_search_len."""
        return self.beam_search_lex(encoder_outputs, beam_size, nbest, decode_max_len, log_prior, None)

    def beam_search_lex(self, encoder_outputs, beam_size, nbest=1, decode_max_len=0, log_prior=None, lexicon=None):
        """beam_search with an optional word list.  lexicon (transformer.lexicon.Lexicon, on the encoder output's device,
        with this decoder's vocab / sos / eos; decode_max_len must then be 0): the search is restricted to the prefixes of
        the words (include/sbl_hip.h, sbl_beam_tail_lex).  Every hypothesis is a word, the n-best are distinct words, scores
        are not renormalised over the allowed tokens, and the search runs maxlen = longest word + 1 steps -> BeamResult.
        None: the unconstrained search of beam_search, launch for launch.  Ragged clips: beam_search_len."""
        return self.beam_search_len(encoder_outputs, None, beam_size, nbest, decode_max_len, log_prior, lexicon)

    def beam_search_len(self, encoder_outputs, encoder_input_lengths, beam_size, nbest=1, decode_max_len=0, log_prior=None,
                        lexicon=None):
        """beam_search / beam_search_lex over a padded batch of ragged clips (those two keep their signatures and call this
        with encoder_input_lengths = None, which is their code path of before, launch for launch).
        encoder_input_lengths (see recognize_beam): clip n attends to its l_n frames and, without a lexicon and with
        decode_max_len == 0, its maxlen is l_n as for the reference alone - every kept hypothesis ends at step l_n - 1 with
        length l_n + 2, and the clip has no live hypothesis from step l_n on (Ti steps are still issued).  With
        decode_max_len != 0 or a lexicon the step count stays uniform (decode_max_len, as in the reference; the longest
        word's + 1) and only the cross-attention learns the lengths."""
        enc = encoder_outputs
        self._check_encoder(enc)
        lens = self._kv_len(encoder_input_lengths, enc)
        N, T, D = enc.shape
        W, nbest = int(beam_size), int(nbest)
        maxlen = int(decode_max_len) or T
        V = self.n_tgt_vocab
        if lexicon is not None:
            if (lexicon.vocab, lexicon.sos_id, lexicon.eos_id) != (V, self.sos_id, self.eos_id):
                raise _lib.SblHipError("Seq2SeqDecoder.beam_search_lex: the lexicon's vocab / sos / eos = %d / %d / %d, the decoder's %d / %d / %d"
                                       % (lexicon.vocab, lexicon.sos_id, lexicon.eos_id, V, self.sos_id, self.eos_id))
            if lexicon.packed.device != enc.device:
                raise _lib.SblHipError("Seq2SeqDecoder.beam_search_lex: the lexicon is on %s, the encoder output on %s"
                                       % (lexicon.packed.device, enc.device))
            if int(decode_max_len) != 0:
                raise _lib.SblHipError("Seq2SeqDecoder.beam_search_lex: decode_max_len = %d with a lexicon (the longest word sets "
                                       "the number of steps; pass 0)" % decode_max_len)
            maxlen = lexicon.max_len + 1
        if not 1 <= W <= min(MAX_BEAM, V):
            raise _lib.SblHipError("Seq2SeqDecoder.beam_search: beam_size = %d outside 1..min(%d, V = %d)" % (W, MAX_BEAM, V))
        if not 1 <= nbest <= MAX_BEAM:
            raise _lib.SblHipError("Seq2SeqDecoder.beam_search: nbest = %d outside 1..%d" % (nbest, MAX_BEAM))
        if not 1 <= maxlen <= min(MAX_KEYS, self.pe_maxlen):
            raise _lib.SblHipError("Seq2SeqDecoder.beam_search: %d decode steps; the cache holds at most %d rows and the "
                                   "positional table %d" % (maxlen, MAX_KEYS, self.pe_maxlen))
        if log_prior is not None and (log_prior.dtype != torch.float32 or tuple(log_prior.shape) != (V, V)
                                      or log_prior.device != enc.device):
            raise _lib.SblHipError("Seq2SeqDecoder.beam_search: log_prior must be a (%d, %d) fp32 tensor on %s" % (V, V, enc.device))
        self._require_eval()
        self._fuse()
        with torch.no_grad():
            # the step count is per clip where the reference's maxlen is the clip's frame count
            clip_steps = lens if lexicon is None and int(decode_max_len) == 0 else None
            return self._beam_cached(enc, W, nbest, maxlen, None if log_prior is None else log_prior.contiguous(),
                                     None if lexicon is None else lexicon.trie(), lens, clip_steps)

    def _beam_cached(self, enc, W, nbest, maxlen, log_prior, trie=None, kv_len=None, clip_steps=None):
        S = enc.size(0) * W       # the W slots of a clip read the clip's cross-attention K / V
        st = ops.BeamState(enc.size(0), W, maxlen, self.sos_id, enc.device, lex=trie is not None)
        tok0 = torch.full((S, 1), self.sos_id, dtype=torch.long, device=enc.device)

        def attn(i, q, k_new, v_new, k_cache, v_cache, Lcap, out, H, n_prev, append, **kw):
            # row i of slot b's cache is written at step i by whatever hypothesis lives in b then
            ops.beam_attn_step(q, k_new, v_new, k_cache, v_cache, Lcap, st.anc[i % 2] if append else None, out, W, H, n_prev, append,
                               **kw)

        self._cached_steps(enc, S, maxlen, tok0, attn,
                           lambda y, w, i, *head: ops.beam_tail(y, w, log_prior, st, i, self.eos_id, *head, trie=trie,
                                                                clip_steps=clip_steps), kv_len=kv_len)
        return BeamResult(*ops.beam_finish(st, nbest, self.eos_id, clip_steps=clip_steps), st.history())

    def recognize_words(self, encoder_outputs, lexicon, beam_size=8, nbest=1, log_prior=None):
        """Closed-vocabulary decode in one pass: the beam search restricted to `lexicon` (beam_search_lex),
        then one lookup launch that names the n-best -> WordBeamResult.  The score of a word is the model's own
        log P(word, eos | clip) (+ log_prior's bigram terms); with a beam no narrower than the trie it is the exact ranking
        of the lexicon.  No host read: capturable as one hipGraph once lexicon.trie() has been built."""
        return self.recognize_words_len(encoder_outputs, None, lexicon, beam_size, nbest, log_prior)

    def recognize_words_len(self, encoder_outputs, encoder_input_lengths, lexicon, beam_size=8, nbest=1, log_prior=None):
        """recognize_words over a padded batch of ragged clips: every cross-attention of clip n sees its first
        encoder_input_lengths[n] encoder rows only (None: recognize_words).  The step count is the longest word's + 1 for
        every clip, as without lengths."""
        res = self.beam_search_len(encoder_outputs, encoder_input_lengths, beam_size, nbest, 0, log_prior, lexicon)
        cand = lexicon.lookup(res.yseq)
        return WordBeamResult(cand[:, 0].long(), cand, res.scores, res.n_hyps, res.yseq)


class Seq2SeqTransformer(nn.Module):
    """Lip crops -> visual frontend -> encoder -> single-direction decoder (LRW/transformer/transformer.py:4-75).  Submodule
    names `encoder`, `decoder`, `lipreading` and their registration order are the reference's, so its state-dict keys load
    and the construction-time Xavier re-draw of every parameter of rank >= 2 (the tied weight once) consumes the RNG as it
    does there."""

    # dp.FlatModel layout (see classifier.ClassifierTransformer)
    FLAT_SEGMENTS = ("decoder.", "encoder.", "lipreading.resnet18.layer4.", "lipreading.resnet18.layer3.",
                     "lipreading.resnet18.layer2.", "lipreading.")
    FLAT_FEEDS = (("encoder", "decoder."), ("lipreading", "encoder."))
    FLAT_FRONTEND = "lipreading"

    def __init__(self, encoder, decoder):
        super(Seq2SeqTransformer, self).__init__()
        self.encoder = encoder
        self.decoder = decoder
        self.lipreading = Lipreading(hiddenDim=512, embedSize=256)
        for w in [p for p in self.parameters() if p.dim() > 1]:
            nn.init.xavier_uniform_(w)

    def _encode(self, frames, input_lengths=None):
        """frames (N, T, H, W) grayscale or an ops.RawClips -> (encoder output (N, T, 512), lengths).  input_lengths = None:
        full lengths, as the reference passes them; else the host lengths of forward or the device int32 (N,) frame counts of
        Transformer._lengths (inference) - the frames behind a clip's count must be all-zero frames, what the loader pads
        with and what the stem's temporal zero padding gives the clip cut to its count; the encoder keeps them out of its
        attention and zeroes their rows."""
        if not isinstance(frames, ops.RawClips):
            frames = frames.unsqueeze(1)
        feats = self.lipreading(frames)
        lengths = [feats.size(1)] * feats.size(0) if input_lengths is None else input_lengths
        enc, *_ = self.encoder(feats, lengths)
        return enc, lengths

    _lengths = staticmethod(Transformer._lengths)

    def forward(self, padded_input, padded_target, input_lengths=None):
        """padded_input (N, T, H, W) or ops.RawClips; padded_target (N, To <= 13), IGNORE_ID padded.
        Returns (pred (N, 14, V), gold (N, 14)).  input_lengths: None, or the clips' frame counts for the encoder's and the
        decoder's key masks (both honour them under autograd; BatchNorm's batch statistics still run over the padded
        frames, as in the reference)."""
        enc, lengths = self._encode(padded_input, input_lengths)
        pred, gold, *_ = self.decoder(padded_target, enc, lengths)
        return pred, gold

    def recognize(self, input, char_list=None, args=None, cached=True, input_lengths=None):
        """Greedy decode of (N, T, H, W) crops (or ops.RawClips): ys int64 (N, T + 1).  In eval() under torch.no_grad() the
        whole call is capturable as one hipGraph (no host sync, no host read of device data).
        input_lengths (here and in every inference method below; gradients disabled): None, or the clips' frame counts (N
        ints, checked before anything runs, or a device int32 (N,) tensor, never read on the host: Transformer._lengths).
        Clip n then decodes as it would alone, cut to its first input_lengths[n] frames (its frames behind the count must be
        all-zero frames), and ys[n] is eos_id behind its input_lengths[n] tokens."""
        lens = self._lengths(input, input_lengths)
        enc, _ = self._encode(input, lens)
        return self.decoder.recognize_beam(enc, char_list, args, cached=cached, encoder_input_lengths=lens)

    def recognize_nbest(self, input, char_list, args, log_prior=None, input_lengths=None):
        """The beam search of LRW1000/transformer/transformer.py:46-72 for every clip of a batch: args.beam_size, args.nbest and
        args.decode_max_len as there (char_list is unused there too).  Returns, per clip, the reference's
        [{'score': float, 'yseq': [ids]}], best first.  One synchronisation, the read of the result."""
        lens = self._lengths(input, input_lengths)
        enc, _ = self._encode(input, lens)
        res = self.decoder.beam_search_len(enc, lens, args.beam_size, args.nbest, args.decode_max_len, log_prior)
        host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t, non_blocking=True) for t in res[:4]]
        torch.cuda.current_stream(res.yseq.device).synchronize()
        yseq, lengths, scores, n_hyps = (t.tolist() for t in host)
        return [[{'score': scores[n][k], 'yseq': yseq[n][k][:lengths[n][k]]} for k in range(n_hyps[n])] for n in range(len(yseq))]

    def validate(self, padded_input, padded_target, meter, valid_rows=None, beam_size=None, log_prior=None, input_lengths=None):
        """One validation batch (the body of LRW/train.py:229-254): greedy decode, then score ys against the (N, To)
        IGNORE_ID-padded targets into `meter` (metrics.ErrorRateMeter) on the device; capturable like recognize.  Returns ys.
        With beam_size the decode is the beam search (log_prior as in Seq2SeqDecoder.beam_search) and ys its 1-best yseq
        (N, T + 2), whose eos padding the scorer strips like the greedy rows' tail.  With input_lengths a clip's row is eos
        behind its own tokens, so it is scored as if decoded alone."""
        if beam_size is None:
            ys = self.recognize(padded_input, input_lengths=input_lengths)
        else:
            lens = self._lengths(padded_input, input_lengths)
            ys = self.decoder.beam_search_len(self._encode(padded_input, lens)[0], lens, beam_size, 1, 0, log_prior).yseq[:, 0]
        meter.update_single(ys, padded_target, valid_rows=valid_rows)
        return ys

    def recognize_words(self, input, lexicon, beam_size=8, nbest=1, log_prior=None):
        """Closed-vocabulary decode of (N, T, H, W) crops (or ops.RawClips): Seq2SeqDecoder.recognize_words on the encoder
        output -> WordBeamResult, the lexicon word of every clip with the distinct words of its n-best and their scores.
        Ragged clips: recognize_words_len."""
        return self.recognize_words_len(input, None, lexicon, beam_size, nbest, log_prior)

    def recognize_words_len(self, input, input_lengths, lexicon, beam_size=8, nbest=1, log_prior=None):
        """recognize_words with the clips' frame counts (input_lengths as in recognize; None: recognize_words)."""
        lens = self._lengths(input, input_lengths)
        enc, _ = self._encode(input, lens)
        return self.decoder.recognize_words_len(enc, lens, lexicon, beam_size=beam_size, nbest=nbest, log_prior=log_prior)

    def validate_words(self, padded_input, gold_word, lexicon, meter, valid_rows=None, beam_size=8, nbest=1, log_prior=None):
        """One validation batch of a closed-vocabulary benchmark: recognize_words, then `meter` (metrics.WordAccuracyMeter)
        counts the clips whose word is gold_word (N,) int64 - word indices into `lexicon`, as Lexicon.from_targets returns
        them - and those whose n-best holds it (the meter's n_in_shortlist).  No host read: in eval() under torch.no_grad()
        the call is capturable as one hipGraph, like validate; `valid_rows` (device int32[1]) masks the tail of a short last
        batch.  Returns the WordBeamResult.  Ragged clips: validate_words_len."""
        return self.validate_words_len(padded_input, None, gold_word, lexicon, meter, valid_rows, beam_size, nbest, log_prior)

    def validate_words_len(self, padded_input, input_lengths, gold_word, lexicon, meter, valid_rows=None, beam_size=8, nbest=1,
                           log_prior=None):
        """validate_words with the clips' frame counts (input_lengths as in recognize; None: validate_words)."""
        res = self.recognize_words_len(padded_input, input_lengths, lexicon, beam_size=beam_size, nbest=nbest, log_prior=log_prior)
        meter.update(res, gold_word, valid_rows=valid_rows)
        return res


__all__ = ["Seq2SeqDecoder", "Seq2SeqTransformer", "BeamResult", "WordBeamResult", "MAX_TGT_LEN"]
