// Batched beam search of the single-direction seq2seq decoder (LRW1000/transformer/decoder.py:131-245): the tail and the
// finish next to the greedy step of decode_step.hip, whose step attention both decodes run.
//
// The reference decodes one clip at a time and re-runs the whole prefix of every hypothesis at every step.  Here a clip
// owns W = beam_size SLOTS, the batch is S = N * W rows, and every launch has that fixed shape: a slot that holds no live
// hypothesis carries the score -inf (its rows are computed and never selected).  All live hypotheses of a clip have the
// same length at step i, so the K / V cache of decode_step.hip carries over, followed through the slots' ancestry rows
// (step_attn_kernel<true> there reads them; the tail here writes them).
//   * beam_tail_kernel: one workgroup per clip: the W projections to V <= 64 classes, log-softmax, + log-prior row of the
//     slot's last token + the slot's score, the best W of the W * V candidates, the hypotheses that end, the new ancestry
//     rows (double-buffered: the kernel reads the parents' rows), the (step, rank) history, and the next input rows.
//     beam_tail_kernel<true> (sbl_beam_tail_lex) is the same body restricted to the prefixes of a word list: a slot's
//     candidates are the tokens its trie node allows (include/sbl_hip.h).
//   * beam_finish_kernel: one wavefront per clip: the nbest best ended hypotheses (stable), traced back through the history.
// Ties (the reference leaves them to torch.topk and a stable sort): the lower parent slot first, then the lower token id;
// in the final list the hypothesis that ended first (earlier step, then better rank).
// A candidate of score -inf (a bigram of frequency zero) is never kept: the reference would carry it as a hypothesis of
// score -inf that can only ever surface behind every finite one.
#include "decode_head.h"

#define BEAM_MAX_LEN 64
#define BEAM_MAX_NBEST 16

// ------------------------------------------------------------------ beam tail: LRW1000/transformer/decoder.py:186-229
// grid N, 256 threads.  Slot n*W + r is beam position r of clip n.  Flags: 0 = nothing kept at this rank, 1 = live, 2 = ended.
// LEX (sbl_beam_tail_lex): every slot carries a node of the lexicon's trie (include/sbl_hip.h); candidate (slot, v) exists only
// where bit v of the node's mask is set - one 8-byte load per slot and a bit test per lane - and the kept rank's node is the
// parent's child under v, a popcount below bit v.  Everything else is the one body, so the two searches share their arithmetic.
// LEN (sbl_beam_tail_len): the clip's own last step, clamp(clip_steps[n], 1, maxlen) - 1, takes the place of maxlen - 1 in the
// forced end; a clip behind its last step has no live slot, so the body keeps nothing for it.
template <bool LEX, bool LEN = false>
__global__ __launch_bounds__(256) void beam_tail_kernel(
    const float* __restrict__ y, long ldy, const float* __restrict__ w, const float* __restrict__ log_prior, float* score,
    int32_t* last_tok, const int32_t* __restrict__ anc_old, int32_t* __restrict__ anc_new, long lda, int32_t* __restrict__ hist_tok,
    int32_t* __restrict__ hist_par, float* __restrict__ hist_score, int32_t* __restrict__ hist_flag, float* __restrict__ end_score,
    int32_t* __restrict__ end_ref, int32_t* end_count, int step, int maxlen, int eos, const float* __restrict__ emb,
    const float* __restrict__ pe, float emb_scale, float* __restrict__ x_next, int W, int V,
    const int64_t* __restrict__ trie_mask, const int32_t* __restrict__ trie_first, int P, int32_t* node,
    const int32_t* __restrict__ clip_steps) {
    __shared__ float s_cand[DH_MAX_W * 64];
    __shared__ int s_tok[DH_MAX_W], s_par[DH_MAX_W];
    __shared__ unsigned long long s_mask[DH_MAX_W];      // LEX: the slots' nodes (clamped to 0 .. P-1) and their masks
    __shared__ int s_node[DH_MAX_W];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x;
    const long slot0 = (long)n * W;

    // logits of the clip's W rows: each wave takes every fourth class and keeps its weight row in registers
    for (int v = wave; v < V; v += 4) {
        const float4* wr = reinterpret_cast<const float4*>(w + (long)v * DH_D);
        const float4 a = wr[lane], c = wr[64 + lane];
        for (int r = 0; r < W; ++r) {
            const float acc = dh_row_dot(reinterpret_cast<const float4*>(y + (slot0 + r) * ldy), a, c, lane);
            if (lane == 0) s_cand[r * 64 + v] = acc;
        }
    }
    __syncthreads();
    // candidates: score + (log_softmax(logits) + log_prior[last token]), lane = class; a dead slot offers nothing.  (The
    // log-softmax reads -inf for NaN; c below is clamped the same way, so a NaN ends as -inf with or without that.)
    for (int r = wave; r < W; r += 4) {
        const float sc = score[slot0 + r];
        int lt = last_tok[slot0 + r];
        lt = lt < 0 ? 0 : (lt >= V ? V - 1 : lt);
        const float lp = dh_log_softmax(lane < V ? s_cand[r * 64 + lane] : -INFINITY, lane < V);
        bool allowed = lane < V;
        if constexpr (LEX) {
            int q = node[slot0 + r];
            q = q < 0 ? 0 : (q >= P ? P - 1 : q);
            const unsigned long long m = (unsigned long long)trie_mask[q];
            allowed = allowed && ((m >> lane) & 1ull);
            if (lane == 0) {
                s_node[r] = q;
                s_mask[r] = m;
            }
        }
        float c = -INFINITY;
        if (allowed && sc > -INFINITY) {
            float local = lp;
            if (log_prior) local += log_prior[(long)lt * V + lane];
            c = sc + local;
            if (!(c > -INFINITY)) c = -INFINITY;      // NaN too
        }
        s_cand[r * 64 + lane] = c;
    }
    __syncthreads();
    if (wave == 0) {
        // W rounds of arg-max over the W * 64 candidates; lane v remembers which of its column's entries are taken.
        // Index = parent * 64 + token, so "lower index on ties" is the documented order.
        unsigned taken = 0;
        float my_sc = -INFINITY;
        int my_idx = DH_NONE;
        for (int r = 0; r < W; ++r) {
            float best = -INFINITY;
            int bi = DH_NONE;
            for (int t = 0; t < W; ++t) {
                const float c = s_cand[t * 64 + lane];
                if (!((taken >> t) & 1u) && c > best) {
                    best = c;
                    bi = t * 64 + lane;
                }
            }
            dh_wave_best(best, bi);
            if (bi != DH_NONE && (bi & 63) == lane) taken |= 1u << (bi >> 6);
            if (lane == r) {
                my_sc = best;
                my_idx = bi;
            }
        }
        const bool kept = lane < W && my_idx != DH_NONE;
        const int tok = kept ? (my_idx & 63) : eos;
        const int par = kept ? (my_idx >> 6) : lane;
        // decoder.py:213-218: at the last step every kept hypothesis gets an <eos> appended, one that ends in <eos> included
        int last = maxlen - 1;
        if constexpr (LEN) {
            const int l = clip_steps[n];
            last = (l < 1 ? 1 : (l > maxlen ? maxlen : l)) - 1;
        }
        const bool ended = kept && (tok == eos || step == last);
        const unsigned long long em = __ballot(ended);
        const int cnt = step == 0 ? 0 : end_count[n];
        const long cap = (long)W * maxlen;
        if (ended) {      // in kept order (decoder.py:222-227)
            const long pos = cnt + __popcll(em & ((1ull << lane) - 1ull));
            if (pos < cap) {
                end_score[n * cap + pos] = my_sc;
                end_ref[n * cap + pos] = step * W + lane;
            }
        }
        if (lane == 0) end_count[n] = cnt + (int)__popcll(em);
        if (lane < W) {
            const long hi = ((long)n * maxlen + step) * W + lane;
            hist_tok[hi] = tok;
            hist_par[hi] = par;
            hist_score[hi] = kept ? my_sc : -INFINITY;
            hist_flag[hi] = kept ? (ended ? 2 : 1) : 0;
            score[slot0 + lane] = kept && !ended ? my_sc : -INFINITY;
            last_tok[slot0 + lane] = tok;
            if constexpr (LEX) {      // the parent's node under tok; <eos> stays at the word's node; nothing kept: the root
                int q = 0;
                if (kept) {
                    q = s_node[par];
                    if (tok != eos) {
                        const unsigned long long below = s_mask[par] & ~(1ull << eos) & ((1ull << tok) - 1ull);
                        q = trie_first[q] + (int)__popcll(below);
                        q = q < 0 ? 0 : (q >= P ? P - 1 : q);
                    }
                }
                node[slot0 + lane] = q;
            }
            s_tok[lane] = tok;
            s_par[lane] = par;
        }
    }
    __syncthreads();
    // the new ancestry rows: the parent's keys 0 .. step-1, then the parent's own row `step`
    const int len = step + 1;
    for (int i = threadIdx.x; i < W * len; i += 256) {
        const int r = i / len, j = i - r * len;
        const long ps = slot0 + s_par[r];
        anc_new[(slot0 + r) * lda + j] = j < step ? anc_old[ps * lda + j] : (int32_t)ps;
    }
    if (x_next)      // (uniform) the next step's input rows
        for (int r = 0; r < W; ++r) dh_next_row(x_next + (slot0 + r) * DH_D, emb, s_tok[r], pe, step + 1, emb_scale);
}

// the checks and the launch of sbl_beam_tail, sbl_beam_tail_lex (trie_mask != NULL) and sbl_beam_tail_len (clip_steps != NULL)
static int beam_tail_launch(const char* name, const float* y, long ldy, const float* w, const float* log_prior, float* score,
                            int32_t* last_tok, const int32_t* anc_old, int32_t* anc_new, long lda, int32_t* hist_tok,
                            int32_t* hist_par, float* hist_score, int32_t* hist_flag, float* end_score, int32_t* end_ref,
                            int32_t* end_count, int step, int maxlen, int eos, const float* emb, const float* pe, int pe_rows,
                            float emb_scale, float* x_next, int N, int W, int V, int D, const int64_t* trie_mask,
                            const int32_t* trie_first, int P, int32_t* node, sbl_stream_t stream,
                            const int32_t* clip_steps = nullptr) {
    SBL_REQUIRE(D == DH_D, "%s: D=%d (built for %d)", name, D, DH_D);
    SBL_REQUIRE(V >= 1 && V <= DH_MAX_V, "%s: V=%d (V <= %d)", name, V, DH_MAX_V);
    SBL_REQUIRE(W >= 1 && W <= DH_MAX_W, "%s: beam W=%d outside 1..%d", name, W, DH_MAX_W);
    SBL_REQUIRE(W <= V, "%s: beam W=%d above V=%d", name, W, V);
    SBL_REQUIRE(maxlen >= 1 && maxlen <= BEAM_MAX_LEN, "%s: maxlen=%d outside 1..%d", name, maxlen, BEAM_MAX_LEN);
    SBL_REQUIRE(N > 0 && step >= 0 && step < maxlen, "%s: N=%d, step %d of %d", name, N, step, maxlen);
    SBL_REQUIRE(eos >= 0 && eos < V, "%s: eos=%d outside the %d classes", name, eos, V);
    SBL_REQUIRE(lda >= maxlen, "%s: ancestry rows of %ld entries for maxlen=%d", name, lda, maxlen);
    SBL_REQUIRE(y && w && score && last_tok && anc_old && anc_new && anc_old != anc_new, "%s: null or aliased state", name);
    SBL_REQUIRE(hist_tok && hist_par && hist_score && hist_flag && end_score && end_ref && end_count, "%s: null output", name);
    SBL_REQUIRE(ldy >= D && ldy % 4 == 0, "%s: row stride %ld", name, ldy);
    SBL_REQUIRE(!x_next || (emb && pe && step + 1 < pe_rows), "%s: next-row embedding needs emb, pe and pe row %d", name, step + 1);
    SBL_REQUIRE(sbl_aligned16(y) && sbl_aligned16(w), "%s: unaligned", name);
#define BEAM_TAIL_ARGS                                                                                                          \
    y, ldy, w, log_prior, score, last_tok, anc_old, anc_new, lda, hist_tok, hist_par, hist_score, hist_flag, end_score, end_ref, \
        end_count, step, maxlen, eos, emb, pe, emb_scale, x_next, W, V, trie_mask, trie_first, P, node, clip_steps
    if (clip_steps)
        hipLaunchKernelGGL((beam_tail_kernel<false, true>), dim3(N), dim3(256), 0, (hipStream_t)stream, BEAM_TAIL_ARGS);
    else if (trie_mask)
        hipLaunchKernelGGL((beam_tail_kernel<true>), dim3(N), dim3(256), 0, (hipStream_t)stream, BEAM_TAIL_ARGS);
    else
        hipLaunchKernelGGL((beam_tail_kernel<false>), dim3(N), dim3(256), 0, (hipStream_t)stream, BEAM_TAIL_ARGS);
#undef BEAM_TAIL_ARGS
    SBL_LAUNCH_CHECK(name);
    return 0;
}

extern "C" int sbl_beam_tail(const float* y, long ldy, const float* w, const float* log_prior, float* score, int32_t* last_tok,
                             const int32_t* anc_old, int32_t* anc_new, long lda, int32_t* hist_tok, int32_t* hist_par,
                             float* hist_score, int32_t* hist_flag, float* end_score, int32_t* end_ref, int32_t* end_count, int step,
                             int maxlen, int eos, const float* emb, const float* pe, int pe_rows, float emb_scale, float* x_next,
                             int N, int W, int V, int D, sbl_stream_t stream) {
    return beam_tail_launch("sbl_beam_tail", y, ldy, w, log_prior, score, last_tok, anc_old, anc_new, lda, hist_tok, hist_par,
                            hist_score, hist_flag, end_score, end_ref, end_count, step, maxlen, eos, emb, pe, pe_rows, emb_scale,
                            x_next, N, W, V, D, nullptr, nullptr, 0, nullptr, stream);
}

extern "C" int sbl_beam_tail_lex(const float* y, long ldy, const float* w, const float* log_prior, float* score, int32_t* last_tok,
                                 const int32_t* anc_old, int32_t* anc_new, long lda, int32_t* hist_tok, int32_t* hist_par,
                                 float* hist_score, int32_t* hist_flag, float* end_score, int32_t* end_ref, int32_t* end_count,
                                 int step, int maxlen, int eos, const float* emb, const float* pe, int pe_rows, float emb_scale,
                                 float* x_next, int N, int W, int V, int D, const int64_t* trie_mask, const int32_t* trie_first,
                                 int P, int32_t* node, sbl_stream_t stream) {
    SBL_REQUIRE(P >= 1, "sbl_beam_tail_lex: P=%d trie nodes", P);
    SBL_REQUIRE(trie_mask && trie_first && node, "sbl_beam_tail_lex: null trie table or node buffer");
    return beam_tail_launch("sbl_beam_tail_lex", y, ldy, w, log_prior, score, last_tok, anc_old, anc_new, lda, hist_tok, hist_par,
                            hist_score, hist_flag, end_score, end_ref, end_count, step, maxlen, eos, emb, pe, pe_rows, emb_scale,
                            x_next, N, W, V, D, trie_mask, trie_first, P, node, stream);
}

extern "C" int sbl_beam_tail_len(const float* y, long ldy, const float* w, const float* log_prior, float* score, int32_t* last_tok,
                                 const int32_t* anc_old, int32_t* anc_new, long lda, int32_t* hist_tok, int32_t* hist_par,
                                 float* hist_score, int32_t* hist_flag, float* end_score, int32_t* end_ref, int32_t* end_count,
                                 int step, int maxlen, int eos, const float* emb, const float* pe, int pe_rows, float emb_scale,
                                 float* x_next, int N, int W, int V, int D, const int32_t* clip_steps, sbl_stream_t stream) {
    SBL_REQUIRE(clip_steps, "sbl_beam_tail_len: clip_steps is NULL");
    return beam_tail_launch("sbl_beam_tail_len", y, ldy, w, log_prior, score, last_tok, anc_old, anc_new, lda, hist_tok, hist_par,
                            hist_score, hist_flag, end_score, end_ref, end_count, step, maxlen, eos, emb, pe, pe_rows, emb_scale,
                            x_next, N, W, V, D, nullptr, nullptr, 0, nullptr, stream, clip_steps);
}

// ------------------------------------------------------------------ n-best and back-trace: LRW1000/transformer/decoder.py:240-245
// grid N, one wavefront.  The ended list of a clip has at most W * maxlen <= 1024 entries = 16 per lane; nbest rounds of
// arg-max with the lower list position on equal scores are the stable descending sort truncated to nbest.
// LEN (sbl_beam_finish_len): the step whose hypotheses carry the appended <eos> is the clip's own last step.
template <bool LEN>
__global__ __launch_bounds__(64) void beam_finish_kernel(const float* __restrict__ end_score, const int32_t* __restrict__ end_ref,
                                                         const int32_t* __restrict__ end_count, const int32_t* __restrict__ hist_tok,
                                                         const int32_t* __restrict__ hist_par, int64_t* __restrict__ yseq,
                                                         int32_t* __restrict__ lengths, float* __restrict__ scores,
                                                         int32_t* __restrict__ n_hyps, int W, int maxlen, int nbest, int sos, int eos,
                                                         const int32_t* __restrict__ clip_steps) {
    const int lane = threadIdx.x;
    const int n = blockIdx.x;
    const int cap = W * maxlen;
    int E = end_count[n];
    E = E < 0 ? 0 : (E > cap ? cap : E);
    const float* es = end_score + (long)n * cap;
    unsigned taken = 0;
    float my_sc = -INFINITY;
    int my_e = DH_NONE;
    for (int k = 0; k < nbest; ++k) {
        float best = -INFINITY;
        int bi = DH_NONE;
        for (int t = 0; t * 64 + lane < E; ++t) {
            const float c = es[t * 64 + lane];
            if (!((taken >> t) & 1u) && (bi == DH_NONE || c > best)) {
                best = c;
                bi = t * 64 + lane;
            }
        }
        dh_wave_best(best, bi);
        if (bi != DH_NONE && (bi & 63) == lane) taken |= 1u << (bi >> 6);
        if (lane == k) {
            my_sc = best;
            my_e = bi;
        }
    }
    if (lane == 0) n_hyps[n] = E < nbest ? E : nbest;
    if (lane >= nbest) return;
    const int Ly = maxlen + 2;
    int64_t* row = yseq + ((long)n * nbest + lane) * Ly;
    for (int t = 0; t < Ly; ++t) row[t] = eos;
    if (my_e == DH_NONE) {      // fewer ended hypotheses than nbest
        lengths[n * nbest + lane] = 0;
        scores[n * nbest + lane] = -INFINITY;
        return;
    }
    const int ref = end_ref[(long)n * cap + my_e];
    int s = ref / W, r = ref - s * W;
    s = s < 0 ? 0 : (s >= maxlen ? maxlen - 1 : s);
    if constexpr (LEN) {
        const int l = clip_steps[n];
        const int last = (l < 1 ? 1 : (l > maxlen ? maxlen : l)) - 1;
        lengths[n * nbest + lane] = s == last ? s + 3 : s + 2;
    } else {
        lengths[n * nbest + lane] = s == maxlen - 1 ? maxlen + 2 : s + 2;      // <sos> + s+1 tokens (+ the last step's <eos>)
    }
    scores[n * nbest + lane] = my_sc;
    row[0] = sos;
    for (int t = s; t >= 0; --t) {
        r = r < 0 ? 0 : (r >= W ? W - 1 : r);
        const long hi = ((long)n * maxlen + t) * W + r;
        row[t + 1] = hist_tok[hi];
        r = hist_par[hi];
    }
}

static int beam_finish_launch(const char* name, const float* end_score, const int32_t* end_ref, const int32_t* end_count,
                              const int32_t* hist_tok, const int32_t* hist_par, int64_t* yseq, int32_t* lengths, float* scores,
                              int32_t* n_hyps, int N, int W, int maxlen, int nbest, int sos, int eos, const int32_t* clip_steps,
                              sbl_stream_t stream) {
    SBL_REQUIRE(W >= 1 && W <= DH_MAX_W, "%s: beam W=%d outside 1..%d", name, W, DH_MAX_W);
    SBL_REQUIRE(nbest >= 1 && nbest <= BEAM_MAX_NBEST, "%s: nbest=%d outside 1..%d", name, nbest, BEAM_MAX_NBEST);
    SBL_REQUIRE(maxlen >= 1 && maxlen <= BEAM_MAX_LEN, "%s: maxlen=%d outside 1..%d", name, maxlen, BEAM_MAX_LEN);
    SBL_REQUIRE(N > 0, "%s: N=%d", name, N);
    SBL_REQUIRE(end_score && end_ref && end_count && hist_tok && hist_par && yseq && lengths && scores && n_hyps, "%s: null pointer",
                name);
    if (clip_steps)
        hipLaunchKernelGGL(beam_finish_kernel<true>, dim3(N), dim3(64), 0, (hipStream_t)stream, end_score, end_ref, end_count, hist_tok,
                           hist_par, yseq, lengths, scores, n_hyps, W, maxlen, nbest, sos, eos, clip_steps);
    else
        hipLaunchKernelGGL(beam_finish_kernel<false>, dim3(N), dim3(64), 0, (hipStream_t)stream, end_score, end_ref, end_count, hist_tok,
                           hist_par, yseq, lengths, scores, n_hyps, W, maxlen, nbest, sos, eos, clip_steps);
    SBL_LAUNCH_CHECK(name);
    return 0;
}

extern "C" int sbl_beam_finish(const float* end_score, const int32_t* end_ref, const int32_t* end_count, const int32_t* hist_tok,
                               const int32_t* hist_par, int64_t* yseq, int32_t* lengths, float* scores, int32_t* n_hyps, int N, int W,
                               int maxlen, int nbest, int sos, int eos, sbl_stream_t stream) {
    return beam_finish_launch("sbl_beam_finish", end_score, end_ref, end_count, hist_tok, hist_par, yseq, lengths, scores, n_hyps, N, W,
                              maxlen, nbest, sos, eos, nullptr, stream);
}

extern "C" int sbl_beam_finish_len(const float* end_score, const int32_t* end_ref, const int32_t* end_count, const int32_t* hist_tok,
                                   const int32_t* hist_par, int64_t* yseq, int32_t* lengths, float* scores, int32_t* n_hyps, int N,
                                   int W, int maxlen, int nbest, int sos, int eos, const int32_t* clip_steps, sbl_stream_t stream) {
    SBL_REQUIRE(clip_steps, "sbl_beam_finish_len: clip_steps is NULL");
    return beam_finish_launch("sbl_beam_finish_len", end_score, end_ref, end_count, hist_tok, hist_par, yseq, lengths, scores, n_hyps, N,
                              W, maxlen, nbest, sos, eos, clip_steps, stream);
}
