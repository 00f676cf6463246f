// Batched beam search of the single-direction seq2seq decoder (LRW1000/transformer/decoder.py:131-245), three kernels
// next to the greedy step of decode_step.hip.
//
// The reference decodes one clip at a time and re-runs the whole prefix of every hypothesis at every step.  Here a clip
// owns W = beam_size SLOTS, the batch is S = N * W rows, and every launch has that fixed shape: a slot that holds no live
// hypothesis carries the score -inf (its rows are computed and never selected).  All live hypotheses of a clip have the
// same length at step i, so the K / V cache of decode_step.hip carries over with one addition: a hypothesis changes its
// parent at every step, and instead of copying cache rows between slots each slot keeps an ANCESTRY row - anc[b][j] is
// the slot whose cache row j holds key j of the hypothesis now living in slot b.
//   * beam_attn_kernel: decode_attn_kernel with the cache slot of key j looked up in anc (score and value pass); the new
//     row is stored at row n_prev of the slot's OWN cache and used from registers.  Rows j < n_prev of every slot were
//     written at step j and are never written again, so no launch reads a row that the same launch writes.
//   * beam_tail_kernel: one workgroup per clip: the W projections to V <= 64 classes, log-softmax, + log-prior row of the
//     slot's last token + the slot's score, the best W of the W * V candidates, the hypotheses that end, the new ancestry
//     rows (double-buffered: the kernel reads the parents' rows), the (step, rank) history, and the next input rows.
//   * beam_finish_kernel: one wavefront per clip: the nbest best ended hypotheses (stable), traced back through the history.
// Ties (the reference leaves them to torch.topk and a stable sort): the lower parent slot first, then the lower token id;
// in the final list the hypothesis that ended first (earlier step, then better rank).
// A candidate of score -inf (a bigram of frequency zero) is never kept: the reference would carry it as a hypothesis of
// score -inf that can only ever surface behind every finite one.
#include "sbl_common.h"

#define BEAM_D 512          // d_model of the decoder (host-checked)
#define BEAM_MAX_KEYS 64    // one key per lane
#define BEAM_MAX_W 16
#define BEAM_MAX_V 64       // one class per lane
#define BEAM_MAX_LEN 64
#define BEAM_MAX_NBEST 16
#define BEAM_NONE 0x7fffffff

// ------------------------------------------------------------------ single-query attention over the slots' K / V caches
// grid (H, S), one wavefront each.  append: keys 0 .. n_prev-1 are row j of cache slot anc[b][j] (clamped to 0 .. S-1, so
// whatever the table holds the reads stay inside the (S, Lcap) rows), plus the new row, stored at row n_prev of slot b.
// No append (cross-attention): slot b reads rows 0 .. n_prev-1 of the hoisted cache of clip b / W, of which there are S / W.
// n_prev + append <= Lcap <= 64 is checked on the host.
__global__ __launch_bounds__(64) void beam_attn_kernel(const float* __restrict__ q, long ldq, const float* __restrict__ k_new,
                                                       const float* __restrict__ v_new, long ldn, float* k_cache, float* v_cache,
                                                       long ldc, int Lcap, const int32_t* __restrict__ anc, long lda,
                                                       float* __restrict__ o, long ldo, int S, int W, int n_prev, int append,
                                                       float scale) {
    const int lane = threadIdx.x;
    const int h = blockIdx.x, b = blockIdx.y;
    const long col = (long)h * 64;
    const float* qrow = q + (long)b * ldq + col;
    int src = append ? b : b / W;      // the cache slot of key `lane`
    if (append && lane < n_prev) {
        src = anc[(long)b * lda + lane];
        src = src < 0 ? 0 : (src >= S ? S - 1 : src);
    }

    float s = -INFINITY;
    if (lane < n_prev) {
        const float4* kr = reinterpret_cast<const float4*>(k_cache + ((long)src * Lcap + lane) * ldc + col);
        const float4* q4 = reinterpret_cast<const float4*>(qrow);
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const float4 a = q4[t], c = kr[t];
            acc += a.x * c.x + a.y * c.y + a.z * c.z + a.w * c.w;
        }
        s = acc * scale;
    }
    float vn = 0.f;
    if (append) {      // (uniform) the new row: lane d holds column d; its score is one wave reduction
        const float kn = k_new[(long)b * ldn + col + lane];
        vn = v_new[(long)b * ldn + col + lane];
        const long own = ((long)b * Lcap + n_prev) * ldc + col + lane;
        k_cache[own] = kn;
        v_cache[own] = vn;
        const float sn = wave_sum(qrow[lane] * kn) * scale;
        if (lane == n_prev) s = sn;
    }
    const float m = wave_max(s);
    const float e = s == -INFINITY ? 0.f : __expf(s - m);
    const float p = e / wave_sum(e);

    float acc = 0.f;
    for (int j = 0; j < n_prev; ++j) {
        const int sj = __shfl(src, j, 64);
        acc += __shfl(p, j, 64) * v_cache[((long)sj * Lcap + j) * ldc + col + lane];
    }
    if (append) acc += __shfl(p, n_prev, 64) * vn;
    o[(long)b * ldo + col + lane] = acc;
}

extern "C" int sbl_beam_attn_step(const float* q, long ldq, const float* k_new, const float* v_new, long ldn, float* k_cache,
                                  float* v_cache, long ldc, int Lcap, const int32_t* anc, long lda, float* o, long ldo, int S,
                                  int W, int H, int n_prev, int append, float scale, sbl_stream_t stream) {
    SBL_REQUIRE(W >= 1 && W <= BEAM_MAX_W, "sbl_beam_attn_step: beam W=%d outside 1..%d", W, BEAM_MAX_W);
    SBL_REQUIRE(S > 0 && H > 0 && S <= 65535 && S % W == 0, "sbl_beam_attn_step: S=%d H=%d (S a multiple of W=%d)", S, H, W);
    SBL_REQUIRE(Lcap >= 1 && Lcap <= BEAM_MAX_KEYS, "sbl_beam_attn_step: Lcap=%d outside 1..%d", Lcap, BEAM_MAX_KEYS);
    SBL_REQUIRE(append == 0 || append == 1, "sbl_beam_attn_step: append=%d", append);
    SBL_REQUIRE(n_prev >= 0 && n_prev + append >= 1 && n_prev + append <= Lcap,
                "sbl_beam_attn_step: %d cached keys (+%d) do not fit Lcap=%d", n_prev, append, Lcap);
    SBL_REQUIRE(q && k_cache && v_cache && o, "sbl_beam_attn_step: null pointer");
    SBL_REQUIRE(!append || (k_new && v_new && ldn >= (long)H * 64), "sbl_beam_attn_step: new K/V row missing");
    SBL_REQUIRE(!append || n_prev == 0 || (anc && lda >= n_prev), "sbl_beam_attn_step: ancestry rows of %ld entries for %d keys",
                lda, n_prev);
    SBL_REQUIRE(ldq >= (long)H * 64 && ldc >= (long)H * 64 && ldo >= (long)H * 64, "sbl_beam_attn_step: row stride below H*64");
    SBL_REQUIRE(ldq % 4 == 0 && ldc % 4 == 0 && sbl_aligned16(q) && sbl_aligned16(k_cache), "sbl_beam_attn_step: unaligned");
    hipLaunchKernelGGL(beam_attn_kernel, dim3(H, S), dim3(64), 0, (hipStream_t)stream, q, ldq, k_new, v_new, ldn, k_cache, v_cache,
                       ldc, Lcap, anc, lda, o, ldo, S, W, n_prev, append, scale);
    SBL_LAUNCH_CHECK("sbl_beam_attn_step");
    return 0;
}

// (value, index) maximum over the wave with the lower index on equal values; BEAM_NONE = nothing to offer.  Every lane
// ends with the same pair.
__device__ __forceinline__ void beam_wave_best(float& best, int& bi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oi != BEAM_NONE && (bi == BEAM_NONE || ov > best || (ov == best && oi < bi))) {
            best = ov;
            bi = oi;
        }
    }
}

// ------------------------------------------------------------------ beam tail: LRW1000/transformer/decoder.py:186-229
// grid N, 256 threads.  Slot n*W + r is beam position r of clip n.  Flags: 0 = nothing kept at this rank, 1 = live, 2 = ended.
__global__ __launch_bounds__(256) void beam_tail_kernel(
    const float* __restrict__ y, long ldy, const float* __restrict__ w, const float* __restrict__ log_prior, float* score,
    int32_t* last_tok, const int32_t* __restrict__ anc_old, int32_t* __restrict__ anc_new, long lda, int32_t* __restrict__ hist_tok,
    int32_t* __restrict__ hist_par, float* __restrict__ hist_score, int32_t* __restrict__ hist_flag, float* __restrict__ end_score,
    int32_t* __restrict__ end_ref, int32_t* end_count, int step, int maxlen, int eos, const float* __restrict__ emb,
    const float* __restrict__ pe, float emb_scale, float* __restrict__ x_next, int W, int V) {
    __shared__ float s_cand[BEAM_MAX_W * 64];
    __shared__ int s_tok[BEAM_MAX_W], s_par[BEAM_MAX_W];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x;
    const long slot0 = (long)n * W;

    // logits of the clip's W rows: each wave takes every fourth class and keeps its weight row in registers
    for (int v = wave; v < V; v += 4) {
        const float4* wr = reinterpret_cast<const float4*>(w + (long)v * BEAM_D);
        const float4 a = wr[lane], c = wr[64 + lane];
        for (int r = 0; r < W; ++r) {
            const float4* yr = reinterpret_cast<const float4*>(y + (slot0 + r) * ldy);
            const float4 y0 = yr[lane], y1 = yr[64 + lane];
            float acc = y0.x * a.x + y0.y * a.y + y0.z * a.z + y0.w * a.w;
            acc += y1.x * c.x + y1.y * c.y + y1.z * c.z + y1.w * c.w;
            acc = wave_sum(acc);
            if (lane == 0) s_cand[r * 64 + v] = acc;
        }
    }
    __syncthreads();
    // candidates: score + (log_softmax(logits) + log_prior[last token]), lane = class; a dead slot offers nothing
    for (int r = wave; r < W; r += 4) {
        const float sc = score[slot0 + r];
        int lt = last_tok[slot0 + r];
        lt = lt < 0 ? 0 : (lt >= V ? V - 1 : lt);
        const float l = lane < V ? s_cand[r * 64 + lane] : -INFINITY;
        const float m = wave_max(l);
        const float lse = logf(wave_sum(lane < V ? expf(l - m) : 0.f));
        float c = -INFINITY;
        if (lane < V && sc > -INFINITY) {
            float local = (l - m) - lse;
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
        int my_idx = BEAM_NONE;
        for (int r = 0; r < W; ++r) {
            float best = -INFINITY;
            int bi = BEAM_NONE;
            for (int t = 0; t < W; ++t) {
                const float c = s_cand[t * 64 + lane];
                if (!((taken >> t) & 1u) && c > best) {
                    best = c;
                    bi = t * 64 + lane;
                }
            }
            beam_wave_best(best, bi);
            if (bi != BEAM_NONE && (bi & 63) == lane) taken |= 1u << (bi >> 6);
            if (lane == r) {
                my_sc = best;
                my_idx = bi;
            }
        }
        const bool kept = lane < W && my_idx != BEAM_NONE;
        const int tok = kept ? (my_idx & 63) : eos;
        const int par = kept ? (my_idx >> 6) : lane;
        // decoder.py:213-218: at the last step every kept hypothesis gets an <eos> appended, one that ends in <eos> included
        const bool ended = kept && (tok == eos || step == maxlen - 1);
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
    if (x_next) {      // (uniform) the next step's input rows
        const float* pr = pe + (long)(step + 1) * BEAM_D;
        for (int r = 0; r < W; ++r) {
            const float* er = emb + (long)s_tok[r] * BEAM_D;
            for (int d = threadIdx.x; d < BEAM_D; d += 256) x_next[(slot0 + r) * BEAM_D + d] = er[d] * emb_scale + pr[d];
        }
    }
}

extern "C" int sbl_beam_tail(const float* y, long ldy, const float* w, const float* log_prior, float* score, int32_t* last_tok,
                             const int32_t* anc_old, int32_t* anc_new, long lda, int32_t* hist_tok, int32_t* hist_par,
                             float* hist_score, int32_t* hist_flag, float* end_score, int32_t* end_ref, int32_t* end_count, int step,
                             int maxlen, int eos, const float* emb, const float* pe, int pe_rows, float emb_scale, float* x_next,
                             int N, int W, int V, int D, sbl_stream_t stream) {
    SBL_REQUIRE(D == BEAM_D, "sbl_beam_tail: D=%d (built for %d)", D, BEAM_D);
    SBL_REQUIRE(V >= 1 && V <= BEAM_MAX_V, "sbl_beam_tail: V=%d (V <= %d)", V, BEAM_MAX_V);
    SBL_REQUIRE(W >= 1 && W <= BEAM_MAX_W, "sbl_beam_tail: beam W=%d outside 1..%d", W, BEAM_MAX_W);
    SBL_REQUIRE(W <= V, "sbl_beam_tail: beam W=%d above V=%d", W, V);
    SBL_REQUIRE(maxlen >= 1 && maxlen <= BEAM_MAX_LEN, "sbl_beam_tail: maxlen=%d outside 1..%d", maxlen, BEAM_MAX_LEN);
    SBL_REQUIRE(N > 0 && step >= 0 && step < maxlen, "sbl_beam_tail: N=%d, step %d of %d", N, step, maxlen);
    SBL_REQUIRE(eos >= 0 && eos < V, "sbl_beam_tail: eos=%d outside the %d classes", eos, V);
    SBL_REQUIRE(lda >= maxlen, "sbl_beam_tail: ancestry rows of %ld entries for maxlen=%d", lda, maxlen);
    SBL_REQUIRE(y && w && score && last_tok && anc_old && anc_new && anc_old != anc_new, "sbl_beam_tail: null or aliased state");
    SBL_REQUIRE(hist_tok && hist_par && hist_score && hist_flag && end_score && end_ref && end_count, "sbl_beam_tail: null output");
    SBL_REQUIRE(ldy >= D && ldy % 4 == 0, "sbl_beam_tail: row stride %ld", ldy);
    SBL_REQUIRE(!x_next || (emb && pe && step + 1 < pe_rows), "sbl_beam_tail: next-row embedding needs emb, pe and pe row %d",
                step + 1);
    SBL_REQUIRE(sbl_aligned16(y) && sbl_aligned16(w), "sbl_beam_tail: unaligned");
    hipLaunchKernelGGL(beam_tail_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, y, ldy, w, log_prior, score, last_tok, anc_old,
                       anc_new, lda, hist_tok, hist_par, hist_score, hist_flag, end_score, end_ref, end_count, step, maxlen, eos, emb,
                       pe, emb_scale, x_next, W, V);
    SBL_LAUNCH_CHECK("sbl_beam_tail");
    return 0;
}

// ------------------------------------------------------------------ n-best and back-trace: LRW1000/transformer/decoder.py:240-245
// grid N, one wavefront.  The ended list of a clip has at most W * maxlen <= 1024 entries = 16 per lane; nbest rounds of
// arg-max with the lower list position on equal scores are the stable descending sort truncated to nbest.
__global__ __launch_bounds__(64) void beam_finish_kernel(const float* __restrict__ end_score, const int32_t* __restrict__ end_ref,
                                                         const int32_t* __restrict__ end_count, const int32_t* __restrict__ hist_tok,
                                                         const int32_t* __restrict__ hist_par, int64_t* __restrict__ yseq,
                                                         int32_t* __restrict__ lengths, float* __restrict__ scores,
                                                         int32_t* __restrict__ n_hyps, int W, int maxlen, int nbest, int sos, int eos) {
    const int lane = threadIdx.x;
    const int n = blockIdx.x;
    const int cap = W * maxlen;
    int E = end_count[n];
    E = E < 0 ? 0 : (E > cap ? cap : E);
    const float* es = end_score + (long)n * cap;
    unsigned taken = 0;
    float my_sc = -INFINITY;
    int my_e = BEAM_NONE;
    for (int k = 0; k < nbest; ++k) {
        float best = -INFINITY;
        int bi = BEAM_NONE;
        for (int t = 0; t * 64 + lane < E; ++t) {
            const float c = es[t * 64 + lane];
            if (!((taken >> t) & 1u) && (bi == BEAM_NONE || c > best)) {
                best = c;
                bi = t * 64 + lane;
            }
        }
        beam_wave_best(best, bi);
        if (bi != BEAM_NONE && (bi & 63) == lane) taken |= 1u << (bi >> 6);
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
    if (my_e == BEAM_NONE) {      // fewer ended hypotheses than nbest
        lengths[n * nbest + lane] = 0;
        scores[n * nbest + lane] = -INFINITY;
        return;
    }
    const int ref = end_ref[(long)n * cap + my_e];
    int s = ref / W, r = ref - s * W;
    s = s < 0 ? 0 : (s >= maxlen ? maxlen - 1 : s);
    lengths[n * nbest + lane] = s == maxlen - 1 ? maxlen + 2 : s + 2;      // <sos> + s+1 tokens (+ the last step's <eos>)
    scores[n * nbest + lane] = my_sc;
    row[0] = sos;
    for (int t = s; t >= 0; --t) {
        r = r < 0 ? 0 : (r >= W ? W - 1 : r);
        const long hi = ((long)n * maxlen + t) * W + r;
        row[t + 1] = hist_tok[hi];
        r = hist_par[hi];
    }
}

extern "C" int sbl_beam_finish(const float* end_score, const int32_t* end_ref, const int32_t* end_count, const int32_t* hist_tok,
                               const int32_t* hist_par, int64_t* yseq, int32_t* lengths, float* scores, int32_t* n_hyps, int N, int W,
                               int maxlen, int nbest, int sos, int eos, sbl_stream_t stream) {
    SBL_REQUIRE(W >= 1 && W <= BEAM_MAX_W, "sbl_beam_finish: beam W=%d outside 1..%d", W, BEAM_MAX_W);
    SBL_REQUIRE(nbest >= 1 && nbest <= BEAM_MAX_NBEST, "sbl_beam_finish: nbest=%d outside 1..%d", nbest, BEAM_MAX_NBEST);
    SBL_REQUIRE(maxlen >= 1 && maxlen <= BEAM_MAX_LEN, "sbl_beam_finish: maxlen=%d outside 1..%d", maxlen, BEAM_MAX_LEN);
    SBL_REQUIRE(N > 0, "sbl_beam_finish: N=%d", N);
    SBL_REQUIRE(end_score && end_ref && end_count && hist_tok && hist_par && yseq && lengths && scores && n_hyps,
                "sbl_beam_finish: null pointer");
    hipLaunchKernelGGL(beam_finish_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, end_score, end_ref, end_count, hist_tok,
                       hist_par, yseq, lengths, scores, n_hyps, W, maxlen, nbest, sos, eos);
    SBL_LAUNCH_CHECK("sbl_beam_finish");
    return 0;
}
