// Beam search of the bidirectional SBL decoder: the step tail, one launch per step next to the per-step stage of
// transformer/decoder.py.
//
// A hypothesis is a PAIR - an l2r prefix and an r2l prefix that are fused with each other, as row b of the two directions is
// in the greedy decode (SBL/transformer/decoder.py:301-385).  A clip owns W = beam_size SLOTS, the batch is S = N * W pairs
// and every launch has that fixed shape; a slot that holds no live pair carries the total score -inf.  Nothing ends early:
// the model is trained on 16 positions with <eos> fed and predicted behind the end, so all pairs have the same length.
//
// One workgroup per clip:
//   1. the 2 * W projections to V <= 64 classes (plain fp32 FMA) and their log-softmax;
//   2. per slot and direction the W best classes, ordered (log-prob descending, token id ascending);
//   3. the clip's candidates (slot s, l2r rank ka, r2l rank kb), total = score[s] + (lpL[s][ka] + lpR[s][kb]) in fp32 in that
//      order, and the best W of them in descending total; exact ties go to the lower s, then the lower ka, then the lower kb.
//      fp32 addition is monotone, so a class outside a direction's W best is behind W candidates of its own slot and the W^3
//      pruned candidates give exactly the result of the exhaustive V^2 per slot.  For fixed (s, ka) the candidates fall with
//      kb, so the W^2 lists are merged by their heads: W rounds of one arg-max over at most 256 heads in one wavefront;
//   4. the candidate of rank r moves to slot r: scores, the prefixes ys_new[r] = ys_old[parent] || token (double-buffered:
//      the kernel reads the parents' rows), and the (step, rank) history.
// A candidate of total -inf (or NaN) is never kept; a rank without a candidate gets the scores -inf, <eos> tokens and its own
// rank as parent.
// The search restricted to a word list (sbl_pair_beam_tail_lex, Decoder.beam_search_lex) is the second kernel of this file: the
// same phases 1 and 4, candidates from the lexicon's pair trie in between.
#include "decode_head.h"

// ---- the phases that pair_beam_tail_kernel and pair_beam_tail_lex_kernel share: one body, so a constrained and an
// unconstrained total come from the same numbers.  All are called by the whole workgroup of 256 threads.

// logits of the clip's 2 * W rows into s_lp[direction][slot][class]: each wave takes every fourth (direction, class) and keeps
// its weight row in registers
__device__ __forceinline__ void pb_logits(float (*s_lp)[DH_MAX_W][64], const float* __restrict__ y_l, const float* __restrict__ y_r,
                                          long ldy, const float* __restrict__ w_l, const float* __restrict__ w_r, long slot0, int W,
                                          int V) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int idx = wave; idx < 2 * V; idx += 4) {
        const int d = idx >= V, v = idx - d * V;
        const float4* wr = reinterpret_cast<const float4*>((d ? w_r : w_l) + (long)v * DH_D);
        const float4 a = wr[lane], c = wr[64 + lane];
        const float* y = d ? y_r : y_l;
        for (int r = 0; r < W; ++r) {
            const float acc = dh_row_dot(reinterpret_cast<const float4*>(y + (slot0 + r) * ldy), a, c, lane);
            if (lane == 0) s_lp[d][r][v] = acc;
        }
    }
}

// log-softmax of the row (direction d, slot r) of s_lp by one wavefront, lane = class: the lane's log-prob (-inf past V)
__device__ __forceinline__ float pb_row_log_softmax(const float (*s_lp)[DH_MAX_W][64], int d, int r, int V) {
    const int lane = threadIdx.x & 63;
    const float l = lane < V ? s_lp[d][r][lane] : -INFINITY;
    return dh_log_softmax(l, lane < V);
}

// the new prefixes: the parent's tokens 0 .. step, the new token, <eos> behind it
__device__ __forceinline__ void pb_write_prefixes(const int64_t* __restrict__ ys_old_l, const int64_t* __restrict__ ys_old_r,
                                                  int64_t* __restrict__ ys_new_l, int64_t* __restrict__ ys_new_r, long ldys, long slot0,
                                                  const int* s_par, const int (*s_tok)[DH_MAX_W], int step, int maxlen, int eos,
                                                  int W) {
    const int len = maxlen + 1;
    for (int i = threadIdx.x; i < 2 * W * len; i += 256) {
        const int d = i >= W * len, rem = i - d * W * len;
        const int r = rem / len, j = rem - r * len;
        const int64_t* old = d ? ys_old_r : ys_old_l;
        int64_t* out = d ? ys_new_r : ys_new_l;
        int64_t t = eos;
        if (j <= step) t = old[(slot0 + s_par[r]) * ldys + j];
        else if (j == step + 1) t = s_tok[d][r];
        out[(slot0 + r) * ldys + j] = t;
    }
}

// grid N, 256 threads.  Slot n*W + r is beam position r of clip n.
__global__ __launch_bounds__(256) void pair_beam_tail_kernel(
    const float* __restrict__ y_l, const float* __restrict__ y_r, long ldy, const float* __restrict__ w_l,
    const float* __restrict__ w_r, float* score, float* score_dir, const int64_t* __restrict__ ys_old_l,
    const int64_t* __restrict__ ys_old_r, int64_t* __restrict__ ys_new_l, int64_t* __restrict__ ys_new_r, long ldys,
    int32_t* __restrict__ hist_tok_l, int32_t* __restrict__ hist_tok_r, int32_t* __restrict__ hist_par,
    float* __restrict__ hist_score, int step, int maxlen, int eos, int W, int V) {
    __shared__ float s_lp[2][DH_MAX_W][64];                  // [direction][slot][class]: logits
    __shared__ float s_top[2][DH_MAX_W][DH_MAX_W];           // [direction][slot][rank]: log-prob of the slot's rank-th class
    __shared__ int s_ttok[2][DH_MAX_W][DH_MAX_W];            // ... and the class
    __shared__ float s_sc[DH_MAX_W], s_sd[2][DH_MAX_W];      // the slots' scores on entry
    __shared__ int s_par[DH_MAX_W], s_tok[2][DH_MAX_W];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x;
    const long slot0 = (long)n * W;

    if (threadIdx.x < W) {
        s_sc[threadIdx.x] = score[slot0 + threadIdx.x];
        s_sd[0][threadIdx.x] = score_dir[(slot0 + threadIdx.x) * 2];
        s_sd[1][threadIdx.x] = score_dir[(slot0 + threadIdx.x) * 2 + 1];
    }
    pb_logits(s_lp, y_l, y_r, ldy, w_l, w_r, slot0, W, V);
    __syncthreads();
    // log-softmax of every row (lane = class) and its W best classes: W rounds of arg-max, the lower class on equal values
    for (int row = wave; row < 2 * W; row += 4) {
        const int d = row >= W, r = row - d * W;
        const float lp = pb_row_log_softmax(s_lp, d, r, V);
        bool used = lane >= V;
        float top = -INFINITY;
        int ttok = eos;
        for (int k = 0; k < W; ++k) {
            float best = used ? -INFINITY : lp;
            int bi = used ? DH_NONE : lane;
            dh_wave_best(best, bi);
            if (bi == lane) used = true;
            if (lane == k && bi != DH_NONE) {
                top = best;
                ttok = bi;
            }
        }
        if (lane < W) {
            s_top[d][r][lane] = top;
            s_ttok[d][r][lane] = ttok;
        }
    }
    __syncthreads();
    if (wave == 0) {
        // list t = s * W + ka holds the candidates (s, ka, kb = 0 .. W-1) in falling order; lane owns the lists lane + 64 q.
        // Candidate index = t * W + kb, so "lower index on ties" is the documented order.
        const int nlist = W * W;
        float base_s[4], base_a[4], head[4];
        int ptr[4], ls[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int t = lane + 64 * q;
            ptr[q] = 0;
            ls[q] = 0;
            base_s[q] = -INFINITY;
            base_a[q] = 0.f;
            head[q] = -INFINITY;
            if (t < nlist) {
                ls[q] = t / W;
                base_s[q] = s_sc[ls[q]];
                base_a[q] = s_top[0][ls[q]][t - ls[q] * W];
                const float c = base_s[q] + (base_a[q] + s_top[1][ls[q]][0]);
                head[q] = c > -INFINITY ? c : -INFINITY;
            }
        }
        float my_sc = -INFINITY;
        int my_idx = DH_NONE;
        for (int r = 0; r < W; ++r) {
            float best = -INFINITY;
            int bi = DH_NONE;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (head[q] > best) {
                    best = head[q];
                    bi = (lane + 64 * q) * W + ptr[q];
                }
            dh_wave_best(best, bi);
            if (lane == r) {
                my_sc = best;
                my_idx = bi;
            }
            if (bi != DH_NONE) {
                const int t = bi / W;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (t == lane + 64 * q) {      // the winner's list moves to its next candidate
                        ptr[q] += 1;
                        head[q] = -INFINITY;
                        if (ptr[q] < W) {
                            const float c = base_s[q] + (base_a[q] + s_top[1][ls[q]][ptr[q]]);
                            head[q] = c > -INFINITY ? c : -INFINITY;
                        }
                    }
            }
        }
        if (lane < W) {
            const bool kept = my_idx != DH_NONE;
            int par = lane, tl = eos, tr = eos;
            float sl = -INFINITY, sr = -INFINITY;
            if (kept) {
                const int t = my_idx / W, kb = my_idx - t * W;
                par = t / W;
                const int ka = t - par * W;
                tl = s_ttok[0][par][ka];
                tr = s_ttok[1][par][kb];
                sl = s_sd[0][par] + s_top[0][par][ka];
                sr = s_sd[1][par] + s_top[1][par][kb];
            }
            const float sc = kept ? my_sc : -INFINITY;
            score[slot0 + lane] = sc;
            score_dir[(slot0 + lane) * 2] = sl;
            score_dir[(slot0 + lane) * 2 + 1] = sr;
            const long hi = ((long)n * maxlen + step) * W + lane;
            hist_tok_l[hi] = tl;
            hist_tok_r[hi] = tr;
            hist_par[hi] = par;
            hist_score[hi] = sc;
            s_par[lane] = par;
            s_tok[0][lane] = tl;
            s_tok[1][lane] = tr;
        }
    }
    __syncthreads();
    pb_write_prefixes(ys_old_l, ys_old_r, ys_new_l, ys_new_r, ldys, slot0, s_par, s_tok, step, maxlen, eos, W);
}

// The requirements the two entries share, refused under the entry's `name`.  hist_extra: one more output that must not be null
// (the lex entry's hist_node; the plain entry passes one of its own again).
static int pair_beam_tail_check(const char* name, const float* y_l, const float* y_r, long ldy, const float* w_l, const float* w_r,
                                const float* score, const float* score_dir, const int64_t* ys_old_l, const int64_t* ys_old_r,
                                const int64_t* ys_new_l, const int64_t* ys_new_r, long ldys, const int32_t* hist_tok_l,
                                const int32_t* hist_tok_r, const int32_t* hist_par, const float* hist_score,
                                const int32_t* hist_extra, int step, int maxlen, int eos, int N, int W, int V, int D) {
    SBL_REQUIRE(D == DH_D, "%s: D=%d (built for %d)", name, D, DH_D);
    SBL_REQUIRE(V >= 1 && V <= DH_MAX_V, "%s: V=%d (V <= %d)", name, V, DH_MAX_V);
    SBL_REQUIRE(W >= 1 && W <= DH_MAX_W, "%s: beam W=%d outside 1..%d", name, W, DH_MAX_W);
    SBL_REQUIRE(W <= V, "%s: beam W=%d above V=%d", name, W, V);
    SBL_REQUIRE(N > 0 && maxlen >= 1 && step >= 0 && step < maxlen, "%s: N=%d, step %d of %d", name, N, step, maxlen);
    SBL_REQUIRE(eos >= 0 && eos < V, "%s: eos=%d outside the %d classes", name, eos, V);
    SBL_REQUIRE(ldys >= maxlen + 1, "%s: prefix rows of %ld entries for maxlen=%d (+1)", name, ldys, maxlen);
    SBL_REQUIRE(y_l && y_r && w_l && w_r && score && score_dir, "%s: null input", name);
    SBL_REQUIRE(ys_old_l && ys_old_r && ys_new_l && ys_new_r && ys_old_l != ys_new_l && ys_old_r != ys_new_r,
                "%s: null or aliased prefix buffers", name);
    SBL_REQUIRE(hist_tok_l && hist_tok_r && hist_par && hist_score && hist_extra, "%s: null output", name);
    SBL_REQUIRE(ldy >= D && ldy % 4 == 0, "%s: row stride %ld", name, ldy);
    SBL_REQUIRE(sbl_aligned16(y_l) && sbl_aligned16(y_r) && sbl_aligned16(w_l) && sbl_aligned16(w_r), "%s: unaligned", name);
    return 0;
}

extern "C" int sbl_pair_beam_tail(const float* y_l, const float* y_r, long ldy, const float* w_l, const float* w_r, float* score,
                                  float* score_dir, const int64_t* ys_old_l, const int64_t* ys_old_r, int64_t* ys_new_l,
                                  int64_t* ys_new_r, long ldys, int32_t* hist_tok_l, int32_t* hist_tok_r, int32_t* hist_par,
                                  float* hist_score, int step, int maxlen, int eos, int N, int W, int V, int D,
                                  sbl_stream_t stream) {
    if (int rc = pair_beam_tail_check("sbl_pair_beam_tail", y_l, y_r, ldy, w_l, w_r, score, score_dir, ys_old_l, ys_old_r, ys_new_l,
                                      ys_new_r, ldys, hist_tok_l, hist_tok_r, hist_par, hist_score, hist_par, step, maxlen, eos, N, W,
                                      V, D))
        return rc;
    hipLaunchKernelGGL(pair_beam_tail_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, y_l, y_r, ldy, w_l, w_r, score, score_dir,
                       ys_old_l, ys_old_r, ys_new_l, ys_new_r, ldys, hist_tok_l, hist_tok_r, hist_par, hist_score, step, maxlen, eos,
                       W, V);
    SBL_LAUNCH_CHECK("sbl_pair_beam_tail");
    return 0;
}

// ------------------------------------------------------------------ the search restricted to a word list (sbl_pair_beam_tail_lex)
// Every slot carries a node of the lexicon's PAIR trie (include/sbl_hip.h): the state (w[:t], w[c-t:]) of one word after t
// steps, so the l2r row spells w and the r2l row reversed(w) and a hypothesis pair is one word.  The tables are CSR: the edges
// of node q are key[begin[q] .. begin[q+1]), key = a * 64 + b (a the l2r token, b the r2l token), ascending inside a node, and
// the child behind entry e is node e + 1 (breadth-first numbering).  word[q] >= 0 marks a terminal node.
//
// Phases 1 and 4 are those of pair_beam_tail_kernel (pb_logits, pb_row_log_softmax, pb_write_prefixes); between them:
//   2. the log-probs of all V classes stay in LDS (the log-softmax is not renormalised over the allowed tokens);
//   3. the candidates of live slot s at node q: ONE if word[q] >= 0 - the pair has ended; tokens (eos, eos), the total and
//      both direction scores carried unchanged (no add), node q - else one per entry e of q's range, total = score[s] +
//      (lpL[s][a] + lpR[s][b]) in fp32 in that order, node e + 1.  The clip's candidates are numbered j = 0, 1, ... slot by
//      slot and entry by entry, and the best W are taken by W rounds of a workgroup-wide arg-max in the order (total
//      descending, j ascending) - exact ties go to the lower slot, then the lower entry, i.e. the lower key.  A round's
//      candidates are those behind the previous round's winner in that order, so nothing is marked and no memory grows
//      with the candidate count: a thread walks j = tid, tid + 256, ..., finds (s, e) through the <= 16 slot offsets in LDS
//      and recomputes the total.  The root's up to 4096 children are 16 evaluations per thread and round.
// Robustness: nodes read from memory are clamped to 0 .. P-1 and begin values to 0 .. E (an empty or inverted range: no
// candidates); a key with a token >= V (or a negative key) is a -inf candidate; the node written is min(e + 1, P - 1).
__global__ __launch_bounds__(256) void pair_beam_tail_lex_kernel(
    const float* __restrict__ y_l, const float* __restrict__ y_r, long ldy, const float* __restrict__ w_l,
    const float* __restrict__ w_r, float* score, float* score_dir, const int64_t* __restrict__ ys_old_l,
    const int64_t* __restrict__ ys_old_r, int64_t* __restrict__ ys_new_l, int64_t* __restrict__ ys_new_r, long ldys,
    int32_t* __restrict__ hist_tok_l, int32_t* __restrict__ hist_tok_r, int32_t* __restrict__ hist_par,
    float* __restrict__ hist_score, int step, int maxlen, int eos, int W, int V, const int32_t* __restrict__ trie_begin,
    const int32_t* __restrict__ trie_key, const int32_t* __restrict__ trie_word, int P, int E,
    const int32_t* __restrict__ node_old, int32_t* __restrict__ node_new, int32_t* __restrict__ hist_node) {
    __shared__ float s_lp[2][DH_MAX_W][64];                  // [direction][slot][class]: logits, then log-probs
    __shared__ float s_sc[DH_MAX_W], s_sd[2][DH_MAX_W];      // the slots' scores on entry
    __shared__ int s_q[DH_MAX_W], s_b0[DH_MAX_W], s_off[DH_MAX_W + 1];      // node, first entry, candidate offset per slot
    __shared__ bool s_end[DH_MAX_W];
    __shared__ float s_rv[2][4], s_wv[DH_MAX_W];             // per-wave bests of a round (two buffers), the rounds' winners
    __shared__ int s_ri[2][4], s_wj[DH_MAX_W];
    __shared__ int s_par[DH_MAX_W], s_tok[2][DH_MAX_W];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x;
    const long slot0 = (long)n * W;

    if (threadIdx.x < W) {
        const int s = threadIdx.x;
        const float sc = score[slot0 + s];
        s_sc[s] = sc;
        s_sd[0][s] = score_dir[(slot0 + s) * 2];
        s_sd[1][s] = score_dir[(slot0 + s) * 2 + 1];
        const int q = min(max(node_old[slot0 + s], 0), P - 1);
        const bool ended = trie_word[q] >= 0;
        const int b0 = min(max(trie_begin[q], 0), E), b1 = min(max(trie_begin[q + 1], 0), E);
        s_q[s] = q;
        s_end[s] = ended;
        s_b0[s] = b0;
        s_off[s + 1] = !(sc > -INFINITY) ? 0 : ended ? 1 : max(b1 - b0, 0);      // a dead (or NaN) slot has no candidate
    }
    pb_logits(s_lp, y_l, y_r, ldy, w_l, w_r, slot0, W, V);
    __syncthreads();
    for (int row = wave; row < 2 * W; row += 4) {
        const int d = row >= W, r = row - d * W;
        const float lp = pb_row_log_softmax(s_lp, d, r, V);
        s_lp[d][r][lane] = lp;                               // the wave's own row: read above, then overwritten
    }
    if (threadIdx.x == 0) {
        int acc = 0;
        s_off[0] = 0;
        for (int s = 0; s < W; ++s) {
            acc += s_off[s + 1];
            s_off[s + 1] = acc;
        }
    }
    __syncthreads();
    const int total = s_off[W];
    float prev_v = INFINITY;                                 // the previous round's winner: everything is behind (+inf, -1)
    int prev_j = -1;
    for (int r = 0; r < W; ++r) {
        float best = -INFINITY;
        int bi = DH_NONE;
        if (r == 0 || prev_j != DH_NONE) {
            int s = 0;
            for (int j = threadIdx.x; j < total; j += 256) {
                while (j >= s_off[s + 1]) ++s;               // j < total = s_off[W]: ends at a slot s < W
                float t;
                if (s_end[s]) {
                    t = s_sc[s];
                } else {
                    const int k = trie_key[s_b0[s] + (j - s_off[s])];
                    const int a = k >> 6, b = k & 63;
                    t = (k >= 0 && a < V && b < V) ? s_sc[s] + (s_lp[0][s][a] + s_lp[1][s][b]) : -INFINITY;
                }
                const bool behind = t < prev_v || (t == prev_v && j > prev_j);
                if (t > -INFINITY && behind && t > best) {   // ascending j: the lower j stays on equal totals
                    best = t;
                    bi = j;
                }
            }
        }
        dh_wave_best(best, bi);
        if (lane == 0) {
            s_rv[r & 1][wave] = best;
            s_ri[r & 1][wave] = bi;
        }
        __syncthreads();
        best = s_rv[r & 1][0];
        bi = s_ri[r & 1][0];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float ov = s_rv[r & 1][w];
            const int oi = s_ri[r & 1][w];
            if (oi != DH_NONE && (bi == DH_NONE || ov > best || (ov == best && oi < bi))) {
                best = ov;
                bi = oi;
            }
        }
        prev_v = best;
        prev_j = bi;
        if (threadIdx.x == 0) {
            s_wv[r] = best;
            s_wj[r] = bi;
        }
    }
    __syncthreads();
    if (threadIdx.x < W) {
        const int r = threadIdx.x;
        const int j = s_wj[r];
        const bool kept = j != DH_NONE;
        int par = r, tl = eos, tr = eos, nd = 0;
        float sc = -INFINITY, sl = -INFINITY, sr = -INFINITY;
        if (kept) {
            par = 0;
            while (j >= s_off[par + 1]) ++par;
            sc = s_wv[r];
            if (s_end[par]) {                                // carried bit for bit
                sl = s_sd[0][par];
                sr = s_sd[1][par];
                nd = s_q[par];
            } else {
                const int e = s_b0[par] + (j - s_off[par]);
                const int k = trie_key[e];
                tl = k >> 6;
                tr = k & 63;
                sl = s_sd[0][par] + s_lp[0][par][tl];
                sr = s_sd[1][par] + s_lp[1][par][tr];
                nd = min(e + 1, P - 1);
            }
        }
        score[slot0 + r] = sc;
        score_dir[(slot0 + r) * 2] = sl;
        score_dir[(slot0 + r) * 2 + 1] = sr;
        node_new[slot0 + r] = nd;
        const long hi = ((long)n * maxlen + step) * W + r;
        hist_tok_l[hi] = tl;
        hist_tok_r[hi] = tr;
        hist_par[hi] = par;
        hist_score[hi] = sc;
        hist_node[hi] = nd;
        s_par[r] = par;
        s_tok[0][r] = tl;
        s_tok[1][r] = tr;
    }
    __syncthreads();
    pb_write_prefixes(ys_old_l, ys_old_r, ys_new_l, ys_new_r, ldys, slot0, s_par, s_tok, step, maxlen, eos, W);
}

extern "C" int sbl_pair_beam_tail_lex(const float* y_l, const float* y_r, long ldy, const float* w_l, const float* w_r,
                                      float* score, float* score_dir, const int64_t* ys_old_l, const int64_t* ys_old_r,
                                      int64_t* ys_new_l, int64_t* ys_new_r, long ldys, int32_t* hist_tok_l, int32_t* hist_tok_r,
                                      int32_t* hist_par, float* hist_score, int step, int maxlen, int eos, int N, int W, int V, int D,
                                      const int32_t* trie_begin, const int32_t* trie_key, const int32_t* trie_word, int P, int E,
                                      const int32_t* node_old, int32_t* node_new, int32_t* hist_node, sbl_stream_t stream) {
    if (int rc = pair_beam_tail_check("sbl_pair_beam_tail_lex", y_l, y_r, ldy, w_l, w_r, score, score_dir, ys_old_l, ys_old_r,
                                      ys_new_l, ys_new_r, ldys, hist_tok_l, hist_tok_r, hist_par, hist_score, hist_node, step, maxlen,
                                      eos, N, W, V, D))
        return rc;
    SBL_REQUIRE(P >= 1 && E >= 0, "sbl_pair_beam_tail_lex: P=%d trie nodes, E=%d edges", P, E);
    SBL_REQUIRE(trie_begin && trie_word && (trie_key || E == 0), "sbl_pair_beam_tail_lex: null trie table");
    SBL_REQUIRE(node_old && node_new && node_old != node_new, "sbl_pair_beam_tail_lex: null or aliased node buffers");
    hipLaunchKernelGGL(pair_beam_tail_lex_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, y_l, y_r, ldy, w_l, w_r, score,
                       score_dir, ys_old_l, ys_old_r, ys_new_l, ys_new_r, ldys, hist_tok_l, hist_tok_r, hist_par, hist_score, step,
                       maxlen, eos, W, V, trie_begin, trie_key, trie_word, P, E, node_old, node_new, hist_node);
    SBL_LAUNCH_CHECK("sbl_pair_beam_tail_lex");
    return 0;
}
