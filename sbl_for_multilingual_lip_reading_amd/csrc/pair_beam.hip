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
#include "decode_head.h"

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
    // logits of the clip's 2 * W rows: each wave takes every fourth (direction, class) and keeps its weight row in registers
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
    __syncthreads();
    // log-softmax of every row (lane = class) and its W best classes: W rounds of arg-max, the lower class on equal values
    for (int row = wave; row < 2 * W; row += 4) {
        const int d = row >= W, r = row - d * W;
        const float l = lane < V ? s_lp[d][r][lane] : -INFINITY;
        const float lp = dh_log_softmax(l, lane < V);
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
    // the new prefixes: the parent's tokens 0 .. step, the new token, <eos> behind it
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

extern "C" int sbl_pair_beam_tail(const float* y_l, const float* y_r, long ldy, const float* w_l, const float* w_r, float* score,
                                  float* score_dir, const int64_t* ys_old_l, const int64_t* ys_old_r, int64_t* ys_new_l,
                                  int64_t* ys_new_r, long ldys, int32_t* hist_tok_l, int32_t* hist_tok_r, int32_t* hist_par,
                                  float* hist_score, int step, int maxlen, int eos, int N, int W, int V, int D,
                                  sbl_stream_t stream) {
    SBL_REQUIRE(D == DH_D, "sbl_pair_beam_tail: D=%d (built for %d)", D, DH_D);
    SBL_REQUIRE(V >= 1 && V <= DH_MAX_V, "sbl_pair_beam_tail: V=%d (V <= %d)", V, DH_MAX_V);
    SBL_REQUIRE(W >= 1 && W <= DH_MAX_W, "sbl_pair_beam_tail: beam W=%d outside 1..%d", W, DH_MAX_W);
    SBL_REQUIRE(W <= V, "sbl_pair_beam_tail: beam W=%d above V=%d", W, V);
    SBL_REQUIRE(N > 0 && maxlen >= 1 && step >= 0 && step < maxlen, "sbl_pair_beam_tail: N=%d, step %d of %d", N, step, maxlen);
    SBL_REQUIRE(eos >= 0 && eos < V, "sbl_pair_beam_tail: eos=%d outside the %d classes", eos, V);
    SBL_REQUIRE(ldys >= maxlen + 1, "sbl_pair_beam_tail: prefix rows of %ld entries for maxlen=%d (+1)", ldys, maxlen);
    SBL_REQUIRE(y_l && y_r && w_l && w_r && score && score_dir, "sbl_pair_beam_tail: null input");
    SBL_REQUIRE(ys_old_l && ys_old_r && ys_new_l && ys_new_r && ys_old_l != ys_new_l && ys_old_r != ys_new_r,
                "sbl_pair_beam_tail: null or aliased prefix buffers");
    SBL_REQUIRE(hist_tok_l && hist_tok_r && hist_par && hist_score, "sbl_pair_beam_tail: null output");
    SBL_REQUIRE(ldy >= D && ldy % 4 == 0, "sbl_pair_beam_tail: row stride %ld", ldy);
    SBL_REQUIRE(sbl_aligned16(y_l) && sbl_aligned16(y_r) && sbl_aligned16(w_l) && sbl_aligned16(w_r), "sbl_pair_beam_tail: unaligned");
    hipLaunchKernelGGL(pair_beam_tail_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, y_l, y_r, ldy, w_l, w_r, score, score_dir,
                       ys_old_l, ys_old_r, ys_new_l, ys_new_r, ldys, hist_tok_l, hist_tok_r, hist_par, hist_score, step, maxlen, eos,
                       W, V);
    SBL_LAUNCH_CHECK("sbl_pair_beam_tail");
    return 0;
}
