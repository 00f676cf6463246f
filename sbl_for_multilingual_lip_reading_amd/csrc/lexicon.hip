// Closed-vocabulary word decode: the last stage of recognition on LRW / LRW1000, whose labels are 500 / 1000 words.  The
// reference can only ask whether the joined phoneme string equals the gold string (SBL/train.py:28-38, SBL/test.py:185-218);
// here the decoder's hypotheses are mapped onto the lexicon and the model chooses between the close words.  Two launches around
// one batched decoder stage (Decoder.score_pairs); the definitions are in include/sbl_hip.h.
//
// sbl_lexicon_shortlist - one workgroup per clip, lanes stride over the words.  A word is 16 bytes (15 token bytes and its
// length), one 128-bit load.  The clip's 2 H hypothesis rows are compacted once per workgroup into LDS (the r2l one reversed:
// lev(p_r, reversed(w)) = lev(reversed(p_r), w), so both directions run against the same word registers); every lane reads
// them as broadcasts.  The dynamic program is score.hip's: the row lives in registers with compile-time indices and the
// columns behind the word's end are transparent (they copy their left neighbour), so the distance is always the last entry.
// A lane keeps the best (D, h) of each of its words as one integer key D << 20 | h << 16 | w in a sorted list of the K
// smallest (compare-exchange with static indices); the clip's K best are then K rounds of a block-wide minimum - wave64
// shuffles, then LDS - in which the winner pops its list.  Keys are distinct integers: no float, no atomics, no order
// dependence.
//
// sbl_pair_score_tail - one workgroup per group of G slots.  For every step the 2 G rows go through the heads and the
// log-softmax of decode_head.h (the code of sbl_pair_beam_tail) and the log-probability of the slot's own token is kept; one lane
// per slot then adds them in ascending step order, the order of the beam search's totals.
//
// sbl_lexicon_lookup - one thread per hypothesis row: the exact walk through the lexicon's trie, the tables the constrained
// beam tail (sbl_beam_tail_lex, beam_step.hip) reads.  It names the words of that search's n-best and is an exact-match lookup.
#include "decode_head.h"

#define LX_THREADS 1024
#define LX_WAVES (LX_THREADS / 64)
#define LX_MAX_H 16
#define LX_MAX_K 16
#define LX_WORD 15           // tokens per word at most (host-checked by the caller that packs the lexicon)
#define LX_WIN 16            // hypothesis entries 1..16 of a 17-wide row
#define LX_NONE 0xFFFFFFFFu

__device__ __forceinline__ unsigned lx_wave_min(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}

// grid N, LX_THREADS threads
__global__ __launch_bounds__(LX_THREADS) void lexicon_shortlist_kernel(
    const int64_t* __restrict__ ys_l, const int64_t* __restrict__ ys_r, long ld_n, long ld_h, const uint4* __restrict__ lex, int Wn,
    int H, int K, int64_t sos, int64_t eos, int64_t ignore, int32_t* __restrict__ cand, int32_t* __restrict__ cand_dist,
    int32_t* __restrict__ cand_hyp, int64_t* __restrict__ cand_ys_l, int64_t* __restrict__ cand_ys_r, int32_t* __restrict__ n_pos) {
    __shared__ unsigned char s_hyp[2 * LX_MAX_H][LX_WIN];      // [h * 2 + direction][position]: the kept tokens (r2l reversed)
    __shared__ int s_hlen[2 * LX_MAX_H];
    __shared__ unsigned s_part[2][LX_WAVES];
    __shared__ unsigned s_sel[LX_MAX_K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x;

    if (tid < 2 * H) {      // entries 1..16, cut before the first eos, without sos / ignore; an id that no byte holds reads 255
        const int h = tid >> 1, d = tid & 1;
        const int64_t* row = (d ? ys_r : ys_l) + n * ld_n + h * ld_h;
        int len = 0;
        bool open = true;
        for (int i = 1; i <= LX_WIN; ++i) {
            const int64_t t = row[i];
            open = open && t != eos;
            if (open && t != sos && t != ignore) ++len;
        }
        s_hlen[tid] = len;
        int k = 0;
        open = true;
        for (int i = 1; i <= LX_WIN; ++i) {
            const int64_t t = row[i];
            open = open && t != eos;
            if (open && t != sos && t != ignore) {
                s_hyp[tid][d ? len - 1 - k : k] = (unsigned char)(t >= 0 && t < 255 ? t : 255);
                ++k;
            }
        }
    }
    __syncthreads();

    unsigned top[LX_MAX_K];      // the lane's K smallest keys, ascending
#pragma unroll
    for (int k = 0; k < LX_MAX_K; ++k) top[k] = LX_NONE;

    for (int w = tid; w < Wn; w += LX_THREADS) {
        const uint4 q = lex[w];
        const unsigned qw[4] = {q.x, q.y, q.z, q.w};
        const int c = min((int)(q.w >> 24), LX_WORD);
        unsigned g[LX_WORD];
#pragma unroll
        for (int j = 0; j < LX_WORD; ++j) g[j] = (qw[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        unsigned best = LX_NONE;      // D << 4 | h
        for (int h = 0; h < H; ++h) {
            int dist = 0;
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                int D[LX_WORD + 1];
                D[0] = 0;
#pragma unroll
                for (int j = 1; j <= LX_WORD; ++j) D[j] = D[j - 1] + (j - 1 < c ? 1 : 0);
                const int len = s_hlen[2 * h + d];
                for (int i = 0; i < len; ++i) {      // (uniform)
                    const unsigned p = s_hyp[2 * h + d][i];
                    int diag = D[0];
                    int left = D[0] + 1;
                    D[0] = left;
#pragma unroll
                    for (int j = 1; j <= LX_WORD; ++j) {
                        const int up = D[j];
                        const int cell = min(min(up + 1, left + 1), diag + (p != g[j - 1] ? 1 : 0));
                        left = j - 1 < c ? cell : left;
                        diag = up;
                        D[j] = left;
                    }
                }
                dist += D[LX_WORD];
            }
            best = min(best, (unsigned)dist << 4 | (unsigned)h);      // equal D: the lower h stays
        }
        unsigned key = best << 16 | (unsigned)w;
#pragma unroll
        for (int k = 0; k < LX_MAX_K; ++k) {      // sorted insert; what falls off the end is not among the K smallest
            const unsigned lo = min(top[k], key);
            key = max(top[k], key);
            top[k] = lo;
        }
    }

    for (int r = 0; r < K; ++r) {
        const unsigned wm = lx_wave_min(top[0]);
        if (lane == 0) s_part[r & 1][wave] = wm;
        __syncthreads();      // one barrier per round: round r + 2 rewrites this buffer behind the barrier of round r + 1
        unsigned m = lane < LX_WAVES ? s_part[r & 1][lane] : LX_NONE;
        m = lx_wave_min(m);
        if (m != LX_NONE && top[0] == m) {      // keys are distinct: exactly one lane
#pragma unroll
            for (int k = 0; k + 1 < LX_MAX_K; ++k) top[k] = top[k + 1];
            top[LX_MAX_K - 1] = LX_NONE;
        }
        if (tid == 0) s_sel[r] = m;
    }
    __syncthreads();

    // the candidates' tables: <sos>, the word (reversed for r2l), <eos> fill
    const unsigned char* lexb = reinterpret_cast<const unsigned char*>(lex);
    const int L = LX_WIN + 1;
    for (int i = tid; i < K * L; i += LX_THREADS) {
        const int r = i / L, j = i - r * L;
        const unsigned key = s_sel[r];
        const long w = key == LX_NONE ? 0 : (long)(key & 0xFFFFu);      // (K <= Wn: every round finds a word)
        const int c = min((int)lexb[w * 16 + 15], LX_WORD);
        const long o = ((long)n * K + r) * L + j;
        int64_t tl = eos, tr = eos;
        if (j == 0) tl = tr = sos;
        else if (j <= c) {
            tl = lexb[w * 16 + j - 1];
            tr = lexb[w * 16 + c - j];
        }
        cand_ys_l[o] = tl;
        cand_ys_r[o] = tr;
        if (j == 0) {
            const long s = (long)n * K + r;
            cand[s] = (int32_t)w;
            cand_dist[s] = key == LX_NONE ? -1 : (int32_t)(key >> 20);
            cand_hyp[s] = key == LX_NONE ? -1 : (int32_t)((key >> 16) & 15u);
            n_pos[s] = c + 1;
        }
    }
}

extern "C" int sbl_lexicon_shortlist(const int64_t* ys_l2r, const int64_t* ys_r2l, long ld_n, long ld_h, int Ly, const uint8_t* lex,
                                     int Wn, int N, int H, int K, int64_t sos, int64_t eos, int64_t ignore, int32_t* cand,
                                     int32_t* cand_dist, int32_t* cand_hyp, int64_t* cand_ys_l2r, int64_t* cand_ys_r2l,
                                     int32_t* n_pos, sbl_stream_t stream) {
    SBL_REQUIRE(N >= 0, "sbl_lexicon_shortlist: N=%d", N);
    SBL_REQUIRE(Ly == LX_WIN + 1, "sbl_lexicon_shortlist: hypothesis rows of %d entries (built for %d)", Ly, LX_WIN + 1);
    SBL_REQUIRE(H >= 1 && H <= LX_MAX_H, "sbl_lexicon_shortlist: H=%d hypotheses per clip outside 1..%d", H, LX_MAX_H);
    SBL_REQUIRE(Wn >= 1 && Wn <= 65536, "sbl_lexicon_shortlist: Wn=%d words outside 1..65536", Wn);
    SBL_REQUIRE(K >= 1 && K <= LX_MAX_K && K <= Wn, "sbl_lexicon_shortlist: shortlist K=%d outside 1..min(Wn=%d, %d)", K, Wn, LX_MAX_K);
    SBL_REQUIRE(ld_h >= 0 && ld_n >= 0 && (H == 1 || ld_h >= Ly), "sbl_lexicon_shortlist: hypothesis strides %ld / %ld", ld_n, ld_h);
    SBL_REQUIRE(sos != eos, "sbl_lexicon_shortlist: sos and eos are both %ld", (long)sos);
    if (N == 0) return 0;
    SBL_REQUIRE(ys_l2r && ys_r2l && lex, "sbl_lexicon_shortlist: null input");
    SBL_REQUIRE(sbl_aligned16(lex), "sbl_lexicon_shortlist: the packed lexicon is not 16-byte aligned");
    SBL_REQUIRE(cand && cand_dist && cand_hyp && cand_ys_l2r && cand_ys_r2l && n_pos, "sbl_lexicon_shortlist: null output");
    hipLaunchKernelGGL(lexicon_shortlist_kernel, dim3(N), dim3(LX_THREADS), 0, (hipStream_t)stream, ys_l2r, ys_r2l, ld_n, ld_h,
                       reinterpret_cast<const uint4*>(lex), Wn, H, K, sos, eos, ignore, cand, cand_dist, cand_hyp, cand_ys_l2r,
                       cand_ys_r2l, n_pos);
    SBL_LAUNCH_CHECK("sbl_lexicon_shortlist");
    return 0;
}

// ------------------------------------------------------------------ trie walk (the tables of sbl_beam_tail_lex)
// grid ceil(R / 256), one thread per row: the row's tokens by the hypothesis rule of the shortlist, walked from the root.
// Node values are clamped to 0 .. P-1 wherever they index a table, so a bad table reads nothing out of bounds.
__global__ __launch_bounds__(256) void lexicon_lookup_kernel(const int64_t* __restrict__ ys, long ldys, int Ly, int R,
                                                             const int64_t* __restrict__ trie_mask, const int32_t* __restrict__ trie_first,
                                                             const int32_t* __restrict__ trie_word, int P, int64_t sos, int64_t eos,
                                                             int64_t ignore, int32_t* __restrict__ word, int32_t* __restrict__ node) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const int64_t* row = ys + r * ldys;
    const unsigned long long not_eos = eos >= 0 && eos < 64 ? ~(1ull << eos) : ~0ull;
    int q = 0;
    bool open = true, found = true;
    for (int i = 1; i < Ly; ++i) {
        const int64_t t = row[i];
        open = open && t != eos;
        if (!open || t == sos || t == ignore || !found) continue;
        const unsigned long long m = (unsigned long long)trie_mask[q] & not_eos;
        if (t < 0 || t >= 64 || !((m >> t) & 1ull)) {
            found = false;
            continue;
        }
        q = trie_first[q] + (int)__popcll(m & ((1ull << t) - 1ull));
        q = q < 0 ? 0 : (q >= P ? P - 1 : q);
    }
    word[r] = found ? trie_word[q] : -1;
    node[r] = found ? q : -1;
}

extern "C" int sbl_lexicon_lookup(const int64_t* ys, long ldys, int Ly, int R, const int64_t* trie_mask, const int32_t* trie_first,
                                  const int32_t* trie_word, int P, int64_t sos, int64_t eos, int64_t ignore, int32_t* word,
                                  int32_t* node, sbl_stream_t stream) {
    SBL_REQUIRE(R >= 0, "sbl_lexicon_lookup: R=%d", R);
    SBL_REQUIRE(Ly >= 1 && ldys >= Ly, "sbl_lexicon_lookup: rows of %d entries with stride %ld", Ly, ldys);
    SBL_REQUIRE(P >= 1, "sbl_lexicon_lookup: P=%d trie nodes", P);
    SBL_REQUIRE(sos != eos, "sbl_lexicon_lookup: sos and eos are both %ld", (long)sos);
    if (R == 0) return 0;
    SBL_REQUIRE(ys && trie_mask && trie_first && trie_word, "sbl_lexicon_lookup: null input");
    SBL_REQUIRE(word && node, "sbl_lexicon_lookup: null output");
    hipLaunchKernelGGL(lexicon_lookup_kernel, dim3((R + 255) / 256), dim3(256), 0, (hipStream_t)stream, ys, ldys, Ly, R, trie_mask,
                       trie_first, trie_word, P, sos, eos, ignore, word, node);
    SBL_LAUNCH_CHECK("sbl_lexicon_lookup");
    return 0;
}

#define PS_MAX_G 16
#define PS_STEPS 16

// grid S / G, 256 threads.  Row (step i, slot s) of y_l / y_r is i * S + s (segment-major, as sbl_gather_last_fwd writes it).
__global__ __launch_bounds__(256) void pair_score_tail_kernel(
    const float* __restrict__ y_l, const float* __restrict__ y_r, long ldy, const float* __restrict__ w_l,
    const float* __restrict__ w_r, const int64_t* __restrict__ ys_l, const int64_t* __restrict__ ys_r, long ldys,
    const int32_t* __restrict__ n_pos, float* __restrict__ logp, float* __restrict__ score_dir, float* __restrict__ score,
    int32_t* __restrict__ best, int S, int G, int V) {
    __shared__ float s_lg[2][PS_MAX_G][64];                // [direction][slot][class]: logits of the current step
    __shared__ float s_lp[PS_STEPS][PS_MAX_G][2];          // [step][slot][direction]: log-prob of the slot's own token
    __shared__ int s_np[PS_MAX_G];
    __shared__ float s_sc[PS_MAX_G];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long slot0 = (long)blockIdx.x * G;

    if (threadIdx.x < G) s_np[threadIdx.x] = n_pos ? min(max(n_pos[slot0 + threadIdx.x], 0), PS_STEPS) : PS_STEPS;
    for (int i = threadIdx.x; i < PS_STEPS * PS_MAX_G * 2; i += 256) (&s_lp[0][0][0])[i] = 0.f;
    __syncthreads();
    int np_max = 0;
    for (int r = 0; r < G; ++r) np_max = max(np_max, s_np[r]);

    for (int i = 0; i < np_max; ++i) {      // (uniform)
        // logits: each wave takes every fourth (direction, class) and keeps its weight row in registers
        for (int idx = wave; idx < 2 * V; idx += 4) {
            const int d = idx >= V, v = idx - d * V;
            const float4* wr = reinterpret_cast<const float4*>((d ? w_r : w_l) + (long)v * DH_D);
            const float4 a = wr[lane], c = wr[64 + lane];
            const float* y = d ? y_r : y_l;
            for (int r = 0; r < G; ++r) {
                if (i >= s_np[r]) continue;      // (uniform)
                const float acc = dh_row_dot(reinterpret_cast<const float4*>(y + ((long)i * S + slot0 + r) * ldy), a, c, lane);
                if (lane == 0) s_lg[d][r][v] = acc;
            }
        }
        __syncthreads();
        for (int row = wave; row < 2 * G; row += 4) {
            const int d = row >= G, r = row - d * G;
            if (i >= s_np[r]) continue;          // (uniform)
            const float lp = dh_log_softmax(lane < V ? s_lg[d][r][lane] : -INFINITY, lane < V);
            const int64_t tok = (d ? ys_r : ys_l)[(slot0 + r) * ldys + i + 1];
            const bool inside = tok >= 0 && tok < V;      // a token that is no class has no probability
            const float mine = __shfl(lp, inside ? (int)tok : 0, 64);
            if (lane == 0) s_lp[i][r][d] = inside ? mine : -INFINITY;
        }
        __syncthreads();
    }

    if (threadIdx.x < G) {      // the sums in ascending step order; score as sbl_pair_beam_tail forms its totals
        const int r = threadIdx.x, np = s_np[r];
        float sl = 0.f, sr = 0.f, sc = 0.f;
        for (int i = 0; i < np; ++i) {
            const float a = s_lp[i][r][0], b = s_lp[i][r][1];
            sl += a;
            sr += b;
            sc += (a + b);
        }
        score_dir[(slot0 + r) * 2] = sl;
        score_dir[(slot0 + r) * 2 + 1] = sr;
        score[slot0 + r] = sc;
        s_sc[r] = sc;
    }
    for (int i = threadIdx.x; i < G * PS_STEPS * 2; i += 256) {      // steps at or behind n_pos read 0
        const int r = i / (PS_STEPS * 2), rem = i - r * PS_STEPS * 2;
        logp[slot0 * PS_STEPS * 2 + i] = s_lp[rem >> 1][r][rem & 1];
    }
    __syncthreads();
    if (threadIdx.x == 0) {      // the largest score; an exact tie stays with the lower rank
        int b = 0;
        for (int r = 1; r < G; ++r)
            if (s_sc[r] > s_sc[b]) b = r;
        best[blockIdx.x] = b;
    }
}

extern "C" int sbl_pair_score_tail(const float* y_l, const float* y_r, long ldy, const float* w_l, const float* w_r,
                                   const int64_t* ys_l2r, const int64_t* ys_r2l, long ldys, const int32_t* n_pos, float* logp,
                                   float* score_dir, float* score, int32_t* best, int S, int G, int V, int D, sbl_stream_t stream) {
    SBL_REQUIRE(D == DH_D, "sbl_pair_score_tail: D=%d (built for %d)", D, DH_D);
    SBL_REQUIRE(V >= 1 && V <= DH_MAX_V, "sbl_pair_score_tail: V=%d (V <= %d)", V, DH_MAX_V);
    SBL_REQUIRE(G >= 1 && G <= PS_MAX_G, "sbl_pair_score_tail: group G=%d outside 1..%d", G, PS_MAX_G);
    SBL_REQUIRE(S >= 0 && S % G == 0, "sbl_pair_score_tail: S=%d slots are no multiple of the group size %d", S, G);
    SBL_REQUIRE((long)S * PS_STEPS <= (1L << 30), "sbl_pair_score_tail: S=%d", S);
    SBL_REQUIRE(ldys >= PS_STEPS + 1, "sbl_pair_score_tail: token rows of %ld entries (%d needed)", ldys, PS_STEPS + 1);
    SBL_REQUIRE(ldy >= D && ldy % 4 == 0, "sbl_pair_score_tail: row stride %ld", ldy);
    if (S == 0) return 0;
    SBL_REQUIRE(y_l && y_r && w_l && w_r && ys_l2r && ys_r2l, "sbl_pair_score_tail: null input");
    SBL_REQUIRE(logp && score_dir && score && best, "sbl_pair_score_tail: null output");
    SBL_REQUIRE(sbl_aligned16(y_l) && sbl_aligned16(y_r) && sbl_aligned16(w_l) && sbl_aligned16(w_r), "sbl_pair_score_tail: unaligned");
    hipLaunchKernelGGL(pair_score_tail_kernel, dim3(S / G), dim3(256), 0, (hipStream_t)stream, y_l, y_r, ldy, w_l, w_r, ys_l2r, ys_r2l,
                       ldys, n_pos, logp, score_dir, score, best, S, G, V);
    SBL_LAUNCH_CHECK("sbl_pair_score_tail");
    return 0;
}
