// Validation scoring: edit distance / word error of greedy decodes against the targets, counters kept on the device
// (SBL/train.py:251-276 with per_compute / wer_compute of :28-42; the definition and its three stated deviations are in
// include/sbl_hip.h).
//
// One LANE per (direction, sample) pair.  The problem is at most 16 x 15 cells per pair and 2N pairs (64 at the
// validation batch of 32): there is nothing to tile and no bandwidth to speak of, the launch is latency-bound.  With one
// lane per pair the whole dynamic program sits in registers with compile-time indices (a 16-entry row, the 16 + 15 token
// ids), a wavefront needs no cross-lane traffic until the final counter reduction, and that reduction covers 64 pairs at
// once: one wavefront per pair would spend its 31 anti-diagonals on shuffles, leave 48 of 64 lanes idle on every one of
// them and still need a second stage to sum the pairs.
//
// Nothing is compacted: a stripped target entry is a TRANSPARENT column (it copies its left neighbour, so the row value at
// any column is the value at the last kept column before it) and a stripped / out-of-window prediction entry leaves the
// row as it is.  That keeps every array index static (a runtime-indexed register array would go to scratch memory).
#include "sbl_common.h"

#define SCORE_MAX_TO 15      // target width bound (host-checked): gold length c <= 15
#define SCORE_WIN 16         // prediction window ys[:c+1] never reaches beyond column 15
#define SCORE_NAME_WORDS 14  // 16 spellings of <= 7 bytes = 112 bytes

// appends the L = len(w) low bytes of w to a big integer (most significant word last), as a shift register
__device__ __forceinline__ void spell_append(uint64_t (&acc)[SCORE_NAME_WORDS], uint64_t w, int L) {
    const int s = 8 * L;      // 0 .. 56; (x >> 1) >> (63 - s) is x >> (64 - s) without the undefined shift by 64 at s = 0
#pragma unroll
    for (int k = SCORE_NAME_WORDS - 1; k > 0; --k) acc[k] = (acc[k] << s) | ((acc[k - 1] >> 1) >> (63 - s));
    acc[0] = (acc[0] << s) | w;
}

__global__ __launch_bounds__(64) void seq_score_kernel(const int64_t* __restrict__ ys0, const int64_t* __restrict__ ys1, int Ly,
                                                       const int64_t* __restrict__ gold0, const int64_t* __restrict__ gold1,
                                                       int To, int N, int64_t sos, int64_t eos, int64_t ignore,
                                                       const uint64_t* __restrict__ names, int n_names,
                                                       const int32_t* __restrict__ valid_rows, int32_t* __restrict__ per_sample,
                                                       unsigned long long* __restrict__ acc) {
    const int lane = threadIdx.x;
    const int dir = blockIdx.y;
    const int n = blockIdx.x * 64 + lane;
    const int nvalid = valid_rows ? min(max(valid_rows[0], 0), N) : N;
    const bool in_range = n < N;
    const bool live = n < nvalid;
    const int row = in_range ? n : 0;      // lanes past the end read row 0 and contribute nothing
    const int64_t* ys = (dir ? ys1 : ys0) + (long)row * Ly;
    const int64_t* gold = (dir ? gold1 : gold0) + (long)row * To;

    int64_t g[SCORE_MAX_TO], p[SCORE_WIN];
    bool gk[SCORE_MAX_TO], pk[SCORE_WIN];      // kept (not sos / eos / ignore, inside the tensor)
    int c = 0;
#pragma unroll
    for (int j = 0; j < SCORE_MAX_TO; ++j) {
        g[j] = j < To ? gold[j] : ignore;
        gk[j] = j < To && g[j] != sos && g[j] != eos && g[j] != ignore;
        c += gk[j] ? 1 : 0;
    }
#pragma unroll
    for (int i = 0; i < SCORE_WIN; ++i) {
        p[i] = i < Ly ? ys[i] : ignore;
        pk[i] = i < Ly && i <= c && p[i] != sos && p[i] != eos && p[i] != ignore;      // the window ys[:c+1]
    }

    // Levenshtein distance, unit costs: D[j] = distance(kept predictions so far, kept targets among the first j columns)
    int D[SCORE_MAX_TO + 1];
    D[0] = 0;
#pragma unroll
    for (int j = 1; j <= SCORE_MAX_TO; ++j) D[j] = D[j - 1] + (gk[j - 1] ? 1 : 0);
#pragma unroll
    for (int i = 0; i < SCORE_WIN; ++i) {
        int diag = D[0];                 // old D[j-1]
        int left = D[0] + 1;             // new D[j-1]
        D[0] = pk[i] ? left : D[0];
#pragma unroll
        for (int j = 1; j <= SCORE_MAX_TO; ++j) {
            const int up = D[j];
            const int cell = min(min(up + 1, left + 1), diag + (p[i] != g[j - 1] ? 1 : 0));
            left = gk[j - 1] ? cell : left;
            diag = up;
            D[j] = pk[i] ? left : up;
        }
    }
    const int dist = D[SCORE_MAX_TO];

    // word error: the two kept sequences spell different strings.  Without a name table the spelling of an id is the id
    // itself, and two sequences differ exactly when their distance is not zero.
    int werr = dist != 0;
    if (names) {      // (uniform)
        uint64_t sp[SCORE_NAME_WORDS], sg[SCORE_NAME_WORDS];
#pragma unroll
        for (int k = 0; k < SCORE_NAME_WORDS; ++k) sp[k] = sg[k] = 0;
        int lp = 0, lg = 0;
#pragma unroll
        for (int i = 0; i < SCORE_WIN; ++i) {
            const bool ok = pk[i] && p[i] >= 0 && p[i] < n_names;      // an id outside the table spells nothing
            const uint64_t e = ok ? names[p[i]] : 0;
            const int L = (int)(e >> 56) & 7;
            spell_append(sp, e & 0x00FFFFFFFFFFFFFFull, L);
            lp += L;
        }
#pragma unroll
        for (int j = 0; j < SCORE_MAX_TO; ++j) {
            const bool ok = gk[j] && g[j] >= 0 && g[j] < n_names;
            const uint64_t e = ok ? names[g[j]] : 0;
            const int L = (int)(e >> 56) & 7;
            spell_append(sg, e & 0x00FFFFFFFFFFFFFFull, L);
            lg += L;
        }
        uint64_t diff = (uint64_t)(lp ^ lg);
#pragma unroll
        for (int k = 0; k < SCORE_NAME_WORDS; ++k) diff |= sp[k] ^ sg[k];
        werr = diff != 0;
    }

    if (per_sample && in_range) {      // (dir, {dist, c, word_err}, n); rows at or beyond valid_rows read -1
        int32_t* o = per_sample + (long)dir * 3 * N + n;
        o[0] = live ? dist : -1;
        o[(long)N] = live ? c : -1;
        o[2L * N] = live ? werr : -1;
    }

    // counters: two packed wave sums (every field's total over 64 lanes stays inside its field: <= 64 in 8 bits,
    // <= 64 * 16 in 16 bits), then the per-length histogram by a transposing butterfly, then <= 37 atomics per wavefront
    const bool scored = live && c > 0;
    unsigned a = (scored ? 1u : 0u) | (live && c == 0 ? 1u << 8 : 0u) | (scored && werr ? 1u << 16 : 0u);
    unsigned b = scored ? (unsigned)dist | (unsigned)c << 16 : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    unsigned h[16];      // h[len] = dist << 16 | 1 for this lane's sample
#pragma unroll
    for (int k = 0; k < 16; ++k) h[k] = scored && c == k ? ((unsigned)dist << 16 | 1u) : 0u;
    // after the step with offset o a lane keeps the half of its bins whose index has bit o equal to its own lane bit o:
    // lane l ends with bin (l & 15) summed over its 16-lane group; two more steps sum the four groups
#define SCORE_TSTEP(NB, O)                                          \
    _Pragma("unroll") for (int k = 0; k < (NB) / 2; ++k) {          \
        const bool hi = (lane & (O)) != 0;                          \
        const unsigned keep = hi ? h[k + (NB) / 2] : h[k];          \
        const unsigned send = hi ? h[k] : h[k + (NB) / 2];          \
        h[k] = keep + __shfl_xor(send, (O), 64);                    \
    }
    SCORE_TSTEP(16, 8) SCORE_TSTEP(8, 4) SCORE_TSTEP(4, 2) SCORE_TSTEP(2, 1)
#undef SCORE_TSTEP
    unsigned hb = h[0];
    hb += __shfl_xor(hb, 16, 64);
    hb += __shfl_xor(hb, 32, 64);

    unsigned long long* out = acc + (long)dir * SBL_SCORE_COUNTERS;
    if (lane < 16) {
        const unsigned d = hb >> 16, cnt = hb & 0xFFFFu;
        if (d) atomicAdd(out + SBL_SCORE_DIST_BY_LEN + lane, (unsigned long long)d);
        if (cnt) atomicAdd(out + SBL_SCORE_COUNT_BY_LEN + lane, (unsigned long long)cnt);
    } else if (lane < 16 + 5) {
        const int k = lane - 16;
        const unsigned v = k == 0 ? (a & 0xFFu) : k == 1 ? ((a >> 8) & 0xFFu) : k == 2 ? (a >> 16) : k == 3 ? (b & 0xFFFFu) : (b >> 16);
        if (v) atomicAdd(out + k, (unsigned long long)v);
    }
}

extern "C" int sbl_seq_score(const int64_t* ys_l2r, const int64_t* ys_r2l, int Ly, const int64_t* gold_l2r, const int64_t* gold_r2l,
                             int To, int N, int64_t sos, int64_t eos, int64_t ignore, const uint64_t* names, int n_names,
                             const int32_t* valid_rows, int32_t* per_sample, uint64_t* acc, sbl_stream_t stream) {
    SBL_REQUIRE(N >= 0, "sbl_seq_score: N=%d", N);
    SBL_REQUIRE(To >= 1 && To <= SCORE_MAX_TO, "sbl_seq_score: target width To=%d outside 1..%d", To, SCORE_MAX_TO);
    SBL_REQUIRE(Ly >= 1, "sbl_seq_score: prediction width Ly=%d", Ly);
    SBL_REQUIRE((names != nullptr) == (n_names > 0), "sbl_seq_score: name table and n_names=%d disagree", n_names);
    SBL_REQUIRE(acc, "sbl_seq_score: null accumulator");
    if (N == 0) return 0;
    SBL_REQUIRE(ys_l2r && ys_r2l && gold_l2r && gold_r2l, "sbl_seq_score: null token tensor");
    hipLaunchKernelGGL(seq_score_kernel, dim3(sbl_cdiv(N, 64), 2), dim3(64), 0, (hipStream_t)stream, ys_l2r, ys_r2l, Ly, gold_l2r,
                       gold_r2l, To, N, sos, eos, ignore, names, n_names, valid_rows, per_sample, (unsigned long long*)acc);
    SBL_LAUNCH_CHECK("sbl_seq_score");
    return 0;
}

// One direction (the single-direction seq2seq model, LRW/train.py:245-260): the same kernel with a grid of one direction;
// acc is one row of SBL_SCORE_COUNTERS counters, per_sample int32 (3, N).
extern "C" int sbl_seq_score1(const int64_t* ys, int Ly, const int64_t* gold, int To, int N, int64_t sos, int64_t eos,
                              int64_t ignore, const uint64_t* names, int n_names, const int32_t* valid_rows, int32_t* per_sample,
                              uint64_t* acc, sbl_stream_t stream) {
    SBL_REQUIRE(N >= 0, "sbl_seq_score1: N=%d", N);
    SBL_REQUIRE(To >= 1 && To <= SCORE_MAX_TO, "sbl_seq_score1: target width To=%d outside 1..%d", To, SCORE_MAX_TO);
    SBL_REQUIRE(Ly >= 1, "sbl_seq_score1: prediction width Ly=%d", Ly);
    SBL_REQUIRE((names != nullptr) == (n_names > 0), "sbl_seq_score1: name table and n_names=%d disagree", n_names);
    SBL_REQUIRE(acc, "sbl_seq_score1: null accumulator");
    if (N == 0) return 0;
    SBL_REQUIRE(ys && gold, "sbl_seq_score1: null token tensor");
    hipLaunchKernelGGL(seq_score_kernel, dim3(sbl_cdiv(N, 64), 1), dim3(64), 0, (hipStream_t)stream, ys, ys, Ly, gold, gold, To, N,
                       sos, eos, ignore, names, n_names, valid_rows, per_sample, (unsigned long long*)acc);
    SBL_LAUNCH_CHECK("sbl_seq_score1");
    return 0;
}
