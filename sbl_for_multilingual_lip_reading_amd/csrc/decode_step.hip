// Single-direction seq2seq decoder (LRW/transformer/decoder.py): scaled embedding + PE for the teacher-forced pass, and the
// kernels of a KV-cached decode step: the step attention, which the greedy decode and the beam search (beam_step.hip) share,
// and the greedy tail.
//
// The single-direction decoder is causal in every layer, so row i of every sub-layer depends on rows <= i only and the
// greedy loop of LRW/transformer/decoder.py:138-176 (which re-runs the whole prefix at every step) can keep each layer's
// self-attention K / V rows and process ONE new row per clip and step.  At the decode batch (32 clips) a step is 32 rows:
// every kernel here is launch- and latency-bound, not bandwidth- or FLOP-bound (a layer's cache is at most 64 x 512 floats
// per clip), so the design goal is few, short launches with no LDS round trips and no cross-wave synchronisation:
//   * step_attn_kernel: one wavefront per (row, head).  Scores: lane j owns key j (<= 64 keys, so one pass), the query's
//     64 floats are read as wave-uniform float4s; softmax max / sum are two wave-shuffle reductions; the value sum puts lane d
//     on output column d, reads V rows coalesced and takes p_j from lane j with one shuffle per key.  No LDS at all.
//     With `append` the step's new K / V row is stored at row n_prev of the row's OWN cache and used FROM REGISTERS for its
//     own score and value term, so the kernel never reads back a row it has just written.
//     In a beam search a row is one of a clip's W slots and a hypothesis changes its parent at every step; instead of
//     copying cache rows between slots each slot keeps an ANCESTRY row - anc[b][j] is the slot whose cache row j holds key j
//     of the hypothesis now living in slot b - and the SLOTS instantiation looks the cache slot of key j up there (score and
//     value pass).  Rows j < n_prev of every slot were written at step j and are never written again, so no launch reads a
//     row that the same launch writes.
//     The LEN instantiations (the `_len` entries, cross-attention over a padded batch of ragged clips) take a key count per
//     K / V entry in place of the launch's one n_prev; the instantiations without it compile as they did before LEN existed.
//   * decode_tail_kernel: one workgroup per clip: the bias-free projection to V <= 64 classes (each wave takes every
//     fourth class, lanes along the 512 features, coalesced), arg-max with the lowest index on ties, the token appended
//     to ys[:, step + 1], and the next step's input row emb[token] * scale + pe[step + 1] - tokens never visit the host.
#include "decode_head.h"

#define DEC_MAX_KEYS 64     // one key per lane

// ------------------------------------------------------------------ emb[tok] * scale + pe: LRW/transformer/decoder.py:111-112
__global__ __launch_bounds__(256) void embed_scale_pe_fwd_kernel(const int64_t* __restrict__ tok, long ldt,
                                                                 const float* __restrict__ emb, const float* __restrict__ pe,
                                                                 float* __restrict__ out, long rows, int L, int D4, int V,
                                                                 float scale, int pos0) {
    const long n4 = rows * D4;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const int c = (int)(i % D4);
        const long r = i / D4;
        const long b = r / L;
        const int l = (int)(r - b * L) + pos0;
        long t = tok[b * ldt + l];
        t = t < 0 ? 0 : (t >= V ? V - 1 : t);
        const float4 e = reinterpret_cast<const float4*>(emb)[t * D4 + c];
        const float4 p = reinterpret_cast<const float4*>(pe)[(long)l * D4 + c];
        reinterpret_cast<float4*>(out)[i] =
            make_float4(e.x * scale + p.x, e.y * scale + p.y, e.z * scale + p.z, e.w * scale + p.w);
    }
}
__global__ __launch_bounds__(256) void embed_scale_bwd_kernel(const int64_t* __restrict__ tok, long ldt,
                                                              const float* __restrict__ dy, float* __restrict__ demb, long rows,
                                                              int L, int D, int V, float scale) {
    const long n = rows * D;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int c = (int)(i % D);
        const long r = i / D;
        const long b = r / L;
        const int l = (int)(r - b * L);
        long t = tok[b * ldt + l];
        t = t < 0 ? 0 : (t >= V ? V - 1 : t);
        atomicAdd(demb + t * D + c, dy[i] * scale);
    }
}
static inline int dec_grid(long n) {
    long g = (n + 255) / 256;
    return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}
extern "C" int sbl_embed_scale_pe_fwd(const int64_t* tok, long ldt, const float* emb, const float* pe, float* out, int B, int L,
                                      int D, int V, float scale, int pos0, sbl_stream_t stream) {
    SBL_REQUIRE(tok && emb && pe && out && B > 0 && L > 0 && D > 0 && D % 4 == 0 && V > 0 && pos0 >= 0,
                "sbl_embed_scale_pe_fwd: bad args");
    SBL_REQUIRE(ldt >= pos0 + L, "sbl_embed_scale_pe_fwd: token row of %ld shorter than %d + %d", ldt, pos0, L);
    SBL_REQUIRE(sbl_aligned16(emb) && sbl_aligned16(pe) && sbl_aligned16(out), "sbl_embed_scale_pe_fwd: unaligned");
    const long rows = (long)B * L;
    hipLaunchKernelGGL(embed_scale_pe_fwd_kernel, dim3(dec_grid(rows * D / 4)), dim3(256), 0, (hipStream_t)stream, tok, ldt, emb,
                       pe, out, rows, L, D / 4, V, scale, pos0);
    SBL_LAUNCH_CHECK("sbl_embed_scale_pe_fwd");
    return 0;
}
extern "C" int sbl_embed_scale_bwd(const int64_t* tok, long ldt, const float* dy, float* demb, int B, int L, int D, int V,
                                   float scale, sbl_stream_t stream) {
    SBL_REQUIRE(tok && dy && demb && B > 0 && L > 0 && D > 0 && V > 0, "sbl_embed_scale_bwd: bad args");
    SBL_REQUIRE(ldt >= L, "sbl_embed_scale_bwd: token row of %ld shorter than %d", ldt, L);
    const long rows = (long)B * L;
    hipLaunchKernelGGL(embed_scale_bwd_kernel, dim3(dec_grid(rows * D)), dim3(256), 0, (hipStream_t)stream, tok, ldt, dy, demb,
                       rows, L, D, V, scale);
    SBL_LAUNCH_CHECK("sbl_embed_scale_bwd");
    return 0;
}

// ------------------------------------------------------------------ single-query attention over a K / V cache
// grid (H, rows), one wavefront each.  Keys: cache rows 0 .. n_prev-1, plus (append) the new row, which is also stored at row
// n_prev of cache b.  n_prev + append <= Lcap <= 64 is checked on the host, so every cache index below is inside the Lcap
// rows of a cache.  Without SLOTS row b owns cache b.  With SLOTS, append: key j is row j of cache anc[b][j] (clamped to
// 0 .. S-1, so whatever the table holds the reads stay inside the S caches); no append (cross-attention): slot b reads the
// hoisted cache of clip b / W, of which there are S / W.
template <bool SLOTS, bool LEN = false>
__global__ __launch_bounds__(64) void step_attn_kernel(const float* __restrict__ q, long ldq, const float* __restrict__ k_new,
                                                       const float* __restrict__ v_new, long ldn, float* k_cache, float* v_cache,
                                                       long ldc, int Lcap, const int32_t* __restrict__ anc, long lda,
                                                       float* __restrict__ o, long ldo, int S, int W, int n_keys, int append_arg,
                                                       float scale) {
    const int lane = threadIdx.x;
    const int h = blockIdx.x, b = blockIdx.y;
    // LEN (the `_len` entries; cross-attention only, so the ancestry argument is free and carries the key counts): the
    // entry's count, clamped to 0 .. n_keys, takes the place of the number of cached keys.  One wavefront per (row, head),
    // so the count is wavefront-uniform, and every load below is predicated on it as it is on n_keys without LEN.
    int n_prev = n_keys;
    const int append = LEN ? 0 : append_arg;
    if constexpr (LEN) {
        const int32_t* kv_len = anc;      // one count per K / V entry: B of them, or S / W with SLOTS (the host passes them here)
        int l = kv_len[SLOTS ? b / W : b];
        l = l < 0 ? 0 : l;
        n_prev = __builtin_amdgcn_readfirstlane(l < n_keys ? l : n_keys);
    }
    const long col = (long)h * 64;
    const float* qrow = q + (long)b * ldq + col;
    // Row 0 of cache b at this head's columns: without SLOTS every cache address is formed from these, with SLOTS from the
    // slot index.  The two forms name the same elements; both are kept because which products of the dot products the
    // compiler contracts into FMAs follows the address arithmetic around them, and with these forms each instantiation
    // compiles to the instructions, and so to the rounding, that it had as a kernel of its own.
    float* kc = k_cache + (long)b * Lcap * ldc + col;
    float* vc = v_cache + (long)b * Lcap * ldc + col;
    int src = b;      // the cache of key `lane`
    if (SLOTS) {
        src = append ? b : b / W;
        if (append && lane < n_prev) {
            src = anc[(long)b * lda + lane];
            src = src < 0 ? 0 : (src >= S ? S - 1 : src);
        }
    }

    // scores of the cached keys: lane j <- q . K[j]
    float s = -INFINITY;
    if (lane < n_prev) {
        const float* kp = SLOTS ? k_cache + ((long)src * Lcap + lane) * ldc + col : kc + (long)lane * ldc;
        const float4* kr = reinterpret_cast<const float4*>(kp);
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
        const long own = SLOTS ? ((long)b * Lcap + n_prev) * ldc + col + lane : (long)n_prev * ldc + lane;
        (SLOTS ? k_cache : kc)[own] = kn;
        (SLOTS ? v_cache : vc)[own] = vn;
        const float sn = wave_sum(qrow[lane] * kn) * scale;
        if (lane == n_prev) s = sn;
    }
    const float m = wave_max(s);
    const float e = s == -INFINITY ? 0.f : __expf(s - m);
    const float p = e / wave_sum(e);

    // output column `lane`: sum_j p_j V[j][lane]
    float acc = 0.f;
    for (int j = 0; j < n_prev; ++j) {
        const float* vr = SLOTS ? v_cache + ((long)__shfl(src, j, 64) * Lcap + j) * ldc + col : vc + (long)j * ldc;
        acc += __shfl(p, j, 64) * vr[lane];
    }
    if (append) acc += __shfl(p, n_prev, 64) * vn;
    o[(long)b * ldo + col + lane] = acc;
}

// the checks and the launch behind the entry points; `name` is the entry's, S rows, anc != nullptr only with slots.  len: the
// `_len` entries, whose key counts kv_len travel in the kernel's ancestry argument (append = 0 leaves it unused).
static int step_attn_launch(const char* name, bool slots, const float* q, long ldq, const float* k_new, const float* v_new, long ldn,
                            float* k_cache, float* v_cache, long ldc, int Lcap, const int32_t* anc, long lda, float* o, long ldo,
                            int S, int W, int H, int n_prev, int append, float scale, sbl_stream_t stream, bool len = false,
                            const int32_t* kv_len = nullptr) {
    SBL_REQUIRE(!len || kv_len, "%s: kv_len is NULL", name);
    SBL_REQUIRE(!len || append == 0, "%s: append=%d (key counts go with the cross-attention, append = 0)", name, append);
    SBL_REQUIRE(Lcap >= 1 && Lcap <= DEC_MAX_KEYS, "%s: Lcap=%d outside 1..%d", name, Lcap, DEC_MAX_KEYS);
    SBL_REQUIRE(append == 0 || append == 1, "%s: append=%d", name, append);
    SBL_REQUIRE(n_prev >= 0 && n_prev + append >= 1 && n_prev + append <= Lcap, "%s: %d cached keys (+%d) do not fit Lcap=%d", name,
                n_prev, append, Lcap);
    SBL_REQUIRE(q && k_cache && v_cache && o, "%s: null pointer", name);
    SBL_REQUIRE(!append || (k_new && v_new && ldn >= (long)H * 64), "%s: new K/V row missing", name);
    SBL_REQUIRE(!slots || !append || n_prev == 0 || (anc && lda >= n_prev), "%s: ancestry rows of %ld entries for %d keys", name, lda,
                n_prev);
    SBL_REQUIRE(ldq >= (long)H * 64 && ldc >= (long)H * 64 && ldo >= (long)H * 64, "%s: row stride below H*64", name);
    SBL_REQUIRE(ldq % 4 == 0 && ldc % 4 == 0 && sbl_aligned16(q) && sbl_aligned16(k_cache), "%s: unaligned", name);
    if (len)
        hipLaunchKernelGGL((slots ? step_attn_kernel<true, true> : step_attn_kernel<false, true>), dim3(H, S), dim3(64), 0,
                           (hipStream_t)stream, q, ldq, k_new, v_new, ldn, k_cache, v_cache, ldc, Lcap, kv_len, 0L, o, ldo, S, W, n_prev,
                           0, scale);
    else
        hipLaunchKernelGGL(slots ? step_attn_kernel<true> : step_attn_kernel<false>, dim3(H, S), dim3(64), 0, (hipStream_t)stream, q,
                           ldq, k_new, v_new, ldn, k_cache, v_cache, ldc, Lcap, anc, lda, o, ldo, S, W, n_prev, append, scale);
    SBL_LAUNCH_CHECK(name);
    return 0;
}

extern "C" int sbl_decode_attn_step(const float* q, long ldq, const float* k_new, const float* v_new, long ldn, float* k_cache,
                                    float* v_cache, long ldc, int Lcap, float* o, long ldo, int B, int H, int n_prev,
                                    int append, float scale, sbl_stream_t stream) {
    SBL_REQUIRE(B > 0 && H > 0 && B <= 65535, "sbl_decode_attn_step: B=%d H=%d", B, H);
    return step_attn_launch("sbl_decode_attn_step", false, q, ldq, k_new, v_new, ldn, k_cache, v_cache, ldc, Lcap, nullptr, 0, o, ldo,
                            B, 1, H, n_prev, append, scale, stream);
}

extern "C" int sbl_beam_attn_step(const float* q, long ldq, const float* k_new, const float* v_new, long ldn, float* k_cache,
                                  float* v_cache, long ldc, int Lcap, const int32_t* anc, long lda, float* o, long ldo, int S,
                                  int W, int H, int n_prev, int append, float scale, sbl_stream_t stream) {
    SBL_REQUIRE(W >= 1 && W <= DH_MAX_W, "sbl_beam_attn_step: beam W=%d outside 1..%d", W, DH_MAX_W);
    SBL_REQUIRE(S > 0 && H > 0 && S <= 65535 && S % W == 0, "sbl_beam_attn_step: S=%d H=%d (S a multiple of W=%d)", S, H, W);
    return step_attn_launch("sbl_beam_attn_step", true, q, ldq, k_new, v_new, ldn, k_cache, v_cache, ldc, Lcap, anc, lda, o, ldo, S,
                            W, H, n_prev, append, scale, stream);
}

// the same two entries with a key count per K/V entry (cross-attention over a padded batch of ragged clips)
extern "C" int sbl_decode_attn_step_len(const float* q, long ldq, const float* k_new, const float* v_new, long ldn, float* k_cache,
                                        float* v_cache, long ldc, int Lcap, float* o, long ldo, int B, int H, int n_prev,
                                        int append, float scale, const int32_t* kv_len, sbl_stream_t stream) {
    SBL_REQUIRE(B > 0 && H > 0 && B <= 65535, "sbl_decode_attn_step_len: B=%d H=%d", B, H);
    return step_attn_launch("sbl_decode_attn_step_len", false, q, ldq, k_new, v_new, ldn, k_cache, v_cache, ldc, Lcap, nullptr, 0, o,
                            ldo, B, 1, H, n_prev, append, scale, stream, true, kv_len);
}

extern "C" int sbl_beam_attn_step_len(const float* q, long ldq, const float* k_new, const float* v_new, long ldn, float* k_cache,
                                      float* v_cache, long ldc, int Lcap, const int32_t* anc, long lda, float* o, long ldo, int S,
                                      int W, int H, int n_prev, int append, float scale, const int32_t* kv_len,
                                      sbl_stream_t stream) {
    SBL_REQUIRE(W >= 1 && W <= DH_MAX_W, "sbl_beam_attn_step_len: beam W=%d outside 1..%d", W, DH_MAX_W);
    SBL_REQUIRE(S > 0 && H > 0 && S <= 65535 && S % W == 0, "sbl_beam_attn_step_len: S=%d H=%d (S a multiple of W=%d)", S, H, W);
    return step_attn_launch("sbl_beam_attn_step_len", true, q, ldq, k_new, v_new, ldn, k_cache, v_cache, ldc, Lcap, anc, lda, o, ldo,
                            S, W, H, n_prev, append, scale, stream, true, kv_len);
}

// ------------------------------------------------------------------ decode tail: LRW/transformer/decoder.py:166-171 + :154-156
__global__ __launch_bounds__(256) void decode_tail_kernel(const float* __restrict__ y, long ldy, const float* __restrict__ w,
                                                          float* __restrict__ logits, long ldl, int64_t* __restrict__ ys, long ldys,
                                                          int step, const float* __restrict__ emb, const float* __restrict__ pe,
                                                          float emb_scale, float* __restrict__ x_next, int V) {
    __shared__ float s_logit[64];
    __shared__ int s_tok;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const float4* yr = reinterpret_cast<const float4*>(y + (long)b * ldy);
    for (int v = wave; v < V; v += 4) {
        const float4* wr = reinterpret_cast<const float4*>(w + (long)v * DH_D);
        const float acc = dh_row_dot(yr, wr[lane], wr[64 + lane], lane);
        if (lane == 0) s_logit[v] = acc;
    }
    __syncthreads();
    if (wave == 0) {
        float best = lane < V ? s_logit[lane] : -INFINITY;
        int bi = lane < V ? lane : DH_NONE;
        if (logits && lane < V) logits[(long)b * ldl + lane] = best;
        // torch.argmax (first maximal index) on every NaN-free row: a DH_NONE lane holds -inf, so against a class it loses
        // under plain (value, index) order as well - the DH_NONE tests only decide rows that hold NaN.  Lane 0 is a class
        // (V >= 1) and only ever takes another class, so the id stays in range on an all-NaN row too (it reads 0 there;
        // torch would return the NaN's index).
        dh_wave_best(best, bi);
        if (lane == 0) {
            ys[(long)b * ldys + step + 1] = bi;
            s_tok = bi;
        }
    }
    __syncthreads();
    if (x_next) dh_next_row(x_next + (long)b * DH_D, emb, s_tok, pe, step + 1, emb_scale);      // (uniform)
}

extern "C" int sbl_decode_tail(const float* y, long ldy, const float* w, float* logits, long ldl, int64_t* ys, long ldys, int step,
                               const float* emb, const float* pe, int pe_rows, float emb_scale, float* x_next, int B, int V, int D,
                               sbl_stream_t stream) {
    SBL_REQUIRE(D == DH_D, "sbl_decode_tail: D=%d (built for %d)", D, DH_D);
    SBL_REQUIRE(B > 0 && V >= 1 && V <= DH_MAX_V, "sbl_decode_tail: B=%d V=%d (V <= 64)", B, V);
    SBL_REQUIRE(y && w && ys && ldy >= D && ldy % 4 == 0, "sbl_decode_tail: bad args");
    SBL_REQUIRE(step >= 0 && step + 1 < ldys, "sbl_decode_tail: step %d beyond the token row of %ld", step, ldys);
    SBL_REQUIRE(!logits || ldl >= V, "sbl_decode_tail: logits row stride %ld below V", ldl);
    SBL_REQUIRE(!x_next || (emb && pe && step + 1 < pe_rows), "sbl_decode_tail: next-row embedding needs emb, pe and pe row %d",
                step + 1);
    SBL_REQUIRE(sbl_aligned16(y) && sbl_aligned16(w), "sbl_decode_tail: unaligned");
    hipLaunchKernelGGL(decode_tail_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, y, ldy, w, logits, ldl, ys, ldys, step, emb,
                       pe, emb_scale, x_next, V);
    SBL_LAUNCH_CHECK("sbl_decode_tail");
    return 0;
}
