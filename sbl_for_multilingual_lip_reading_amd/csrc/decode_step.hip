// Single-direction seq2seq decoder (LRW/transformer/decoder.py): scaled embedding + PE for the teacher-forced pass, and the
// three kernels of a KV-cached greedy decode step.
//
// The single-direction decoder is causal in every layer, so row i of every sub-layer depends on rows <= i only and the
// greedy loop of LRW/transformer/decoder.py:138-176 (which re-runs the whole prefix at every step) can keep each layer's
// self-attention K / V rows and process ONE new row per clip and step.  At the decode batch (32 clips) a step is 32 rows:
// every kernel here is launch- and latency-bound, not bandwidth- or FLOP-bound (a layer's cache is at most 64 x 512 floats
// per clip), so the design goal is few, short launches with no LDS round trips and no cross-wave synchronisation:
//   * decode_attn_kernel: one wavefront per (clip, head).  Scores: lane j owns key j (<= 64 keys, so one pass), the query's
//     64 floats are read as wave-uniform float4s; softmax max / sum are two wave-shuffle reductions; the value sum puts lane d
//     on output column d, reads V rows coalesced and takes p_j from lane j with one shuffle per key.  No LDS at all.
//     With `append` the step's new K / V row is stored at cache row n_prev and used FROM REGISTERS for its own score and
//     value term, so the kernel never reads back a row it has just written.
//   * decode_tail_kernel: one workgroup per clip: the bias-free projection to V <= 64 classes (each wave takes every
//     fourth class, lanes along the 512 features, coalesced), arg-max with the lowest index on ties, the token appended
//     to ys[:, step + 1], and the next step's input row emb[token] * scale + pe[step + 1] - tokens never visit the host.
#include "sbl_common.h"

#define DEC_D 512           // d_model of the decoder (host-checked)
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
// grid (H, B), one wavefront each.  Keys: cache rows 0 .. n_prev-1, plus (append) the new row, which is also stored at
// cache row n_prev.  n_prev + append <= Lcap <= 64 is checked on the host, so every cache index below is inside the
// (B, Lcap) rows of the cache.
__global__ __launch_bounds__(64) void decode_attn_kernel(const float* __restrict__ q, long ldq, const float* __restrict__ k_new,
                                                         const float* __restrict__ v_new, long ldn, float* k_cache,
                                                         float* v_cache, long ldc, int Lcap, float* __restrict__ o, long ldo,
                                                         int n_prev, int append, float scale) {
    const int lane = threadIdx.x;
    const int h = blockIdx.x, b = blockIdx.y;
    const long col = (long)h * 64;
    const float* qrow = q + (long)b * ldq + col;
    float* kc = k_cache + (long)b * Lcap * ldc + col;
    float* vc = v_cache + (long)b * Lcap * ldc + col;

    // scores of the cached keys: lane j <- q . K[j]
    float s = -INFINITY;
    if (lane < n_prev) {
        const float4* kr = reinterpret_cast<const float4*>(kc + (long)lane * ldc);
        const float4* q4 = reinterpret_cast<const float4*>(qrow);
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const float4 a = q4[t], c = kr[t];
            acc += a.x * c.x + a.y * c.y + a.z * c.z + a.w * c.w;
        }
        s = acc * scale;
    }
    float kn = 0.f, vn = 0.f;
    if (append) {      // (uniform) the new row: lane d holds column d; its score is one wave reduction
        kn = k_new[(long)b * ldn + col + lane];
        vn = v_new[(long)b * ldn + col + lane];
        kc[(long)n_prev * ldc + lane] = kn;
        vc[(long)n_prev * ldc + lane] = vn;
        const float sn = wave_sum(qrow[lane] * kn) * scale;
        if (lane == n_prev) s = sn;
    }
    const float m = wave_max(s);
    const float e = s == -INFINITY ? 0.f : __expf(s - m);
    const float p = e / wave_sum(e);

    // output column `lane`: sum_j p_j V[j][lane]
    float acc = 0.f;
    for (int j = 0; j < n_prev; ++j) acc += __shfl(p, j, 64) * vc[(long)j * ldc + lane];
    if (append) acc += __shfl(p, n_prev, 64) * vn;
    o[(long)b * ldo + col + lane] = acc;
}

extern "C" int sbl_decode_attn_step(const float* q, long ldq, const float* k_new, const float* v_new, long ldn, float* k_cache,
                                    float* v_cache, long ldc, int Lcap, float* o, long ldo, int B, int H, int n_prev,
                                    int append, float scale, sbl_stream_t stream) {
    SBL_REQUIRE(B > 0 && H > 0 && B <= 65535, "sbl_decode_attn_step: B=%d H=%d", B, H);
    SBL_REQUIRE(Lcap >= 1 && Lcap <= DEC_MAX_KEYS, "sbl_decode_attn_step: Lcap=%d outside 1..%d", Lcap, DEC_MAX_KEYS);
    SBL_REQUIRE(append == 0 || append == 1, "sbl_decode_attn_step: append=%d", append);
    SBL_REQUIRE(n_prev >= 0 && n_prev + append >= 1 && n_prev + append <= Lcap,
                "sbl_decode_attn_step: %d cached keys (+%d) do not fit Lcap=%d", n_prev, append, Lcap);
    SBL_REQUIRE(q && k_cache && v_cache && o, "sbl_decode_attn_step: null pointer");
    SBL_REQUIRE(!append || (k_new && v_new && ldn >= (long)H * 64), "sbl_decode_attn_step: new K/V row missing");
    SBL_REQUIRE(ldq >= (long)H * 64 && ldc >= (long)H * 64 && ldo >= (long)H * 64, "sbl_decode_attn_step: row stride below H*64");
    SBL_REQUIRE(ldq % 4 == 0 && ldc % 4 == 0 && sbl_aligned16(q) && sbl_aligned16(k_cache), "sbl_decode_attn_step: unaligned");
    hipLaunchKernelGGL(decode_attn_kernel, dim3(H, B), dim3(64), 0, (hipStream_t)stream, q, ldq, k_new, v_new, ldn, k_cache,
                       v_cache, ldc, Lcap, o, ldo, n_prev, append, scale);
    SBL_LAUNCH_CHECK("sbl_decode_attn_step");
    return 0;
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
    const float4 y0 = yr[lane], y1 = yr[64 + lane];
    for (int v = wave; v < V; v += 4) {
        const float4* wr = reinterpret_cast<const float4*>(w + (long)v * DEC_D);
        const float4 a = wr[lane], c = wr[64 + lane];
        float acc = y0.x * a.x + y0.y * a.y + y0.z * a.z + y0.w * a.w;
        acc += y1.x * c.x + y1.y * c.y + y1.z * c.z + y1.w * c.w;
        acc = wave_sum(acc);
        if (lane == 0) s_logit[v] = acc;
    }
    __syncthreads();
    if (wave == 0) {
        float best = lane < V ? s_logit[lane] : -INFINITY;
        int bi = lane < V ? lane : 0x7fffffff;
        if (logits && lane < V) logits[(long)b * ldl + lane] = best;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > best || (ov == best && oi < bi)) {
                best = ov;
                bi = oi;
            }
        }
        if (lane == 0) {
            const int t = bi == 0x7fffffff ? 0 : bi;      // all-NaN row: torch would return the NaN's index; ids stay in range
            ys[(long)b * ldys + step + 1] = t;
            s_tok = t;
        }
    }
    __syncthreads();
    if (x_next) {      // (uniform) the next step's input row
        const long t = s_tok;
        const float* er = emb + t * DEC_D;
        const float* pr = pe + (long)(step + 1) * DEC_D;
        for (int d = threadIdx.x; d < DEC_D; d += 256) x_next[(long)b * DEC_D + d] = er[d] * emb_scale + pr[d];
    }
}

extern "C" int sbl_decode_tail(const float* y, long ldy, const float* w, float* logits, long ldl, int64_t* ys, long ldys, int step,
                               const float* emb, const float* pe, int pe_rows, float emb_scale, float* x_next, int B, int V, int D,
                               sbl_stream_t stream) {
    SBL_REQUIRE(D == DEC_D, "sbl_decode_tail: D=%d (built for %d)", D, DEC_D);
    SBL_REQUIRE(B > 0 && V >= 1 && V <= 64, "sbl_decode_tail: B=%d V=%d (V <= 64)", B, V);
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
