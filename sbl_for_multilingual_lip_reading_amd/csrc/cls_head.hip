// Classification heads of the stage-1 pre-training model (CLS/transformer/transformer.py:31-35, restated as in
// oracle.sbl_oracle.cls_forward) and their cross-entropy loss (CLS/train.py:115-130).
//
// Shapes: enc (N, T, 512); fc_1500 = (W1 (C1, 512), b1); fc_2 = (W2 (C2, 512), b2).
//   logits1 = mean_t(enc) W1^T + b1,   logits2 = enc[:, lang_index] W2^T + b2
//   loss    = CE(logits1, tgt1) + w CE(logits2, tgt2)   (each CE a mean over rows whose target is not ignore_id)
//
// About 50 MFLOP and one 3 MB operand (W1): the cost is launches, so forward = 2 launches, loss forward 1, loss backward 1,
// head backward 1.  Every workgroup that touches W1 owns a slice of CLS_CB classes, so W1 is read once per launch and dW1
// written once.  Hand-offs between workgroups happen only at kernel boundaries.  Plain fp32 FMA throughout, independent of
// sbl_set_matmul_precision.  Deterministic: no atomics; every sum runs over its terms in a fixed order.
#include "sbl_common.h"

#define CLS_D 512          // model width (the only one the heads are built for)
#define CLS_CB 8           // classes of fc_1500 per workgroup: 188 workgroups at C1 = 1500
#define CLS_RC 4           // clips per input-gradient workgroup
#define CLS_DS 64          // feature columns per input-gradient workgroup
#define CLS_KC 512         // classes per LDS chunk of the input-gradient workgroups
#define CLS_MAX_C2 16
static_assert(CLS_RC == 4, "the input-gradient workgroups hand one clip to each of their four wavefronts");

// ------------------------------------------------------------------ forward 1: mean over time
// pooled[n, :] = sum_t enc[n, t, :] / T (t ascending), written row-major (saved for backward) and transposed (D, N) for
// the logits kernel, whose lanes run over clips.
__global__ __launch_bounds__(128) void cls_pool_kernel(const float* __restrict__ enc, float* __restrict__ pooled,
                                                       float* __restrict__ pooled_t, int N, int T) {
    const int n = blockIdx.x;
    const int d = threadIdx.x * 4;
    const float* src = enc + (long)n * T * CLS_D + d;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < T; ++t) s += *(const f32x4*)(src + (long)t * CLS_D);
    const float fT = (float)T;
    const f32x4 m = {s.x / fT, s.y / fT, s.z / fT, s.w / fT};
    *(f32x4*)(pooled + (long)n * CLS_D + d) = m;
    pooled_t[(long)(d + 0) * N + n] = m.x;
    pooled_t[(long)(d + 1) * N + n] = m.y;
    pooled_t[(long)(d + 2) * N + n] = m.z;
    pooled_t[(long)(d + 3) * N + n] = m.w;
}

// ------------------------------------------------------------------ forward 2: both heads' logits
// Workgroups [0, nslice): classes [CLS_CB*b, CLS_CB*b + CLS_CB) of fc_1500 for every clip.  Lanes run over 64 clips (coalesced
// pooled_t reads), the four wavefronts over quarters of D with the slice's weights as LDS broadcasts; the quarters are added
// in LDS in a fixed order.  Workgroup nslice: fc_2 on row lang_index of every clip, one wavefront per clip, lanes over D.
__global__ __launch_bounds__(256) void cls_logits_kernel(const float* __restrict__ enc, const float* __restrict__ pooled_t,
                                                         const float* __restrict__ w1, const float* __restrict__ b1,
                                                         const float* __restrict__ w2, const float* __restrict__ b2,
                                                         float* __restrict__ logits1, float* __restrict__ logits2, int N, int T,
                                                         int li, int C1, int C2, int nslice) {
    __shared__ float wt[CLS_D][CLS_CB];                 // 16 KB: the slice's rows of W1, transposed
    __shared__ float part[4][64][CLS_CB + 1];           // per-quarter partial sums of a 64-clip chunk
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if ((int)blockIdx.x == nslice) {
        for (int n = wv; n < N; n += 4) {
            const float* x = enc + ((long)n * T + li) * CLS_D;
            const f32x4 xa = *(const f32x4*)(x + lane * 4), xb = *(const f32x4*)(x + 256 + lane * 4);
            for (int j = 0; j < C2; ++j) {
                const float* w = w2 + (long)j * CLS_D;
                const f32x4 wa = *(const f32x4*)(w + lane * 4), wb = *(const f32x4*)(w + 256 + lane * 4);
                float s = xa.x * wa.x;
                s = fmaf(xa.y, wa.y, s);
                s = fmaf(xa.z, wa.z, s);
                s = fmaf(xa.w, wa.w, s);
                s = fmaf(xb.x, wb.x, s);
                s = fmaf(xb.y, wb.y, s);
                s = fmaf(xb.z, wb.z, s);
                s = fmaf(xb.w, wb.w, s);
                s = wave_sum(s);
                if (lane == 0) logits2[(long)n * C2 + j] = s + b2[j];
            }
        }
        return;
    }
    const int c0 = blockIdx.x * CLS_CB;
    for (int i = tid; i < CLS_D * CLS_CB; i += 256) {
        const int c = i / CLS_D, d = i % CLS_D;
        wt[d][c] = (c0 + c < C1) ? w1[(long)(c0 + c) * CLS_D + d] : 0.f;
    }
    __syncthreads();
    const int dlo = wv * (CLS_D / 4);
    for (int r0 = 0; r0 < N; r0 += 64) {
        const int r = r0 + lane;
        float acc[CLS_CB];
#pragma unroll
        for (int c = 0; c < CLS_CB; ++c) acc[c] = 0.f;
        if (r < N) {
            const float* p = pooled_t + (long)dlo * N + r;
#pragma unroll 4
            for (int d = 0; d < CLS_D / 4; ++d) {
                const float x = p[(long)d * N];
#pragma unroll
                for (int c = 0; c < CLS_CB; ++c) acc[c] = fmaf(x, wt[dlo + d][c], acc[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < CLS_CB; ++c) part[wv][lane][c] = acc[c];
        __syncthreads();
        for (int o = tid; o < 64 * CLS_CB; o += 256) {
            const int rr = o / CLS_CB, c = o % CLS_CB;
            const int row = r0 + rr;
            if (row < N && c0 + c < C1) {
                float s = part[0][rr][c] + part[1][rr][c];
                s += part[2][rr][c];
                s += part[3][rr][c];
                logits1[(long)row * C1 + c0 + c] = s + b1[c0 + c];
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ cross entropy of one row (one wavefront)
// loss = logsumexp(x) - x[g]; correct = (argmax x == g), ties to the lowest index.  A target outside [0, C) is never used
// as an index: its row's loss is NaN.  The caller reads lane 0.
__device__ __forceinline__ void cls_ce_row(const float* __restrict__ x, int C, long g, int lane, float& loss, float& correct) {
    float mx = -INFINITY;
    int am = 0x7fffffff;
    for (int c = lane; c < C; c += 64) {
        const float v = x[c];
        if (v > mx) {
            mx = v;
            am = c;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(mx, o, 64);
        const int oi = __shfl_xor(am, o, 64);
        if (ov > mx || (ov == mx && oi < am)) {
            mx = ov;
            am = oi;
        }
    }
    float se = 0.f, xg = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float v = x[c];
        se += expf(v - mx);
        if (c == g) xg = v;
    }
    se = wave_sum(se);
    xg = wave_sum(xg);
    loss = (g >= 0 && g < C) ? (logf(se) + mx) - xg : __int_as_float(0x7fc00000);
    correct = (am == g) ? 1.f : 0.f;
}

// ------------------------------------------------------------------ loss forward: one workgroup, no atomics
// Wavefront w takes rows w, w+16, ... in order; the 16 wavefront partials are added in order by thread 0.
// stats = {sum of head-1 row losses, head-1 valid rows, head-1 correct, the same three for head 2};
// loss = stats[0]/stats[1] + w * stats[3]/stats[4] (NaN when a head has no valid row, like torch's mean reduction).
__global__ __launch_bounds__(1024) void cls_loss_fwd_kernel(const float* __restrict__ l1, const float* __restrict__ l2,
                                                            const int64_t* __restrict__ t1, const int64_t* __restrict__ t2,
                                                            int N, int C1, int C2, float lw, int ignore_id,
                                                            float* __restrict__ loss, float* __restrict__ stats) {
    __shared__ float red[16][6];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int n = wv; n < N; n += 16) {
        float l, k;
        const long g1 = t1[n], g2 = t2[n];
        if (g1 != ignore_id) {
            cls_ce_row(l1 + (long)n * C1, C1, g1, lane, l, k);
            a[0] += l;
            a[1] += 1.f;
            a[2] += k;
        }
        if (g2 != ignore_id) {
            cls_ce_row(l2 + (long)n * C2, C2, g2, lane, l, k);
            a[3] += l;
            a[4] += 1.f;
            a[5] += k;
        }
    }
    if (lane == 0)
        for (int i = 0; i < 6; ++i) red[wv][i] = a[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        float s[6];
        for (int i = 0; i < 6; ++i) {
            s[i] = red[0][i];
            for (int w = 1; w < 16; ++w) s[i] += red[w][i];
            stats[i] = s[i];
        }
        loss[0] = s[0] / s[1] + lw * (s[3] / s[4]);
    }
}

// ------------------------------------------------------------------ loss backward: one wavefront per clip, both heads
// dlogits = scale * (softmax - onehot) with scale = gscale[0] / n_valid (head 1) and gscale[0] * w / n_valid (head 2);
// ignored rows get 0.
__device__ __forceinline__ void cls_ce_bwd_row(const float* __restrict__ x, float* __restrict__ dx, int C, long g, int ignore_id,
                                               float scale, int lane) {
    if (g == ignore_id) {
        for (int c = lane; c < C; c += 64) dx[c] = 0.f;
        return;
    }
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, x[c]);
    mx = wave_max(mx);
    float se = 0.f;
    for (int c = lane; c < C; c += 64) se += expf(x[c] - mx);
    se = __shfl(wave_sum(se), 0, 64);
    for (int c = lane; c < C; c += 64) dx[c] = scale * (expf(x[c] - mx) / se - (c == g ? 1.f : 0.f));
}

__global__ __launch_bounds__(256) void cls_loss_bwd_kernel(const float* __restrict__ l1, const float* __restrict__ l2,
                                                           const int64_t* __restrict__ t1, const int64_t* __restrict__ t2,
                                                           int N, int C1, int C2, float lw, int ignore_id,
                                                           const float* __restrict__ stats, const float* __restrict__ gscale,
                                                           float* __restrict__ d1, float* __restrict__ d2) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const float g = gscale[0];
    cls_ce_bwd_row(l1 + (long)n * C1, d1 + (long)n * C1, C1, t1[n], ignore_id, g / stats[1], lane);
    cls_ce_bwd_row(l2 + (long)n * C2, d2 + (long)n * C2, C2, t2[n], ignore_id, g * lw / stats[4], lane);
}

// ------------------------------------------------------------------ head backward: one launch, three kinds of workgroup
//  [0, nw1)             dW1 / db1 for classes [CLS_CB*b, +CLS_CB): a thread owns two feature columns and runs over the clips
//                       in order, the slice of dlogits1 staged in LDS 256 clips at a time;
//  [nw1, nw1 + nw2)     dW2 / db2 (at most one workgroup);
//  [nw1 + nw2, ...)     d_enc for CLS_RC clips x CLS_DS columns: dpooled = dlogits1 W1 (the four wavefronts take quarters
//                       of each CLS_KC-class chunk, added in LDS in order), d_enc[n, t] = dpooled / T, plus dlogits2 W2 on
//                       t == lang_index.
// accumulate: parameter gradients += (persistent flat gradient buffers) instead of =.  A gradient pointer may be NULL: it is
// not computed (and its workgroups are not launched).
__global__ __launch_bounds__(256) void cls_head_bwd_kernel(const float* __restrict__ enc, const float* __restrict__ pooled,
                                                           const float* __restrict__ d1, const float* __restrict__ d2,
                                                           const float* __restrict__ w1, const float* __restrict__ w2,
                                                           float* __restrict__ d_enc, float* __restrict__ dw1,
                                                           float* __restrict__ db1, float* __restrict__ dw2,
                                                           float* __restrict__ db2, int N, int T, int li, int C1, int C2,
                                                           int accumulate, int nw1, int nw2) {
    __shared__ float dls[256][CLS_CB];                                   // dW1: 256 clips of the slice's dlogits1
    __shared__ __attribute__((aligned(16))) float dlt[CLS_KC][CLS_RC];   // d_enc: one class chunk of the clips, class-major
    __shared__ float part[4][CLS_RC][CLS_DS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.x;
    if (b < nw1) {
        const int c0 = b * CLS_CB;
        float acc0[CLS_CB], acc1[CLS_CB];
#pragma unroll
        for (int c = 0; c < CLS_CB; ++c) acc0[c] = acc1[c] = 0.f;
        float bsum = 0.f;
        for (int r0 = 0; r0 < N; r0 += 256) {
            const int rn = min(256, N - r0);
            for (int i = tid; i < 256 * CLS_CB; i += 256) {
                const int rr = i / CLS_CB, c = i % CLS_CB;
                dls[rr][c] = (rr < rn && c0 + c < C1) ? d1[(long)(r0 + rr) * C1 + c0 + c] : 0.f;
            }
            __syncthreads();
            const float* p = pooled + (long)r0 * CLS_D + 2 * tid;
            for (int rr = 0; rr < rn; ++rr) {
                const float2 x = *(const float2*)(p + (long)rr * CLS_D);
#pragma unroll
                for (int c = 0; c < CLS_CB; ++c) {
                    acc0[c] = fmaf(dls[rr][c], x.x, acc0[c]);
                    acc1[c] = fmaf(dls[rr][c], x.y, acc1[c]);
                }
            }
            if (tid < CLS_CB)
                for (int rr = 0; rr < rn; ++rr) bsum += dls[rr][tid];
            __syncthreads();
        }
        if (dw1) {
#pragma unroll
            for (int c = 0; c < CLS_CB; ++c) {
                if (c0 + c < C1) {
                    float2* o = (float2*)(dw1 + (long)(c0 + c) * CLS_D + 2 * tid);
                    float2 v = make_float2(acc0[c], acc1[c]);
                    if (accumulate) {
                        const float2 old = *o;
                        v.x += old.x;
                        v.y += old.y;
                    }
                    *o = v;
                }
            }
        }
        if (db1 && tid < CLS_CB && c0 + tid < C1) db1[c0 + tid] = accumulate ? db1[c0 + tid] + bsum : bsum;
        return;
    }
    if (b < nw1 + nw2) {
        float acc0[CLS_MAX_C2], acc1[CLS_MAX_C2];
#pragma unroll
        for (int j = 0; j < CLS_MAX_C2; ++j) acc0[j] = acc1[j] = 0.f;
        for (int n = 0; n < N; ++n) {
            const float2 x = *(const float2*)(enc + ((long)n * T + li) * CLS_D + 2 * tid);
#pragma unroll
            for (int j = 0; j < CLS_MAX_C2; ++j) {
                if (j < C2) {
                    const float g = d2[(long)n * C2 + j];
                    acc0[j] = fmaf(g, x.x, acc0[j]);
                    acc1[j] = fmaf(g, x.y, acc1[j]);
                }
            }
        }
        if (dw2) {
#pragma unroll
            for (int j = 0; j < CLS_MAX_C2; ++j) {
                if (j < C2) {
                    float2* o = (float2*)(dw2 + (long)j * CLS_D + 2 * tid);
                    float2 v = make_float2(acc0[j], acc1[j]);
                    if (accumulate) {
                        const float2 old = *o;
                        v.x += old.x;
                        v.y += old.y;
                    }
                    *o = v;
                }
            }
        }
        if (db2 && tid < C2) {
            float s = 0.f;
            for (int n = 0; n < N; ++n) s += d2[(long)n * C2 + tid];
            db2[tid] = accumulate ? db2[tid] + s : s;
        }
        return;
    }
    const int e = b - nw1 - nw2;
    const int n0 = (e / (CLS_D / CLS_DS)) * CLS_RC;
    const int d = (e % (CLS_D / CLS_DS)) * CLS_DS + lane;
    float acc[CLS_RC];
#pragma unroll
    for (int r = 0; r < CLS_RC; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < C1; k0 += CLS_KC) {
        const int kn = min(CLS_KC, C1 - k0);
        for (int i = tid; i < CLS_KC * CLS_RC; i += 256) {
            const int r = i / CLS_KC, c = i % CLS_KC;
            dlt[c][r] = (c < kn && n0 + r < N) ? d1[(long)(n0 + r) * C1 + k0 + c] : 0.f;
        }
        __syncthreads();
        const int cb = wv * (CLS_KC / 4), ce = min(cb + CLS_KC / 4, kn);
        const float* w = w1 + (long)k0 * CLS_D + d;
#pragma unroll 4
        for (int c = cb; c < ce; ++c) {
            const float x = w[(long)c * CLS_D];
            const f32x4 g = *(const f32x4*)&dlt[c][0];
            acc[0] = fmaf(g.x, x, acc[0]);
            acc[1] = fmaf(g.y, x, acc[1]);
            acc[2] = fmaf(g.z, x, acc[2]);
            acc[3] = fmaf(g.w, x, acc[3]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < CLS_RC; ++r) part[wv][r][lane] = acc[r];
    __syncthreads();
    const int n = n0 + wv;          // wavefront r writes clip n0 + r
    if (n >= N || !d_enc) return;
    float dp = part[0][wv][lane] + part[1][wv][lane];
    dp += part[2][wv][lane];
    dp += part[3][wv][lane];
    dp = dp / (float)T;
    float ql = 0.f;
    for (int j = 0; j < C2; ++j) ql = fmaf(d2[(long)n * C2 + j], w2[(long)j * CLS_D + d], ql);
    float* o = d_enc + (long)n * T * CLS_D + d;
    for (int t = 0; t < T; ++t) o[(long)t * CLS_D] = (t == li) ? dp + ql : dp;
}

// ------------------------------------------------------------------ host entry points
static int cls_check_dims(const char* who, int N, int T, int D, int C1, int C2, int lang_index) {
    SBL_REQUIRE(N > 0, "%s: N = %d clips (must be >= 1)", who, N);
    SBL_REQUIRE(T > 0, "%s: T = %d frames (must be >= 1)", who, T);
    SBL_REQUIRE(D == CLS_D, "%s: D = %d (the heads are built for D = %d)", who, D, CLS_D);
    SBL_REQUIRE(lang_index >= 0 && lang_index < T, "%s: lang_index = %d outside [0, T = %d)", who, lang_index, T);
    SBL_REQUIRE(C1 > 0 && C2 > 0 && C2 <= CLS_MAX_C2, "%s: C1 = %d, C2 = %d classes (need C1 >= 1, 1 <= C2 <= %d)", who, C1,
                C2, CLS_MAX_C2);
    return 0;
}

static int cls_check_loss(const char* who, int N, int C1, int C2) {
    SBL_REQUIRE(N > 0, "%s: N = %d clips (must be >= 1)", who, N);
    SBL_REQUIRE(C1 > 0 && C2 > 0, "%s: C1 = %d, C2 = %d classes (must be >= 1)", who, C1, C2);
    return 0;
}

extern "C" int sbl_cls_head_fwd(const float* enc, const float* w1, const float* b1, const float* w2, const float* b2,
                                float* pooled, float* pooled_t, float* logits1, float* logits2, int N, int T, int D, int C1,
                                int C2, int lang_index, sbl_stream_t stream) {
    const char* who = "sbl_cls_head_fwd";
    const int rc = cls_check_dims(who, N, T, D, C1, C2, lang_index);
    if (rc) return rc;
    SBL_REQUIRE(enc && w1 && b1 && w2 && b2 && pooled && pooled_t && logits1 && logits2, "%s: null pointer", who);
    SBL_REQUIRE(sbl_aligned16(enc) && sbl_aligned16(w1) && sbl_aligned16(w2) && sbl_aligned16(pooled),
                "%s: enc, w1, w2 and pooled must be 16-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cls_pool_kernel, dim3(N), dim3(128), 0, s, enc, pooled, pooled_t, N, T);
    SBL_LAUNCH_CHECK(who);
    const int nslice = sbl_cdiv(C1, CLS_CB);
    hipLaunchKernelGGL(cls_logits_kernel, dim3(nslice + 1), dim3(256), 0, s, enc, pooled_t, w1, b1, w2, b2, logits1, logits2, N,
                       T, lang_index, C1, C2, nslice);
    SBL_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int sbl_cls_loss_fwd(const float* logits1, const float* logits2, const int64_t* tgt1, const int64_t* tgt2, int N,
                                int C1, int C2, float lang_weight, int ignore_id, float* loss, float* stats6,
                                sbl_stream_t stream) {
    const char* who = "sbl_cls_loss_fwd";
    const int rc = cls_check_loss(who, N, C1, C2);
    if (rc) return rc;
    SBL_REQUIRE(logits1 && logits2 && tgt1 && tgt2 && loss && stats6, "%s: null pointer", who);
    hipLaunchKernelGGL(cls_loss_fwd_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, logits1, logits2, tgt1, tgt2, N, C1, C2,
                       lang_weight, ignore_id, loss, stats6);
    SBL_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int sbl_cls_loss_bwd(const float* logits1, const float* logits2, const int64_t* tgt1, const int64_t* tgt2,
                                const float* stats6, const float* gscale, float* dlogits1, float* dlogits2, int N, int C1,
                                int C2, float lang_weight, int ignore_id, sbl_stream_t stream) {
    const char* who = "sbl_cls_loss_bwd";
    const int rc = cls_check_loss(who, N, C1, C2);
    if (rc) return rc;
    SBL_REQUIRE(logits1 && logits2 && tgt1 && tgt2 && stats6 && gscale && dlogits1 && dlogits2, "%s: null pointer", who);
    hipLaunchKernelGGL(cls_loss_bwd_kernel, dim3(sbl_cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, logits1, logits2, tgt1, tgt2,
                       N, C1, C2, lang_weight, ignore_id, stats6, gscale, dlogits1, dlogits2);
    SBL_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int sbl_cls_head_bwd(const float* enc, const float* pooled, const float* dlogits1, const float* dlogits2,
                                const float* w1, const float* w2, float* d_enc, float* dw1, float* db1, float* dw2, float* db2,
                                int N, int T, int D, int C1, int C2, int lang_index, int accumulate, sbl_stream_t stream) {
    const char* who = "sbl_cls_head_bwd";
    const int rc = cls_check_dims(who, N, T, D, C1, C2, lang_index);
    if (rc) return rc;
    SBL_REQUIRE(dlogits1 && dlogits2, "%s: null pointer (dlogits1 / dlogits2)", who);
    SBL_REQUIRE(!(dw1 || db1) || pooled, "%s: null pointer (pooled, needed for dW1 / db1)", who);
    SBL_REQUIRE(!(dw2 || db2) || enc, "%s: null pointer (enc, needed for dW2 / db2)", who);
    SBL_REQUIRE(!d_enc || (w1 && w2), "%s: null pointer (w1 / w2, needed for d_enc)", who);
    SBL_REQUIRE((!pooled || sbl_aligned16(pooled)) && (!enc || sbl_aligned16(enc)) && (!w1 || sbl_aligned16(w1)) &&
                    (!dw1 || sbl_aligned16(dw1)) && (!dw2 || sbl_aligned16(dw2)),
                "%s: enc, pooled, w1, dw1 and dw2 must be 16-byte aligned", who);
    SBL_REQUIRE(accumulate == 0 || accumulate == 1, "%s: accumulate = %d (0 or 1)", who, accumulate);
    const long nw1 = (dw1 || db1) ? sbl_cdiv(C1, CLS_CB) : 0;
    const long nw2 = (dw2 || db2) ? 1 : 0;
    const long ne = d_enc ? (long)sbl_cdiv(N, CLS_RC) * (CLS_D / CLS_DS) : 0;
    SBL_REQUIRE(nw1 + nw2 + ne <= 0x7fffffffL, "%s: N = %d is too large", who, N);
    const int grid = (int)(nw1 + nw2 + ne);
    if (grid == 0) return 0;
    hipLaunchKernelGGL(cls_head_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, enc, pooled, dlogits1, dlogits2, w1,
                       w2, d_enc, dw1, db1, dw2, db2, N, T, lang_index, C1, C2, accumulate, (int)nw1, (int)nw2);
    SBL_LAUNCH_CHECK(who);
    return 0;
}
