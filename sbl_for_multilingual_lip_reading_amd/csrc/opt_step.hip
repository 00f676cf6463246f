// Device-side optimizer step: gradient sum of squares -> (norm, clip coefficient, step count, rate, bias corrections, skip
// flag) in a double[8] state buffer -> Adam that reads every per-step scalar from that buffer.  Nothing returns to the host
// between the three launches, so zero_grad + forward + backward + update can be captured as one hipGraph.  The Adam launch
// can also keep an exponential moving average of the weights (sbl_adam_ema_step_dev), and sbl_swap_f32 exchanges live and
// averaged weights in place for evaluation.
#include "sbl_common.h"

#include <math.h>

// one block per 256 float4; at most SBL_OPT_MAX_BLOCKS blocks (the Python side mirrors this to size the workspace)
static inline int opt_grid(long n) {
    const long g = ((n + 3) / 4 + 255) / 256;
    return (int)(g > SBL_OPT_MAX_BLOCKS ? SBL_OPT_MAX_BLOCKS : (g < 1 ? 1 : g));
}
static inline bool opt_aligned8(const void* p) { return (((uintptr_t)p) & 7) == 0; }

// torch.clamp's rule: both comparisons are false for NaN, so NaN stays NaN; +-inf becomes +-c.  (fminf(fmaxf(x, -c), c)
// would turn NaN into a bound and hide it from the non-finite guard.)  c <= 0: off.
__device__ __forceinline__ float clamp_nan(float x, float c) {
    if (c > 0.f) x = x < -c ? -c : (x > c ? c : x);
    return x;
}
// elements [4i, 4i+4): one 16-byte load when the base is aligned, four scalar loads otherwise (same element order, so
// the summation order below does not depend on the alignment)
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* __restrict__ a, long i) {
    if (VEC) return reinterpret_cast<const float4*>(a)[i];
    return make_float4(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]);
}
template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ a, long i, float4 x) {
    if (VEC) {
        reinterpret_cast<float4*>(a)[i] = x;
    } else {
        a[4 * i] = x.x, a[4 * i + 1] = x.y, a[4 * i + 2] = x.z, a[4 * i + 3] = x.w;
    }
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// 256 threads -> thread 0; fixed order: xor butterfly inside each wave, then waves 0..3 in index order
__device__ __forceinline__ double block_sum_f64(double v, double* s4) {
    v = wave_sum_f64(v);
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s4[0] + s4[1]) + s4[2]) + s4[3];
}

// ------------------------------------------------------------------ sum of squares of the clamped, scaled gradient
// No atomics and no ticket: thread (block, lane) always takes float4 number block*256 + lane + k*grid*256, k = 0, 1, ...,
// the n % 4 tail elements go to lanes 0..2 of block 0 after their loop, and the combine order is fixed, so partial[b] is a
// function of (data, n, grid) alone: two runs give the same bits.
template <bool VEC>
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, long n, float gscale, float clip,
                                                         double* __restrict__ partial) {
    __shared__ double s4[4];
    const long n4 = n >> 2;
    double acc = 0.0;
    // four trips of the grid-stride loop per iteration, loads first (one 16-byte load in flight per thread does not cover
    // the memory latency); a trip past the end contributes +0.0 four times, which leaves the accumulator's bits alone, so
    // the order of additions is that of the plain loop
    const long stride = (long)gridDim.x * 256;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += 4 * stride) {
        float4 x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = i + k * stride < n4 ? load4<VEC>(g, i + k * stride) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double a = clamp_nan(x[k].x * gscale, clip), b = clamp_nan(x[k].y * gscale, clip);
            const double c = clamp_nan(x[k].z * gscale, clip), d = clamp_nan(x[k].w * gscale, clip);
            acc += a * a;
            acc += b * b;
            acc += c * c;
            acc += d * d;
        }
    }
    if (blockIdx.x == 0 && (n4 << 2) + threadIdx.x < n) {
        const double a = clamp_nan(g[(n4 << 2) + threadIdx.x] * gscale, clip);
        acc += a * a;
    }
    const double tot = block_sum_f64(acc, s4);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}
extern "C" int sbl_grad_sumsq(const float* g, long n, float grad_scale, float clip_value, double* partials, long capacity,
                              long offset, sbl_stream_t stream) {
    SBL_REQUIRE(g && partials, "sbl_grad_sumsq: null pointer");
    SBL_REQUIRE(n > 0, "sbl_grad_sumsq: n=%ld must be positive", n);
    SBL_REQUIRE(opt_aligned8(partials) && (((uintptr_t)g) & 3) == 0, "sbl_grad_sumsq: unaligned gradient or workspace");
    const int grid = opt_grid(n);
    SBL_REQUIRE(offset >= 0 && offset + grid <= capacity, "sbl_grad_sumsq: workspace of %ld doubles too small for %d partials at offset %ld",
                capacity, grid, offset);
    if (sbl_aligned16(g))
        hipLaunchKernelGGL(grad_sumsq_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, g, n, grad_scale, clip_value,
                           partials + offset);
    else
        hipLaunchKernelGGL(grad_sumsq_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, g, n, grad_scale, clip_value,
                           partials + offset);
    SBL_LAUNCH_CHECK("sbl_grad_sumsq");
    return 0;
}

// ------------------------------------------------------------------ finalize: one block
// beta^t rounded to nearest, by binary powering in double-double (about 100 bits): the host path (sbl_adam_step) takes
// 1 - pow(beta, t), where one ulp of pow is 49 ulp of the difference at beta2 = 0.98, t = 1, so a device pow() that is
// "only" 1-2 ulp off would not reproduce the host's bias corrections.
struct dd {
    double hi, lo;
};
// Contraction is off in here: fusing `p + e` into fma(a.hi, b.hi, e) would count the product's rounding error twice.
__device__ __forceinline__ dd dd_mul(dd a, dd b) {
#pragma clang fp contract(off)
    const double p = a.hi * b.hi;
    double e = fma(a.hi, b.hi, -p);
    e += a.hi * b.lo + a.lo * b.hi;
    dd r;
    r.hi = p + e;
    r.lo = e - (r.hi - p);
    return r;
}
__device__ double pow_int_rn(double base, long t) {
    dd r = {1.0, 0.0}, b = {base, 0.0};
    while (t > 0) {
        if (t & 1) r = dd_mul(r, b);
        b = dd_mul(b, b);
        t >>= 1;
    }
    return r.hi;
}
// t^-1/2 for an integer-valued t >= 1: 1 / sqrt(t) (two roundings) plus one Newton correction with an exact residual
__device__ double rsqrt_refined(double t) {
#pragma clang fp contract(off)
    const double y = 1.0 / sqrt(t);
    const double yy = y * y, yy_lo = fma(y, y, -yy);
    const double r = fma(-t, yy, 1.0) - t * yy_lo;      // 1 - t y^2
    return fma(y, 0.5 * r, y);
}

// The sum of squares of finite floats cannot overflow a double (n * 1.2e77 << 1.8e308), so !isfinite(sum) holds exactly
// when some clamped element is +-inf or NaN: the sum doubles as the non-finite detector and no counting pass is needed.
// Summation order: thread j adds partials j, j + 256, ... in increasing index, then the fixed block combine above - a
// function of nparts alone.
__global__ __launch_bounds__(256) void opt_finalize_kernel(double* __restrict__ st, const double* __restrict__ partial,
                                                           long nparts, double max_norm, int skip_nonfinite, double noam_scale,
                                                           double warm_pow, double b1, double b2) {
    __shared__ double s4[4];
    double acc = 0.0;
    for (long i = threadIdx.x; i < nparts; i += 256) acc += partial[i];
    const double sum = block_sum_f64(acc, s4);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(sum);
    const bool finite = isfinite(sum);
    // torch.nn.utils.clip_grad_norm_: coef = clamp(max_norm / (norm + 1e-6), max = 1)
    const double coef = max_norm > 0.0 ? fmin(1.0, max_norm / (norm + 1e-6)) : 1.0;
    st[SBL_OPT_GRAD_NORM] = norm;
    st[SBL_OPT_CLIP_COEF] = coef;
    if (finite || !skip_nonfinite) {
        const double t = st[SBL_OPT_STEP] + 1.0;
        double lr = st[SBL_OPT_LR];
        if (noam_scale > 0.0) lr = noam_scale * fmin(rsqrt_refined(t), t * warm_pow);
        st[SBL_OPT_STEP] = t;
        st[SBL_OPT_LR] = lr;
        st[SBL_OPT_STEP_SIZE] = lr / (1.0 - pow_int_rn(b1, (long)t));
        st[SBL_OPT_INV_SQRT_BC2] = 1.0 / sqrt(1.0 - pow_int_rn(b2, (long)t));
        st[SBL_OPT_SKIP] = 0.0;
    } else {
        st[SBL_OPT_SKIPPED] += 1.0;
        st[SBL_OPT_SKIP] = 1.0;
    }
}
extern "C" int sbl_opt_finalize(double* state, const double* partials, long nparts, double max_norm, int skip_nonfinite,
                                double noam_k, double noam_warmup, float beta1, float beta2, sbl_stream_t stream) {
    SBL_REQUIRE(state && partials, "sbl_opt_finalize: null pointer");
    SBL_REQUIRE(nparts > 0, "sbl_opt_finalize: nparts=%ld must be positive", nparts);
    SBL_REQUIRE(opt_aligned8(state) && opt_aligned8(partials), "sbl_opt_finalize: unaligned state or workspace");
    SBL_REQUIRE((noam_k > 0.0) == (noam_warmup > 0.0), "sbl_opt_finalize: Noam schedule needs k > 0 and warmup > 0 (or both 0: off)");
    SBL_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "sbl_opt_finalize: betas outside [0, 1)");
    // the host's own arithmetic for the constants of TransformerOptimizer._update_lr: k * 512^-0.5 and warmup^-1.5
    const double scale = noam_k > 0.0 ? noam_k * pow(512.0, -0.5) : 0.0;
    const double warm_pow = noam_k > 0.0 ? pow(noam_warmup, -1.5) : 0.0;
    hipLaunchKernelGGL(opt_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, state, partials, nparts, max_norm,
                       skip_nonfinite, scale, warm_pow, (double)beta1, (double)beta2);
    SBL_LAUNCH_CHECK("sbl_opt_finalize");
    return 0;
}

// ------------------------------------------------------------------ Adam, per-step scalars from the state buffer
// g' = clamp(g * gscale) * coef, then adam_kernel's arithmetic (misc.hip) in its order.  A skipped step returns before the
// first store: p, m, v keep their bits.
// One element of the update; both Adam kernels below expand it, so their p, m, v agree bit for bit.  It reads gscale,
// clip, coef, b1, b2, step_size, inv_sqrt_bc2 and eps from the kernel that expands it.
#define SBL_ADAM_ONE(P, G, M, V)                                         \
    do {                                                                 \
        const float gi = clamp_nan((G) * gscale, clip) * coef;           \
        const float mi = b1 * (M) + (1.f - b1) * gi;                     \
        const float vi = b2 * (V) + (1.f - b2) * gi * gi;                \
        (M) = mi;                                                        \
        (V) = vi;                                                        \
        (P) -= step_size * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);        \
    } while (0)
template <bool VEC>
__global__ __launch_bounds__(256) void adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, long n, const double* __restrict__ st, float b1,
                                                       float b2, float eps, float gscale, float clip) {
    if (st[SBL_OPT_SKIP] != 0.0) return;
    const float coef = (float)st[SBL_OPT_CLIP_COEF];
    const float step_size = (float)st[SBL_OPT_STEP_SIZE], inv_sqrt_bc2 = (float)st[SBL_OPT_INV_SQRT_BC2];
    const long n4 = n >> 2;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 g4 = load4<VEC>(g, i);
        float4 p4 = load4<VEC>(p, i), m4 = load4<VEC>(m, i), v4 = load4<VEC>(v, i);
        SBL_ADAM_ONE(p4.x, g4.x, m4.x, v4.x);
        SBL_ADAM_ONE(p4.y, g4.y, m4.y, v4.y);
        SBL_ADAM_ONE(p4.z, g4.z, m4.z, v4.z);
        SBL_ADAM_ONE(p4.w, g4.w, m4.w, v4.w);
        store4<VEC>(m, i, m4);
        store4<VEC>(v, i, v4);
        store4<VEC>(p, i, p4);
    }
    const long j = (n4 << 2) + threadIdx.x;
    if (blockIdx.x == 0 && j < n) {
        float pj = p[j], mj = m[j], vj = v[j];
        SBL_ADAM_ONE(pj, g[j], mj, vj);
        m[j] = mj;
        v[j] = vj;
        p[j] = pj;
    }
}
extern "C" int sbl_adam_step_dev(float* p, const float* g, float* m, float* v, long n, const double* state, float beta1,
                                 float beta2, float eps, float grad_scale, float clip_value, sbl_stream_t stream) {
    SBL_REQUIRE(p && g && m && v && state, "sbl_adam_step_dev: null pointer");
    SBL_REQUIRE(n > 0, "sbl_adam_step_dev: n=%ld must be positive", n);
    SBL_REQUIRE(opt_aligned8(state), "sbl_adam_step_dev: unaligned state buffer");
    SBL_REQUIRE(((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 3) == 0, "sbl_adam_step_dev: unaligned buffer");
    const int grid = opt_grid(n);
    if (sbl_aligned16(p) && sbl_aligned16(g) && sbl_aligned16(m) && sbl_aligned16(v))
        hipLaunchKernelGGL(adam_dev_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, state, beta1, beta2,
                           eps, grad_scale, clip_value);
    else
        hipLaunchKernelGGL(adam_dev_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, state, beta1, beta2,
                           eps, grad_scale, clip_value);
    SBL_LAUNCH_CHECK("sbl_adam_step_dev");
    return 0;
}

// ------------------------------------------------------------------ Adam + exponential moving average of the weights
// SBL_ADAM_ONE for p, m, v (adam_dev_kernel's bits), then e += w * (p_new - e) in fp32: the difference is rounded, the
// product and the sum are one fused multiply-add.  w = (float)(1 - d_t) with d_t in double from t = st[SBL_OPT_STEP], the
// count sbl_opt_finalize has already advanced: d_t = min(decay, (1 + t) / (10 + t)) under warm-up, else decay.  Every
// thread derives w itself (two double operations): no launch and no state slot of its own.  A skipped step returns before
// the first store: p, m, v, e keep their bits.
template <bool VEC>
__global__ __launch_bounds__(256) void adam_ema_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, float* __restrict__ e, long n,
                                                           const double* __restrict__ st, float b1, float b2, float eps,
                                                           float gscale, float clip, double decay, int warm) {
    if (st[SBL_OPT_SKIP] != 0.0) return;
    const float coef = (float)st[SBL_OPT_CLIP_COEF];
    const float step_size = (float)st[SBL_OPT_STEP_SIZE], inv_sqrt_bc2 = (float)st[SBL_OPT_INV_SQRT_BC2];
    const double t = st[SBL_OPT_STEP];
    const double d_t = warm ? fmin(decay, (1.0 + t) / (10.0 + t)) : decay;
    const float w = (float)(1.0 - d_t);
    const long n4 = n >> 2;
#define SBL_EMA_ONE(E, P) (E) = __fmaf_rn(w, (P) - (E), (E))
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 g4 = load4<VEC>(g, i);
        float4 p4 = load4<VEC>(p, i), m4 = load4<VEC>(m, i), v4 = load4<VEC>(v, i), e4 = load4<VEC>(e, i);
        SBL_ADAM_ONE(p4.x, g4.x, m4.x, v4.x);
        SBL_ADAM_ONE(p4.y, g4.y, m4.y, v4.y);
        SBL_ADAM_ONE(p4.z, g4.z, m4.z, v4.z);
        SBL_ADAM_ONE(p4.w, g4.w, m4.w, v4.w);
        SBL_EMA_ONE(e4.x, p4.x);
        SBL_EMA_ONE(e4.y, p4.y);
        SBL_EMA_ONE(e4.z, p4.z);
        SBL_EMA_ONE(e4.w, p4.w);
        store4<VEC>(m, i, m4);
        store4<VEC>(v, i, v4);
        store4<VEC>(p, i, p4);
        store4<VEC>(e, i, e4);
    }
    const long j = (n4 << 2) + threadIdx.x;
    if (blockIdx.x == 0 && j < n) {
        float pj = p[j], mj = m[j], vj = v[j], ej = e[j];
        SBL_ADAM_ONE(pj, g[j], mj, vj);
        SBL_EMA_ONE(ej, pj);
        m[j] = mj;
        v[j] = vj;
        p[j] = pj;
        e[j] = ej;
    }
#undef SBL_EMA_ONE
}
#undef SBL_ADAM_ONE
extern "C" int sbl_adam_ema_step_dev(float* p, const float* g, float* m, float* v, float* e, long n, const double* state,
                                     float beta1, float beta2, float eps, float grad_scale, float clip_value, double ema_decay,
                                     int ema_warmup, sbl_stream_t stream) {
    SBL_REQUIRE(p && g && m && v && e && state, "sbl_adam_ema_step_dev: null pointer");
    SBL_REQUIRE(n > 0, "sbl_adam_ema_step_dev: n=%ld must be positive", n);
    SBL_REQUIRE(opt_aligned8(state), "sbl_adam_ema_step_dev: unaligned state buffer");
    SBL_REQUIRE(((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v) | ((uintptr_t)e)) & 3) == 0,
                "sbl_adam_ema_step_dev: unaligned buffer");
    SBL_REQUIRE(ema_decay > 0.0 && ema_decay < 1.0, "sbl_adam_ema_step_dev: ema_decay=%g outside (0, 1)", ema_decay);
    const int grid = opt_grid(n);
    if (sbl_aligned16(p) && sbl_aligned16(g) && sbl_aligned16(m) && sbl_aligned16(v) && sbl_aligned16(e))
        hipLaunchKernelGGL(adam_ema_dev_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, e, n, state, beta1,
                           beta2, eps, grad_scale, clip_value, ema_decay, ema_warmup);
    else
        hipLaunchKernelGGL(adam_ema_dev_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, e, n, state, beta1,
                           beta2, eps, grad_scale, clip_value, ema_decay, ema_warmup);
    SBL_LAUNCH_CHECK("sbl_adam_ema_step_dev");
    return 0;
}

// ------------------------------------------------------------------ exchange of two buffers
// a[i] <-> b[i]: every element is loaded from both sides by the one thread that then stores it to both, so the exchange
// is exact and needs no scratch; the ranges must not overlap (the host refuses).
template <bool VEC>
__global__ __launch_bounds__(256) void swap_kernel(float* __restrict__ a, float* __restrict__ b, long n) {
    const long n4 = n >> 2;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 a4 = load4<VEC>(a, i), b4 = load4<VEC>(b, i);
        store4<VEC>(a, i, b4);
        store4<VEC>(b, i, a4);
    }
    const long j = (n4 << 2) + threadIdx.x;
    if (blockIdx.x == 0 && j < n) {
        const float aj = a[j], bj = b[j];
        a[j] = bj;
        b[j] = aj;
    }
}
extern "C" int sbl_swap_f32(float* a, float* b, long n, sbl_stream_t stream) {
    SBL_REQUIRE(a && b, "sbl_swap_f32: null pointer");
    SBL_REQUIRE(n > 0, "sbl_swap_f32: n=%ld must be positive", n);
    SBL_REQUIRE(((((uintptr_t)a) | ((uintptr_t)b)) & 3) == 0, "sbl_swap_f32: unaligned buffer");
    const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, bytes = (uintptr_t)n * 4;
    SBL_REQUIRE(ua < ub ? ub - ua >= bytes : ua - ub >= bytes, "sbl_swap_f32: the two ranges of %ld elements overlap", n);
    const int grid = opt_grid(n);
    if (sbl_aligned16(a) && sbl_aligned16(b))
        hipLaunchKernelGGL(swap_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, b, n);
    else
        hipLaunchKernelGGL(swap_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, b, n);
    SBL_LAUNCH_CHECK("sbl_swap_f32");
    return 0;
}
