// The two output heads of the SBL decoder as the step tails evaluate them (pair_beam.hip, lexicon.hip): a bias-free
// Linear(512, V <= 64) in plain fp32 FMA, one wavefront per (class, row) dot product, and the log-softmax of a row with
// one class per lane.  Both tails include this, so a beam total and a rescored total are sums of the same numbers.
#pragma once
#include "sbl_common.h"

#define PB_D 512          // d_model of the decoder (host-checked)
#define PB_MAX_V 64       // one class per lane

// y . w for one 512-wide row: the lane holds w[4 lane .. 4 lane + 3] in a and w[256 + 4 lane ..] in c; every lane returns the sum
__device__ __forceinline__ float pb_row_dot(const float4* __restrict__ yr, const float4 a, const float4 c, int lane) {
    const float4 y0 = yr[lane], y1 = yr[64 + lane];
    float acc = y0.x * a.x + y0.y * a.y + y0.z * a.z + y0.w * a.w;
    acc += y1.x * c.x + y1.y * c.y + y1.z * c.z + y1.w * c.w;
    return wave_sum(acc);
}

// log-softmax over the wavefront: l = the lane's logit (-inf on the lanes past V), in_v = lane < V.  NaN reads -inf.
__device__ __forceinline__ float pb_log_softmax(float l, bool in_v) {
    const float m = wave_max(l);
    const float lse = logf(wave_sum(in_v ? expf(l - m) : 0.f));
    float lp = (l - m) - lse;
    if (!(lp > -INFINITY)) lp = -INFINITY;      // NaN too
    return lp;
}
