// What the decode step tails share (decode_step.hip, beam_step.hip, pair_beam.hip, lexicon.hip): the output head as they
// evaluate it - a bias-free Linear(512, V <= 64) in plain fp32 FMA, one wavefront per (class, row) dot product - the
// log-softmax of a row with one class per lane, the wave arg-best, and the next step's input row.  Every tail includes this,
// so a greedy token, a beam total and a rescored total come from the same numbers.
#pragma once
#include "sbl_common.h"

#define DH_D 512               // d_model of the decoder (host-checked)
#define DH_MAX_V 64            // one class per lane
#define DH_MAX_W 16            // beam slots per clip
#define DH_NONE 0x7fffffff     // index of a lane that has nothing to offer

// y . w for one 512-wide row: the lane holds w[4 lane .. 4 lane + 3] in a and w[256 + 4 lane ..] in c; every lane returns the sum
__device__ __forceinline__ float dh_row_dot(const float4* __restrict__ yr, const float4 a, const float4 c, int lane) {
    const float4 y0 = yr[lane], y1 = yr[64 + lane];
    float acc = y0.x * a.x + y0.y * a.y + y0.z * a.z + y0.w * a.w;
    acc += y1.x * c.x + y1.y * c.y + y1.z * c.z + y1.w * c.w;
    return wave_sum(acc);
}

// log-softmax over the wavefront: l = the lane's logit (-inf on the lanes past V), in_v = lane < V.  NaN reads -inf.
__device__ __forceinline__ float dh_log_softmax(float l, bool in_v) {
    const float m = wave_max(l);
    const float lse = logf(wave_sum(in_v ? expf(l - m) : 0.f));
    float lp = (l - m) - lse;
    if (!(lp > -INFINITY)) lp = -INFINITY;      // NaN too
    return lp;
}

// (value, index) maximum over the wave with the lower index on equal values; DH_NONE = nothing to offer.  Every lane ends
// with the same pair.
__device__ __forceinline__ void dh_wave_best(float& best, int& bi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oi != DH_NONE && (bi == DH_NONE || ov > best || (ov == best && oi < bi))) {
            best = ov;
            bi = oi;
        }
    }
}

// the next step's input row x = emb[tok] * scale + pe[pos], by a workgroup of 256 threads
__device__ __forceinline__ void dh_next_row(float* __restrict__ x, const float* __restrict__ emb, long tok,
                                            const float* __restrict__ pe, int pos, float scale) {
    const float* er = emb + tok * DH_D;
    const float* pr = pe + (long)pos * DH_D;
    for (int d = threadIdx.x; d < DH_D; d += 256) x[d] = er[d] * scale + pr[d];
}
