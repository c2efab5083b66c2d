// The noise mapping include/morgana_hip.h documents for mg_vae_sample_f32, as device helpers: what the latent surface samplers
// (sampling.hip) and the mixture-density sampler (mdn.hip) draw from.  Flat element i is word i % 4 of Philox block i / 4 with counter
// words (q low, q high, ctr low, site ^ ctr high) and key (seed low, seed high); ctr is the dropout step counter (dropout.hip).
#pragma once
#include "philox.h"

// the u(w) of vae.hip: odd multiple of 2^-24 inside (0, 1), exact in fp32
__device__ __forceinline__ float smp_uniform(unsigned x) { return (float)((x >> 8) | 1u) * 5.9604644775390625e-8f; }

__device__ __forceinline__ u32q smp_block(int64_t q, unsigned long long ctr, unsigned site, unsigned seed_lo, unsigned seed_hi) {
    return philox4x32_10(u32q{(unsigned)q, (unsigned)((unsigned long long)q >> 32), (unsigned)ctr, site ^ (unsigned)(ctr >> 32)}, seed_lo,
                         seed_hi);
}

__device__ __forceinline__ unsigned smp_word(const u32q& w, int j) { return j == 0 ? w.x : j == 1 ? w.y : j == 2 ? w.z : w.w; }

// One Box-Muller pair from two words: (n0, n1) = sqrt(-2 ln u(a)) (cos, sin)(2 pi u(b)) - vae_box_muller's arithmetic.  A block's words
// (x, y) give elements 4q, 4q + 1 and (z, w) give 4q + 2, 4q + 3: for a caller that wants all four values of a block it has drawn.
__device__ __forceinline__ void smp_normal_pair(unsigned a, unsigned b, float& n0, float& n1) {
    const float r = sqrtf(-2.f * logf(smp_uniform(a)));
    float s, c;
    sincospif(2.f * smp_uniform(b), &s, &c);
    n0 = r * c;
    n1 = r * s;
}

// N(0, 1) value of flat element i: words (x, y) of block i / 4 make elements 4q, 4q + 1 and (z, w) make 4q + 2, 4q + 3 as
// sqrt(-2 ln u(a)) (cos, sin)(2 pi u(b)) - vae_box_muller's arithmetic, one element of the pair.  Never 0: u < 1 and 2 u(b) is an odd
// multiple of 2^-23, never a multiple of 1/2.
__device__ __forceinline__ float smp_normal(int64_t i, unsigned long long ctr, unsigned site, unsigned seed_lo, unsigned seed_hi) {
    const u32q w = smp_block(i >> 2, ctr, site, seed_lo, seed_hi);
    const int j = (int)(i & 3);
    const unsigned a = j < 2 ? w.x : w.z, b = j < 2 ? w.y : w.w;
    const float r = sqrtf(-2.f * logf(smp_uniform(a)));
    float s, c;
    sincospif(2.f * smp_uniform(b), &s, &c);
    return r * ((j & 1) ? s : c);
}
