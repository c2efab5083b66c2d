// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): the counter-based generator behind the
// dropout masks (dropout.hip) and the VAE sampler's noise (vae.hip).  One block maps a 128-bit counter and a 64-bit key to four words.
#pragma once

#define PHILOX_M0 0xD2511F53u
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u
#define PHILOX_W1 0xBB67AE85u

struct u32q { unsigned x, y, z, w; };

__host__ __device__ static inline u32q philox4x32_10(u32q c, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)PHILOX_M0 * c.x, p1 = (unsigned long long)PHILOX_M1 * c.z;
        const u32q n = {(unsigned)(p1 >> 32) ^ c.y ^ k0, (unsigned)p1, (unsigned)(p0 >> 32) ^ c.w ^ k1, (unsigned)p0};
        c = n;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return c;
}
