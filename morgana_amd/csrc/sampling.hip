// Latent surface samplers (morgana.sampling, reference sampling.py): points at a fixed distance from the prior's centre, the latents a
// latent-conditioned model's predict() is fed for controlled, varied renditions of one utterance.
//   * sphere:    out = centre + radius g / |g|, g ~ N(0, 1) by Box-Muller on Philox4x32-10 words - the noise mapping of vae.hip, word
//     for word (flat element i = r D + c, block i / 4: blocks straddle rows when D % 4 != 0) - and its backward;
//   * ellipsoid: D - 1 uniform angles per row, x_n = radii_n prod_{j < n} sin(angle_j) cos(angle_n) (the reference's arithmetic,
//     sampling.py:103-113; its `centre` is NOT added), the in-row product as a wave scan, and its backward.
// The counter scheme is dropout.hip's: a captured graph draws new noise on every replay.  One wave per row; every reduction and the
// scan run in one fixed order (no atomics): the same bits on every call.  Every entry point checks its arguments on the host,
// allocates nothing and never synchronises.  Only vector (global) stores.
#include "common.h"
#include "philox_noise.h"                                 // smp_uniform / smp_block / smp_word / smp_normal: shared with mdn.hip

// Rows of up to SPH_REG * 64 values stay in registers between the norm and the scaling; longer rows loop over chunks of 64 with a
// carried per-lane partial sum and draw their noise a second time (the same function of the same words: the same bits).
#define SPH_REG 4

template <bool REG>
__global__ __launch_bounds__(256) void sphere_sample_kernel(const float* __restrict__ centre, const float* __restrict__ radius, int64_t rows,
                                                            int D, unsigned seed_lo, unsigned seed_hi, unsigned site,
                                                            const unsigned long long* __restrict__ counter, float* __restrict__ out,
                                                            float* __restrict__ unit) {
    const unsigned long long ctr = counter ? counter[0] : 0ull;
    const float rad = radius[0];
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    for (int64_t r = wave; r < rows; r += n_waves) {
        const int64_t base = r * D;
        float g[SPH_REG];
        float ss = 0.f;
        if (REG) {
#pragma unroll
            for (int k = 0; k < SPH_REG; ++k) {
                const int c = lane + 64 * k;
                g[k] = c < D ? smp_normal(base + c, ctr, site, seed_lo, seed_hi) : 0.f;
                ss += g[k] * g[k];
            }
        } else {
            for (int c = lane; c < D; c += 64) {
                const float v = smp_normal(base + c, ctr, site, seed_lo, seed_hi);
                ss += v * v;
            }
        }
        // xor butterfly: every lane ends with the same sum, added in the same order on every call
        const float norm = sqrtf(mg_wave_sum(ss));
        // a division, not a product with 1 / norm: g / |g| is exactly +-1 for D = 1
        if (REG) {
#pragma unroll
            for (int k = 0; k < SPH_REG; ++k) {
                const int c = lane + 64 * k;
                if (c < D) {
                    const float u = g[k] / norm;
                    unit[base + c] = u;
                    out[base + c] = centre[c] + rad * u;
                }
            }
        } else {
            for (int c = lane; c < D; c += 64) {
                const float u = smp_normal(base + c, ctr, site, seed_lo, seed_hi) / norm;
                unit[base + c] = u;
                out[base + c] = centre[c] + rad * u;
            }
        }
    }
}

// The D - 1 angles of row r: element i = r (D - 1) + c uses word i % 4 of block i / 4; column 0 is phi = 2 pi u, the others theta = pi u.
// In units of pi (sincospif: no rounded multiple of pi is ever formed): 2 u or u.
__device__ __forceinline__ float smp_angle_over_pi(int64_t i, int c, unsigned long long ctr, unsigned site, unsigned seed_lo, unsigned seed_hi) {
    const u32q w = smp_block(i >> 2, ctr, site, seed_lo, seed_hi);
    const float u = smp_uniform(smp_word(w, (int)(i & 3)));
    return c == 0 ? 2.f * u : u;
}

__global__ __launch_bounds__(256) void ellipsoid_angles_kernel(int64_t n, int A, unsigned seed_lo, unsigned seed_hi, unsigned site,
                                                               const unsigned long long* __restrict__ counter, float* __restrict__ angles) {
    const unsigned long long ctr = counter ? counter[0] : 0ull;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        angles[i] = 3.14159265358979323846f * smp_angle_over_pi(i, (int)(i % A), ctr, site, seed_lo, seed_hi);
}

// One wave per row, 64 columns a chunk: lane l of chunk k owns column n = 64 k + l, its sine enters an inclusive product scan over the
// lanes (Hillis-Steele, offsets 1, 2, ..., 32: one fixed association), `carry` is the product of every earlier chunk.  Column n needs
// the EXCLUSIVE product (sines of columns < n): the scan value of the lane below, the carry for lane 0.
__global__ __launch_bounds__(256) void ellipsoid_sample_kernel(const float* __restrict__ radii, int64_t rows, int D, unsigned seed_lo,
                                                               unsigned seed_hi, unsigned site,
                                                               const unsigned long long* __restrict__ counter, float* __restrict__ out,
                                                               float* __restrict__ factor) {
    const unsigned long long ctr = counter ? counter[0] : 0ull;
    const int lane = threadIdx.x & 63;
    const int A = D - 1;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    for (int64_t r = wave; r < rows; r += n_waves) {
        float carry = 1.f;
        for (int n0 = 0; n0 < D; n0 += 64) {                       // wave-uniform trip count: every lane reaches the shuffles
            const int n = n0 + lane;
            float s = 1.f, c = 1.f;                                // column D - 1 has no angle: cos_padded = 1; columns past it: unused
            if (n < A) sincospif(smp_angle_over_pi(r * A + n, n, ctr, site, seed_lo, seed_hi), &s, &c);
            float p = s;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const float below = __shfl_up(p, off, 64);
                if (lane >= off) p *= below;
            }
            p *= carry;
            float excl = __shfl_up(p, 1, 64);
            if (lane == 0) excl = carry;
            carry = __shfl(p, 63, 64);
            if (n < D) {
                const float f = excl * c;
                factor[r * D + n] = f;
                out[r * D + n] = radii[n] * f;
            }
        }
    }
}

// out[c] = sum over rows of a[r, c] (b[r, c]) for the 64 columns of workgroup blockIdx.x.  Narrow rows (D <= 32) put 64 / W rows side
// by side in a wave, W = D rounded up to a power of two.  SUM_WAVES waves take every SUM_WAVES-th group of rows in order, fp64
// partials; one thread per column then adds the partials in a fixed order.
#define SUM_WAVES 16
__global__ __launch_bounds__(64 * SUM_WAVES) void column_sum_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t rows,
                                                                    int D, int W, float* __restrict__ out) {
    __shared__ double part[SUM_WAVES][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int side = 64 / W;                                       // rows side by side in one wave (1 when D > 32)
    const int col = blockIdx.x * 64 + (lane % W), sub = lane / W;
    double acc = 0.0;
    if (col < D) {
#pragma unroll 4
        for (int64_t r = (int64_t)wv * side + sub; r < rows; r += (int64_t)SUM_WAVES * side) {
            const double v = (double)a[r * D + col];
            acc += b ? v * (double)b[r * D + col] : v;
        }
    }
    part[wv][lane] = acc;
    __syncthreads();
    if (wv == 0 && sub == 0 && col < D) {
        double total = 0.0;
        for (int w = 0; w < SUM_WAVES; ++w)
            for (int s = 0; s < side; ++s) total += part[w][s * W + lane];
        out[col] = (float)total;
    }
}

// out[0] = sum over all n elements of a[i] b[i]: one workgroup, fixed strided subsets in fp64, then a fixed tree in LDS (kld_kernel's shape).
__global__ __launch_bounds__(1024) void dot_total_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                                         float* __restrict__ out) {
    __shared__ double part[1024];
    double acc = 0.0;
#pragma unroll 4
    for (int64_t i = threadIdx.x; i < n; i += 1024) acc += (double)a[i] * (double)b[i];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)part[0];
}

// one wave per row, four per workgroup
static int smp_rows_grid(int64_t rows) {
    int64_t blocks = mg_ceil_div(rows, 4);
    if (blocks > 8192) blocks = 8192;
    return (int)(blocks < 1 ? 1 : blocks);
}

static void launch_column_sum(const float* a, const float* b, int64_t rows, int D, float* out, hipStream_t stream) {
    int W = 64;
    if (D <= 32)
        for (W = 1; W < D; W <<= 1) {}
    hipLaunchKernelGGL(column_sum_kernel, dim3((unsigned)mg_ceil_div(D, 64)), dim3(64 * SUM_WAVES), 0, stream, a, b, rows, D, W, out);
}

extern "C" {

int mg_sphere_sample_f32(const float* centre, const float* radius, int64_t rows, int D, uint64_t seed, uint32_t site, const uint64_t* counter,
                         float* out, float* unit, void* stream) {
    MG_CHECK_ARG(centre && radius && out && unit && rows >= 0 && D >= 1, "mg_sphere_sample_f32: bad arguments (rows=%lld D=%d)", (long long)rows,
                 D);
    if (rows == 0) return MG_OK;
    if (D <= SPH_REG * 64)
        hipLaunchKernelGGL(sphere_sample_kernel<true>, dim3(smp_rows_grid(rows)), dim3(256), 0, (hipStream_t)stream, centre, radius, rows, D,
                           (unsigned)seed, (unsigned)(seed >> 32), site, (const unsigned long long*)counter, out, unit);
    else
        hipLaunchKernelGGL(sphere_sample_kernel<false>, dim3(smp_rows_grid(rows)), dim3(256), 0, (hipStream_t)stream, centre, radius, rows, D,
                           (unsigned)seed, (unsigned)(seed >> 32), site, (const unsigned long long*)counter, out, unit);
    MG_CHECK_LAUNCH("mg_sphere_sample_f32");
    return MG_OK;
}

int mg_sphere_sample_bwd_f32(const float* dout, const float* unit, int64_t rows, int D, float* dcentre, float* dradius, void* stream) {
    MG_CHECK_ARG(dout && unit && dcentre && dradius && rows >= 0 && D >= 1, "mg_sphere_sample_bwd_f32: bad arguments (rows=%lld D=%d)",
                 (long long)rows, D);
    launch_column_sum(dout, nullptr, rows, D, dcentre, (hipStream_t)stream);                 // rows == 0: the sums are 0 and are written
    MG_CHECK_LAUNCH("mg_sphere_sample_bwd_f32");
    hipLaunchKernelGGL(dot_total_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, dout, unit, rows * D, dradius);
    MG_CHECK_LAUNCH("mg_sphere_sample_bwd_f32");
    return MG_OK;
}

int mg_ellipsoid_angles_f32(int64_t rows, int D, uint64_t seed, uint32_t site, const uint64_t* counter, float* angles, void* stream) {
    MG_CHECK_ARG(angles && rows >= 0, "mg_ellipsoid_angles_f32: bad arguments (rows=%lld D=%d)", (long long)rows, D);
    MG_CHECK_ARG(D >= 2, "mg_ellipsoid_angles_f32: D=%d must be >= 2 (D - 1 angles per row)", D);
    const int64_t n = rows * (D - 1);
    if (n == 0) return MG_OK;
    int64_t blocks = mg_ceil_div(n, 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(ellipsoid_angles_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, n, D - 1, (unsigned)seed,
                       (unsigned)(seed >> 32), site, (const unsigned long long*)counter, angles);
    MG_CHECK_LAUNCH("mg_ellipsoid_angles_f32");
    return MG_OK;
}

int mg_ellipsoid_sample_f32(const float* radii, int64_t rows, int D, uint64_t seed, uint32_t site, const uint64_t* counter, float* out,
                            float* factor, void* stream) {
    MG_CHECK_ARG(radii && out && factor && rows >= 0, "mg_ellipsoid_sample_f32: bad arguments (rows=%lld D=%d)", (long long)rows, D);
    MG_CHECK_ARG(D >= 2, "mg_ellipsoid_sample_f32: D=%d must be >= 2 (D - 1 angles per row)", D);
    if (rows == 0) return MG_OK;
    hipLaunchKernelGGL(ellipsoid_sample_kernel, dim3(smp_rows_grid(rows)), dim3(256), 0, (hipStream_t)stream, radii, rows, D, (unsigned)seed,
                       (unsigned)(seed >> 32), site, (const unsigned long long*)counter, out, factor);
    MG_CHECK_LAUNCH("mg_ellipsoid_sample_f32");
    return MG_OK;
}

int mg_ellipsoid_sample_bwd_f32(const float* dout, const float* factor, int64_t rows, int D, float* dradii, void* stream) {
    MG_CHECK_ARG(dout && factor && dradii && rows >= 0, "mg_ellipsoid_sample_bwd_f32: bad arguments (rows=%lld D=%d)", (long long)rows, D);
    MG_CHECK_ARG(D >= 2, "mg_ellipsoid_sample_bwd_f32: D=%d must be >= 2", D);
    launch_column_sum(dout, factor, rows, D, dradii, (hipStream_t)stream);
    MG_CHECK_LAUNCH("mg_ellipsoid_sample_bwd_f32");
    return MG_OK;
}

}  // extern "C"
