// The pieces a latent-conditioned SPSS model (morgana.base_models.BaseVAE, reference base_models.py:288-381) adds to the step:
//   * the reparameterised sample z = mean + exp(0.5 logvar) eps, eps ~ N(0, 1) by Box-Muller on Philox4x32-10 words (the counter scheme
//     of dropout.hip: a captured graph draws new noise on every replay), and its backward;
//   * the KL divergence against N(0, I) (reference losses.py:64-67) with one deterministic reduction, and its backward;
//   * latent conditioning of the first layer: the gather + concat of upsample.hip with a per-item latent block behind the frame features,
//     a per-item row add (the latent's part of a first layer that runs at phone rate) and a per-item row sum (the gradient of the
//     latent, z being broadcast over every row of its item).
// Every entry point checks its arguments on the host, allocates nothing and never synchronises.  Only vector (global) stores.
#include "common.h"
#include "philox.h"

// (x >> 8) | 1 is odd and below 2^24, so u = that * 2^-24 is exact in fp32 and lies in (0, 1): log(u) is finite, u never reaches 1.
__device__ __forceinline__ float vae_uniform(unsigned x) { return (float)((x >> 8) | 1u) * 5.9604644775390625e-8f; }

// Box-Muller: (a, b) -> sqrt(-2 ln u(a)) * (cos 2pi u(b), sin 2pi u(b))
__device__ __forceinline__ void vae_box_muller(unsigned a, unsigned b, float& n0, float& n1) {
    const float r = sqrtf(-2.f * logf(vae_uniform(a)));
    float s, c;
    sincospif(2.f * vae_uniform(b), &s, &c);
    n0 = r * c;
    n1 = r * s;
}

// one thread per Philox block = 4 consecutive elements of the flattened rows x Z array
__global__ __launch_bounds__(256) void vae_sample_kernel(const float* __restrict__ mean, int ldm, const float* __restrict__ logvar, int ldv,
                                                         int64_t n, int Z, unsigned seed_lo, unsigned seed_hi, unsigned site,
                                                         const unsigned long long* __restrict__ counter, float* __restrict__ z,
                                                         float* __restrict__ eps) {
    const unsigned long long ctr = counter ? counter[0] : 0ull;
    const int64_t blocks4 = (n + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < blocks4; q += (int64_t)gridDim.x * 256) {
        const u32q w = philox4x32_10(u32q{(unsigned)q, (unsigned)((unsigned long long)q >> 32), (unsigned)ctr, site ^ (unsigned)(ctr >> 32)},
                                     seed_lo, seed_hi);
        float e[4];
        vae_box_muller(w.x, w.y, e[0], e[1]);
        vae_box_muller(w.z, w.w, e[2], e[3]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t i = 4 * q + j;
            if (i < n) {
                const int64_t r = i / Z, c = i - r * Z;
                eps[i] = e[j];
                z[i] = mean[r * ldm + c] + expf(0.5f * logvar[r * ldv + c]) * e[j];
            }
        }
    }
}

__global__ __launch_bounds__(256) void vae_sample_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ eps,
                                                             const float* __restrict__ logvar, int ldv, int64_t n, int Z,
                                                             float* __restrict__ dmean, float* __restrict__ dlogvar) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / Z, c = i - r * Z;
        const float g = dz[i];
        if (dmean) dmean[i] = g;
        dlogvar[i] = 0.5f * g * eps[i] * expf(0.5f * logvar[r * ldv + c]);
    }
}

// One workgroup: every thread sums a fixed strided subset in fp64, then a fixed tree in LDS - the same order on every call.
__global__ __launch_bounds__(256) void kld_kernel(const float* __restrict__ mean, int ldm, const float* __restrict__ logvar, int ldv,
                                                  int64_t rows, int Z, float* __restrict__ out) {
    __shared__ double part[256];
    const int64_t n = rows * Z;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const int64_t r = i / Z, c = i - r * Z;
        const float m = mean[r * ldm + c], lv = logvar[r * ldv + c];
        acc += (double)(1.f + lv - m * m - expf(lv));
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)(-0.5 * part[0] / (double)rows);
}

__global__ __launch_bounds__(256) void kld_bwd_kernel(const float* __restrict__ grad, const float* __restrict__ mean, int ldm,
                                                      const float* __restrict__ logvar, int ldv, int64_t rows, int Z,
                                                      float* __restrict__ dmean, float* __restrict__ dlogvar) {
    const float g = grad[0] / (float)rows;
    const int64_t n = rows * Z;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / Z, c = i - r * Z;
        dmean[i] = g * mean[r * ldm + c];
        dlogvar[i] = g * 0.5f * (expf(logvar[r * ldv + c]) - 1.f);
    }
}

// out[m] = [src[rows[m]] (0 for rows[m] < 0) | extra[m] | z[m / rows_per_item] | 0 ...] up to ldo.  One wave per row, as
// gather_concat_kernel (upsample.hip); rows == NULL reads src row m (a frame-rate input that is already materialised).
template <bool OUT_BF16>
__global__ __launch_bounds__(256) void gather_concat_latent_kernel(const float* __restrict__ src, const int32_t* __restrict__ rows,
                                                                   const float* __restrict__ extra, const float* __restrict__ z,
                                                                   void* __restrict__ out_, int64_t M, int F, int C, int Z,
                                                                   int64_t rows_per_item, int ldo) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    const bool vec = (F & 3) == 0;
    for (int64_t m = wave; m < M; m += n_waves) {
        const int64_t r = rows ? (int64_t)rows[m] : m;
        const float* s = src + (size_t)(r < 0 ? 0 : r) * F;
        const float* x = extra ? extra + (size_t)m * C : nullptr;
        const float* zb = z + (size_t)(m / rows_per_item) * Z;
        auto value = [&](int e) -> float {
            if (e < F) return r >= 0 ? s[e] : 0.f;
            if (e < F + C) return x[e - F];
            if (e < F + C + Z) return zb[e - F - C];
            return 0.f;
        };
        if (OUT_BF16) {
            uint16_t* o = (uint16_t*)out_ + (size_t)m * ldo;
            for (int c = lane; c < (ldo >> 3); c += 64) {
                const int k = c << 3;
                float v[8];
                if (r >= 0 && vec && k + 8 <= F) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(s + k);
                    const f32x4 b = *reinterpret_cast<const f32x4*>(s + k + 4);
                    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
                    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = value(k + j);
                }
                bf16x8 p;
#pragma unroll
                for (int j = 0; j < 8; ++j) p[j] = (short)mg_f2bf(v[j]);
                *reinterpret_cast<bf16x8*>(o + k) = p;
            }
        } else {
            float* o = (float*)out_ + (size_t)m * ldo;
            for (int e = lane; e < ldo; e += 64) o[e] = value(e);
        }
    }
}

// P[r, 0:N] += U[r / rows_per_item, 0:N] for r < rows; one thread per element
__global__ __launch_bounds__(256) void rows_add_per_item_kernel(float* __restrict__ P, int ldp, int64_t rows, int N, const float* __restrict__ U,
                                                                int ldu, int64_t rows_per_item) {
    const int64_t n = rows * N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / N, c = i - r * N;
        P[r * ldp + c] += U[(r / rows_per_item) * ldu + c];
    }
}

// s[b, n] = sum over the rows of item b of G[r, n] (times H[r, n] (1 - H[r, n]) when H is given: a sigmoid's gradient factor).
// Workgroup (column chunk of 64, item b): RS_WAVES waves take every RS_WAVES-th row in order (sixteen streams of loads in flight per
// column chunk: the generic path's 64 x 1000 rows are read at a useful rate), their partials are added in a fixed order.
#define RS_WAVES 16
template <bool IN_BF16>
__global__ __launch_bounds__(64 * RS_WAVES) void rows_sum_per_item_kernel(const void* __restrict__ G_, int ldg, const float* __restrict__ H,
                                                                          int ldh, int64_t rows_per_item, int N, float* __restrict__ s, int lds) {
    __shared__ float part[RS_WAVES][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;
    const int64_t b = blockIdx.y;
    float acc = 0.f;
    if (col < N) {
        const int64_t r0 = b * rows_per_item;
#pragma unroll 4
        for (int64_t j = wv; j < rows_per_item; j += RS_WAVES) {
            const int64_t r = r0 + j;
            float g;
            if constexpr (IN_BF16) g = mg_bf2f(((const uint16_t*)G_)[r * ldg + col]);
            else g = ((const float*)G_)[r * ldg + col];
            if (H) {
                const float h = H[r * ldh + col];
                g *= h * (1.f - h);
            }
            acc += g;
        }
    }
    part[wv][lane] = acc;
    __syncthreads();
    if (wv == 0 && col < N) {
        float total = part[0][lane];
#pragma unroll
        for (int w = 1; w < RS_WAVES; ++w) total += part[w][lane];
        s[b * lds + col] = total;
    }
}

static int vae_grid(int64_t n) {
    int64_t blocks = mg_ceil_div(n, 256);
    if (blocks > 8192) blocks = 8192;
    return (int)(blocks < 1 ? 1 : blocks);
}

// one wave per row, four per workgroup
static int wave_rows_grid(int64_t M) {
    int64_t blocks = mg_ceil_div(M, 4);
    if (blocks > 8192) blocks = 8192;
    return (int)(blocks < 1 ? 1 : blocks);
}

extern "C" {

int mg_vae_sample_f32(const float* mean, int ldm, const float* logvar, int ldv, int64_t rows, int Z, uint64_t seed, uint32_t site,
                      const uint64_t* counter, float* z, float* eps, void* stream) {
    MG_CHECK_ARG(mean && logvar && z && eps && rows >= 0 && Z > 0, "mg_vae_sample_f32: bad arguments (rows=%lld Z=%d)", (long long)rows, Z);
    MG_CHECK_ARG(ldm >= Z && ldv >= Z, "mg_vae_sample_f32: ldm=%d and ldv=%d must be >= Z=%d", ldm, ldv, Z);
    const int64_t n = rows * Z;
    if (n == 0) return MG_OK;
    hipLaunchKernelGGL(vae_sample_kernel, dim3(vae_grid(mg_ceil_div(n, 4))), dim3(256), 0, (hipStream_t)stream, mean, ldm, logvar, ldv, n, Z,
                       (unsigned)seed, (unsigned)(seed >> 32), site, (const unsigned long long*)counter, z, eps);
    MG_CHECK_LAUNCH("mg_vae_sample_f32");
    return MG_OK;
}

int mg_vae_sample_bwd_f32(const float* dz, const float* eps, const float* logvar, int ldv, int64_t rows, int Z, float* dmean, float* dlogvar,
                          void* stream) {
    MG_CHECK_ARG(dz && eps && logvar && dlogvar && rows >= 0 && Z > 0, "mg_vae_sample_bwd_f32: bad arguments (rows=%lld Z=%d)", (long long)rows,
                 Z);
    MG_CHECK_ARG(ldv >= Z, "mg_vae_sample_bwd_f32: ldv=%d must be >= Z=%d", ldv, Z);
    const int64_t n = rows * Z;
    if (n == 0) return MG_OK;
    hipLaunchKernelGGL(vae_sample_bwd_kernel, dim3(vae_grid(n)), dim3(256), 0, (hipStream_t)stream, dz, eps, logvar, ldv, n, Z, dmean, dlogvar);
    MG_CHECK_LAUNCH("mg_vae_sample_bwd_f32");
    return MG_OK;
}

int mg_kld_standard_normal_f32(const float* mean, int ldm, const float* logvar, int ldv, int64_t rows, int Z, float* out, void* stream) {
    MG_CHECK_ARG(mean && logvar && out && rows > 0 && Z > 0, "mg_kld_standard_normal_f32: bad arguments (rows=%lld Z=%d)", (long long)rows, Z);
    MG_CHECK_ARG(ldm >= Z && ldv >= Z, "mg_kld_standard_normal_f32: ldm=%d and ldv=%d must be >= Z=%d", ldm, ldv, Z);
    hipLaunchKernelGGL(kld_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, mean, ldm, logvar, ldv, rows, Z, out);
    MG_CHECK_LAUNCH("mg_kld_standard_normal_f32");
    return MG_OK;
}

int mg_kld_standard_normal_bwd_f32(const float* grad, const float* mean, int ldm, const float* logvar, int ldv, int64_t rows, int Z,
                                   float* dmean, float* dlogvar, void* stream) {
    MG_CHECK_ARG(grad && mean && logvar && dmean && dlogvar && rows > 0 && Z > 0,
                 "mg_kld_standard_normal_bwd_f32: bad arguments (rows=%lld Z=%d)", (long long)rows, Z);
    MG_CHECK_ARG(ldm >= Z && ldv >= Z, "mg_kld_standard_normal_bwd_f32: ldm=%d and ldv=%d must be >= Z=%d", ldm, ldv, Z);
    hipLaunchKernelGGL(kld_bwd_kernel, dim3(vae_grid(rows * Z)), dim3(256), 0, (hipStream_t)stream, grad, mean, ldm, logvar, ldv, rows, Z, dmean,
                       dlogvar);
    MG_CHECK_LAUNCH("mg_kld_standard_normal_bwd_f32");
    return MG_OK;
}

static int check_latent_concat(const char* name, const float* src, const float* extra, const float* z, const void* out, int64_t M, int F, int C,
                               int Z, int64_t rows_per_item, int ldo) {
    MG_CHECK_ARG(src && z && out && M >= 0 && F > 0 && C >= 0 && Z > 0, "%s: bad arguments (M=%lld F=%d C=%d Z=%d)", name, (long long)M, F, C, Z);
    MG_CHECK_ARG((C == 0) == (extra == nullptr), "%s: extra must be given exactly when C=%d > 0", name, C);
    MG_CHECK_ARG(rows_per_item > 0, "%s: rows_per_item=%lld must be > 0", name, (long long)rows_per_item);
    MG_CHECK_ARG(ldo >= F + C + Z, "%s: ldo=%d must be >= F+C+Z=%d", name, ldo, F + C + Z);
    return MG_OK;
}

int mg_gather_concat_latent_f32(const float* src, const int32_t* rows, const float* extra, const float* z, float* out, int64_t M, int F, int C,
                                int Z, int64_t rows_per_item, int ldo, void* stream) {
    const int rc = check_latent_concat("mg_gather_concat_latent_f32", src, extra, z, out, M, F, C, Z, rows_per_item, ldo);
    if (rc != MG_OK) return rc;
    if (M == 0) return MG_OK;
    hipLaunchKernelGGL(gather_concat_latent_kernel<false>, dim3(wave_rows_grid(M)), dim3(256), 0, (hipStream_t)stream, src, rows,
                       extra, z, (void*)out, M, F, C, Z, rows_per_item, ldo);
    MG_CHECK_LAUNCH("mg_gather_concat_latent_f32");
    return MG_OK;
}

int mg_gather_concat_latent_bf16(const float* src, const int32_t* rows, const float* extra, const float* z, uint16_t* out, int64_t M, int F,
                                 int C, int Z, int64_t rows_per_item, int ldo, void* stream) {
    const int rc = check_latent_concat("mg_gather_concat_latent_bf16", src, extra, z, out, M, F, C, Z, rows_per_item, ldo);
    if (rc != MG_OK) return rc;
    MG_CHECK_ARG(ldo % 8 == 0, "mg_gather_concat_latent_bf16: ldo=%d must be a multiple of 8", ldo);
    MG_CHECK_ARG(((uintptr_t)out % 16 == 0) && ((uintptr_t)src % 16 == 0), "mg_gather_concat_latent_bf16: buffers must be 16-byte aligned");
    if (M == 0) return MG_OK;
    hipLaunchKernelGGL(gather_concat_latent_kernel<true>, dim3(wave_rows_grid(M)), dim3(256), 0, (hipStream_t)stream, src, rows,
                       extra, z, (void*)out, M, F, C, Z, rows_per_item, ldo);
    MG_CHECK_LAUNCH("mg_gather_concat_latent_bf16");
    return MG_OK;
}

int mg_rows_add_per_item_f32(float* P, int ldp, int64_t rows, int N, const float* U, int ldu, int64_t rows_per_item, void* stream) {
    MG_CHECK_ARG(P && U && rows >= 0 && N > 0 && rows_per_item > 0, "mg_rows_add_per_item_f32: bad arguments (rows=%lld N=%d rows_per_item=%lld)",
                 (long long)rows, N, (long long)rows_per_item);
    MG_CHECK_ARG(ldp >= N && ldu >= N, "mg_rows_add_per_item_f32: ldp=%d and ldu=%d must be >= N=%d", ldp, ldu, N);
    if (rows == 0) return MG_OK;
    hipLaunchKernelGGL(rows_add_per_item_kernel, dim3(vae_grid(rows * N)), dim3(256), 0, (hipStream_t)stream, P, ldp, rows, N, U, ldu,
                       rows_per_item);
    MG_CHECK_LAUNCH("mg_rows_add_per_item_f32");
    return MG_OK;
}

int mg_rows_sum_per_item(const void* G, int ldg, int bf16, const float* H, int ldh, int64_t B, int64_t rows_per_item, int N, float* s, int lds,
                         void* stream) {
    MG_CHECK_ARG(G && s && B >= 0 && rows_per_item >= 0 && N > 0, "mg_rows_sum_per_item: bad arguments (B=%lld rows_per_item=%lld N=%d)",
                 (long long)B, (long long)rows_per_item, N);
    MG_CHECK_ARG(ldg >= N && lds >= N && (!H || ldh >= N), "mg_rows_sum_per_item: ldg=%d, lds=%d and ldh=%d must be >= N=%d", ldg, lds, ldh, N);
    MG_CHECK_ARG(B <= 65535, "mg_rows_sum_per_item: B=%lld items exceed 65535", (long long)B);
    if (B == 0) return MG_OK;
    const dim3 grid((unsigned)mg_ceil_div(N, 64), (unsigned)B);
    if (bf16)
        hipLaunchKernelGGL(rows_sum_per_item_kernel<true>, grid, dim3(64 * RS_WAVES), 0, (hipStream_t)stream, G, ldg, H, ldh, rows_per_item, N, s, lds);
    else
        hipLaunchKernelGGL(rows_sum_per_item_kernel<false>, grid, dim3(64 * RS_WAVES), 0, (hipStream_t)stream, G, ldg, H, ldh, rows_per_item, N, s, lds);
    MG_CHECK_LAUNCH("mg_rows_sum_per_item");
    return MG_OK;
}

}  // extern "C"
