// K19 - seq_len-masked mixture-density negative log likelihood, forward + backward, and what generation feeds to MLPG: the most
// probable component (mdn_select_kernel) or a component DRAWN from the mixture weights (mdn_sample_kernel).  The reference ships no MDN layer (its author trained one with it; Zen & Senior, "Deep mixture density
// networks for acoustic modeling in statistical parametric speech synthesis", ICASSP 2014): the definition is include/morgana_hip.h's.
//
// A frame's row holds K logits a, K*D means mu and K*D log standard deviations s (component-major); the target y has D values.
//     z_kd = (y_d - mu_kd) exp(-s_kd),  q_k = log_softmax(a)_k - sum_d (0.5 z_kd^2 + s_kd) - D log sqrt(2 pi),  l = -logsumexp_k q / D
// Composed of torch ops this is about 15 launches over (B, T, K, D) temporaries and their autograd mirrors; here ONE pass reads each
// frame's row once, writes its whole gradient and leaves one partial per workgroup, and a one-workgroup pass finishes the
// per-utterance normalisation in a fixed order (no float atomics: the same bits on every call).  HBM-bound.  Algorithmic bytes per
// valid frame: 4 W read + 4 W written (gradient) + 4 D (target), W = K (1 + 2 D).
//
// One WAVE per frame row, four waves per workgroup.  The K*D (mean, log-std) pairs are taken in their FLAT order i = k D + d, lane
// l owning i = l + 64 j: every load and every gradient store is a run of consecutive floats whatever K and D are (the three runs of
// a row start at offsets that are in general not multiples of 16 bytes, so all accesses are plain 4-byte ones), and no lane idles
// unless the row is shorter than a wave.  What the flat order does not give is q_k's sum over d; the work mapping of that sum is
// chosen per regime by template parameters:
//
//   K*D <= MDN_REG_MAX (1024): z and exp(-s) stay in registers between the two phases (responsibilities, then gradient), NV = 1..16
//       pairs per lane.  The terms 0.5 z^2 + s go through a wave-private slice of LDS and come back as a SEGMENTED sum:
//         D <= MDN_SMALL_D (16)  lane k adds the D terms of component k one after the other (lf0: D = 3, K up to 64 - a loop over k
//                                with a 64-lane tree per component would run 6 shuffle levels K times with 3 live lanes);
//         D >  MDN_SMALL_D       component after component, lanes stride d and one wave tree finishes it (mcep: D = 180, K = 4 - a
//                                serial sum in one lane would be 180 dependent LDS reads with 4 live lanes).
//       MDN_ROWS_REG (16) frames per workgroup, four per wave.
//   K*D <= MG_MDN_MAX_ROW (16384): no register copy; the sum takes the strided form straight from memory (K <= 64 makes D >= 17
//       here) and the gradient phase reads the row again.  A row is at most 128 KB and was just read: the second read hits the L2,
//       HBM still sees one.  MDN_ROWS_WIDE (4) frames per workgroup, one per wave.
// Pad frames (t >= n_b) read nothing: their gradient row is written as zero, their target is never looked at.
#include <float.h>

#include "common.h"
#include "philox_noise.h"
#include "seq_reduce.h"

#define MDN_REG_MAX 1024        // longest K*D of the register path (16 pairs per lane)
#define MDN_SMALL_D 16          // widest D summed by one lane per component
#define MDN_ROWS_REG 16         // frames per workgroup, register path (4 per wave)
#define MDN_ROWS_WIDE 4         // frames per workgroup, re-read path (1 per wave)
#define MDN_ROWS_SELECT 16      // frames per workgroup, selection and sampling
#define MDN_SAMPLE_ELEMENT_D 64 // widest D whose noise is drawn one element per lane; above, one Philox block (4 elements) per lane
#define MDN_HALF_LOG_2PI 0.9189385332046727f

static inline int mdn_rows_per_wg(int K, int D) { return K * D <= MDN_REG_MAX ? MDN_ROWS_REG : MDN_ROWS_WIDE; }

// LDS traffic of ONE wave is in order: this keeps the compiler from moving it and waits for the reads to have landed
__device__ __forceinline__ void mdn_wave_fence() {
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

struct mdn_args {
    const float* pred;
    const float* target;
    const int64_t* seq_len;
    float* grad;
    float* partial;
    int ldp, ldt, ldg, B, T, K, D;
    unsigned magic;             // floor(2^32 / D) + 1: i / D == __umulhi(i, magic) for every i < MG_MDN_MAX_ROW (D >= 2)
    float floor;
    int has_floor;
    float grad_scale;
};

__device__ __forceinline__ int mdn_component(int i, int D, unsigned magic) { return D == 1 ? i : (int)__umulhi((unsigned)i, magic); }

// max(s, floor) as torch.clamp has it (a NaN stays a NaN); `floored` = the gradient of s is cut
__device__ __forceinline__ float mdn_floor(float s, const mdn_args& a, bool& floored) {
    floored = a.has_floor && s < a.floor;
    return floored ? a.floor : s;
}

// q (one component per lane, -inf past K) -> responsibilities r = exp(q - logsumexp q) in the same lanes, returns -logsumexp q
__device__ __forceinline__ float mdn_responsibilities(float q, float& r) {
    const float qmax = mg_wave_max(q);
    const float e = expf(q - qmax);                       // exp(-inf) = 0: a removed component (and a lane past K) adds nothing
    const float s = mg_wave_sum(e);
    r = e / s;
    return -(qmax + logf(s));
}

// Register path.  grid (ceil(T / MDN_ROWS_REG), B), 256 threads.  partial[b * gridDim.x + chunk] = sum of the chunk's frame losses.
template <int NV, bool SMALL_D>
__global__ __launch_bounds__(256) void masked_mdn_reg_kernel(mdn_args a) {
    __shared__ float term[4][NV * 64];
    __shared__ float resp[4][64];
    __shared__ float red[4];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = a.K, D = a.D, N = K * D;
    const int64_t n_b = mg_valid_frames(a.seq_len, b, a.T);
    const float coef = a.grad_scale / ((float)D * (float)n_b * (float)a.B);
    const float norm = (float)D * MDN_HALF_LOG_2PI;
    const int t0 = blockIdx.x * MDN_ROWS_REG;
    float acc = 0.f;
    for (int r = wave; r < MDN_ROWS_REG; r += 4) {
        const int t = t0 + r;
        if (t >= a.T) break;
        const size_t row = (size_t)b * a.T + t;
        float* g = a.grad ? a.grad + row * a.ldg : nullptr;
        if (t >= n_b) {                                   // pad frame: zeros out, nothing in
            if (g) {
                if (lane < K) g[lane] = 0.f;
#pragma unroll
                for (int j = 0; j < NV; ++j)
                    if (lane + 64 * j < N) g[K + lane + 64 * j] = g[K + N + lane + 64 * j] = 0.f;
            }
            continue;
        }
        const float* x = a.pred + row * a.ldp;
        const float* y = a.target + row * a.ldt;
        float z[NV], es[NV];
        unsigned cut = 0;                                 // bit j: the log-std of pair j sits on the floor
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int i = lane + 64 * j;
            z[j] = es[j] = 0.f;
            if (i < N) {
                const int d = i - mdn_component(i, D, a.magic) * D;
                bool floored;
                const float s = mdn_floor(x[K + N + i], a, floored);
                if (floored) cut |= 1u << j;
                es[j] = expf(-s);
                z[j] = (y[d] - x[K + i]) * es[j];
                term[wave][i] = 0.5f * z[j] * z[j] + s;
            }
        }
        mdn_wave_fence();
        float sum = 0.f;                                  // lane k: sum_d of component k's terms
        if (SMALL_D) {
            if (lane < K)
                for (int d = 0; d < D; ++d) sum += term[wave][lane * D + d];
        } else {
            for (int k = 0; k < K; ++k) {
                float p = 0.f;
                for (int d = lane; d < D; d += 64) p += term[wave][k * D + d];
                p = mg_wave_sum(p);
                if (lane == k) sum = p;
            }
        }
        const float av = lane < K ? x[lane] : -INFINITY;
        const float amax = mg_wave_max(av);
        const float ea = expf(av - amax);                 // all logits -inf: -inf - -inf = NaN, the frame's loss is NaN
        const float sa = mg_wave_sum(ea);
        const float q = lane < K ? (((av - amax) - logf(sa)) - sum) - norm : -INFINITY;
        float rk;
        acc += mdn_responsibilities(q, rk) / (float)D;
        if (g) {
            if (lane < K) g[lane] = coef * (ea / sa - rk);
            resp[wave][lane] = rk;
            mdn_wave_fence();
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int i = lane + 64 * j;
                if (i < N) {
                    const float cr = coef * resp[wave][mdn_component(i, D, a.magic)];
                    g[K + i] = -(cr * z[j]) * es[j];
                    g[K + N + i] = (cut >> j) & 1u ? 0.f : cr * (1.f - z[j] * z[j]);
                }
            }
        }
        mdn_wave_fence();                                 // the next frame overwrites term / resp
    }
    if (lane == 0) red[wave] = acc;                       // acc is wave-uniform
    __syncthreads();
    if (threadIdx.x == 0) a.partial[(size_t)b * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// Re-read path.  grid (ceil(T / MDN_ROWS_WIDE), B), 256 threads, wave w takes frame t0 + w.
__global__ __launch_bounds__(256) void masked_mdn_reread_kernel(mdn_args a) {
    __shared__ float red[4];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = a.K, D = a.D, N = K * D;
    const int64_t n_b = mg_valid_frames(a.seq_len, b, a.T);
    const float coef = a.grad_scale / ((float)D * (float)n_b * (float)a.B);
    const float norm = (float)D * MDN_HALF_LOG_2PI;
    const int t = blockIdx.x * MDN_ROWS_WIDE + wave;
    float acc = 0.f;
    if (t < a.T) {
        const size_t row = (size_t)b * a.T + t;
        float* g = a.grad ? a.grad + row * a.ldg : nullptr;
        if (t >= n_b) {
            if (g) {
                if (lane < K) g[lane] = 0.f;
                for (int i = lane; i < N; i += 64) g[K + i] = g[K + N + i] = 0.f;
            }
        } else {
            const float* x = a.pred + row * a.ldp;
            const float* y = a.target + row * a.ldt;
            float sum = 0.f;
            for (int k = 0; k < K; ++k) {
                float p = 0.f;
                for (int d = lane; d < D; d += 64) {
                    bool floored;
                    const float s = mdn_floor(x[K + N + k * D + d], a, floored);
                    const float zz = (y[d] - x[K + k * D + d]) * expf(-s);
                    p += 0.5f * zz * zz + s;
                }
                p = mg_wave_sum(p);
                if (lane == k) sum = p;
            }
            const float av = lane < K ? x[lane] : -INFINITY;
            const float amax = mg_wave_max(av);
            const float ea = expf(av - amax);
            const float sa = mg_wave_sum(ea);
            const float q = lane < K ? (((av - amax) - logf(sa)) - sum) - norm : -INFINITY;
            float rk;
            acc = mdn_responsibilities(q, rk) / (float)D;
            if (g) {
                if (lane < K) g[lane] = coef * (ea / sa - rk);
                for (int k = 0; k < K; ++k) {
                    const float cr = coef * __shfl(rk, k, 64);
                    for (int d = lane; d < D; d += 64) {
                        bool floored;
                        const float s = mdn_floor(x[K + N + k * D + d], a, floored);
                        const float es = expf(-s);
                        const float zz = (y[d] - x[K + k * D + d]) * es;
                        g[K + k * D + d] = -(cr * zz) * es;
                        g[K + N + k * D + d] = floored ? 0.f : cr * (1.f - zz * zz);
                    }
                }
            }
        }
    }
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) a.partial[(size_t)b * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup: loss = loss_weight * (1/B) sum_b ( sum_chunks partial[b,:] / n_b ) + loss_keep * loss, fixed summation order.
__global__ __launch_bounds__(256) void masked_mdn_finish_kernel(const float* __restrict__ partial, const int64_t* __restrict__ seq_len, int B,
                                                                int T, int chunks, float loss_weight, float loss_keep,
                                                                float* __restrict__ loss) {
    __shared__ float red[256];
    const float sum = mg_utterance_mean_sum(partial, seq_len, B, T, chunks, red);
    if (threadIdx.x == 0) {
        const float l = loss_weight * (sum / (float)B);
        loss[0] = loss_keep != 0.f ? l + loss_keep * loss[0] : l;
    }
}

// Generation: k* = the lowest index among the largest logits, its means copied, its variances exp(2 max(s, floor)).  One wave per
// frame; a valid frame reads K logits and 2 D values.  grid (ceil(T / MDN_ROWS_SELECT), B), 256 threads.
__global__ __launch_bounds__(256) void mdn_select_kernel(const float* __restrict__ pred, int ldp, const int64_t* __restrict__ seq_len, int T,
                                                         int K, int D, float floor, int has_floor, int64_t* __restrict__ component,
                                                         float* __restrict__ mean, float* __restrict__ variance) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_b = mg_valid_frames(seq_len, b, T);
    const int t0 = blockIdx.x * MDN_ROWS_SELECT;
    for (int r = wave; r < MDN_ROWS_SELECT; r += 4) {
        const int t = t0 + r;
        if (t >= T) break;
        const size_t row = (size_t)b * T + t;
        if (t >= n_b) {
            if (lane == 0) component[row] = 0;
            for (int d = lane; d < D; d += 64) {
                mean[row * D + d] = 0.f;
                variance[row * D + d] = 1.f;               // MLPG's precisions stay finite for a reader that ignores seq_len
            }
            continue;
        }
        const float* x = pred + row * ldp;
        float m = lane < K ? x[lane] : -INFINITY;
        int im = lane;                                    // lanes past K hold -inf and a larger index: they lose every merge
        mg_wave_argmax(m, im);
        im = __shfl(im, 0, 64);
        if (im >= K) im = K - 1;
        if (lane == 0) component[row] = im;
        const float* mu = x + K + (size_t)im * D;
        const float* sd = mu + (size_t)K * D;
        for (int d = lane; d < D; d += 64) {
            float s = sd[d];
            if (has_floor && s < floor) s = floor;
            mean[row * D + d] = mu[d];
            variance[row * D + d] = expf(2.f * s);
        }
    }
}

// Generation by SAMPLING: component k with probability softmax(a / temperature)_k, then that component's mean (plus noise_scale
// standard deviations of N(0, 1) noise when NOISE) and variance - mdn_select_kernel's frame mapping, grid and pad rule.  One wave
// per frame, lane k owns logit k:
//   w_k = expf((a_k - max a) inv_temperature)       0 exactly for a -inf logit and for the lanes past K
//   c_k = inclusive prefix sum of w over the lanes  Hillis-Steele, offsets 1, 2, ..., 32: ONE association on every call
//   S   = c_63                                      = c_{K-1}: the lanes past K add exact zeros
//   u   = u(word r % 4 of Philox block r / 4), r = b T + t, under component_site: a frame's draw does not depend on seq_len,
//         the grid or ldp (a pad frame's counter is simply not used)
//   k*  = the lowest k with u S < c_k, by ballot.  A component with w_k = 0 has c_k = c_{k-1} (c_0 = 0 < u S): never the lowest.
//         No such k (u S rounded up to S): the highest k with w_k > 0.  S is NaN (every logit -inf, an inf or a NaN among them):
//         mdn_select_kernel's component, the lowest index among the largest logits.
// Mean, NOISE: fmaf(noise_scale expf(s'), g, mu) with g = the N(0, 1) value of flat element r D + d under noise_site (philox_noise.h:
// the noise mapping of mg_vae_sample_f32); without NOISE an exact copy, no noise word is drawn.
// Where the arithmetic goes: a Philox block is 10 rounds of two 32 x 32 -> 64 multiplies, and every lane that needs one word of it
// pays for all four.  So the wave's four frames draw their uniforms in ONE pass before the loop (lane l: frame l & 3), and with
// NOISE and D > MDN_SAMPLE_ELEMENT_D a lane owns a whole BLOCK of the flat element array - four values, two Box-Muller pairs - and
// writes those of them that lie in its row (blocks straddle rows when D % 4 != 0: the first and the last block of a row are shared
// with its neighbours, which draw them again to the same bits).  Up to MDN_SAMPLE_ELEMENT_D values a row is one pass of one element
// per lane either way, and the block form would only double each lane's dependent chain (measured at D = 3: 46 against 42 us).
template <bool NOISE>
__global__ __launch_bounds__(256) void mdn_sample_kernel(const float* __restrict__ pred, int ldp, const int64_t* __restrict__ seq_len, int T,
                                                         int K, int D, float floor, int has_floor, float inv_temperature, float noise_scale,
                                                         unsigned seed_lo, unsigned seed_hi, unsigned component_site, unsigned noise_site,
                                                         const unsigned long long* __restrict__ counter, int64_t* __restrict__ component,
                                                         float* __restrict__ mean, float* __restrict__ variance) {
    const unsigned long long ctr = counter ? counter[0] : 0ull;
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_b = mg_valid_frames(seq_len, b, T);
    const int t0 = blockIdx.x * MDN_ROWS_SELECT;
    float u_mine;                                         // lane l: the uniform of the wave's frame t0 + wave + 4 (l & 3)
    {
        const size_t row_l = (size_t)b * T + (size_t)(t0 + wave + 4 * (lane & 3));
        u_mine = smp_uniform(smp_word(smp_block((int64_t)(row_l >> 2), ctr, component_site, seed_lo, seed_hi), (int)(row_l & 3)));
    }
    for (int r = wave; r < MDN_ROWS_SELECT; r += 4) {
        const int t = t0 + r;
        if (t >= T) break;
        const size_t row = (size_t)b * T + t;
        if (t >= n_b) {
            if (lane == 0) component[row] = 0;
            for (int d = lane; d < D; d += 64) {
                mean[row * D + d] = 0.f;
                variance[row * D + d] = 1.f;
            }
            continue;
        }
        const float* x = pred + row * ldp;
        const float a = lane < K ? x[lane] : -INFINITY;
        const float amax = mg_wave_max(a);
        const float w = lane < K ? expf((a - amax) * inv_temperature) : 0.f;
        float c = w;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float below = __shfl_up(c, off, 64);
            if (lane >= off) c += below;
        }
        const float total = __shfl(c, 63, 64);
        int im;
        if (total != total) {                             // wave-uniform
            float m = a;
            im = lane;                                    // lanes past K hold -inf and a larger index: they lose every merge
            mg_wave_argmax(m, im);
            im = __shfl(im, 0, 64);
            if (im >= K) im = K - 1;
        } else {
            const float us = __shfl(u_mine, r >> 2, 64) * total;
            const unsigned long long above = __ballot(lane < K && us < c);
            const unsigned long long live = __ballot(w > 0.f);            // never empty: the largest logit has w = 1
            im = above ? __ffsll((long long)above) - 1 : 63 - __clzll((long long)live);
            if (im < 0) im = 0;                           // cannot happen (above); the reads below stay inside the row whatever
            if (im >= K) im = K - 1;
        }
        if (lane == 0) component[row] = im;
        const float* mu = x + K + (size_t)im * D;
        const float* sd = mu + (size_t)K * D;
        if (NOISE && D > MDN_SAMPLE_ELEMENT_D) {
            const int64_t e0 = (int64_t)row * D;          // the row's flat elements are [e0, e0 + D): blocks e0 / 4 .. (e0 + D - 1) / 4
            for (int64_t q = (e0 >> 2) + lane; q <= ((e0 + D - 1) >> 2); q += 64) {
                const u32q words = smp_block(q, ctr, noise_site, seed_lo, seed_hi);
                float g[4];
                smp_normal_pair(words.x, words.y, g[0], g[1]);
                smp_normal_pair(words.z, words.w, g[2], g[3]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t d = 4 * q + j - e0;
                    if (d >= 0 && d < D) {
                        float s = sd[d];
                        if (has_floor && s < floor) s = floor;
                        variance[e0 + d] = expf(2.f * s);
                        mean[e0 + d] = fmaf(noise_scale * expf(s), g[j], mu[d]);
                    }
                }
            }
        } else {                                          // one element per lane: with NOISE a lane's chain is one block and ONE pair
            for (int d = lane; d < D; d += 64) {
                float s = sd[d];
                if (has_floor && s < floor) s = floor;
                variance[row * D + d] = expf(2.f * s);
                if (NOISE)
                    mean[row * D + d] = fmaf(noise_scale * expf(s), smp_normal((int64_t)(row * D + d), ctr, noise_site, seed_lo, seed_hi), mu[d]);
                else
                    mean[row * D + d] = mu[d];
            }
        }
    }
}

static size_t mdn_ws_bytes(int B, int T, int K, int D) {
    if (B <= 0 || T <= 0 || K <= 0 || D <= 0 || K > MG_MDN_MAX_COMPONENTS || (int64_t)K * D > MG_MDN_MAX_ROW) return 256;
    const int64_t chunks = mg_ceil_div(T, mdn_rows_per_wg(K, D));
    return mg_align_up((size_t)B * (size_t)chunks * sizeof(float), 256);
}

extern "C" {

size_t mg_masked_mdn_workspace_bytes(int B, int T, int K, int D) { return mdn_ws_bytes(B, T, K, D); }

int mg_masked_mdn_f32(const float* pred, int ldp, int col0, const float* target, int ldt, const int64_t* seq_len, int B, int T, int K,
                      int D, float min_log_std, int has_floor, float grad_scale, float loss_weight, float loss_keep, float* loss,
                      float* grad, int ldg, int gcol0, void* workspace, size_t workspace_bytes, void* stream) {
    MG_CHECK_ARG(pred && target && loss, "mg_masked_mdn_f32: pred, target and loss must not be NULL");
    MG_CHECK_ARG(B > 0 && T > 0 && K > 0 && D > 0, "mg_masked_mdn_f32: bad shape (B=%d T=%d K=%d D=%d)", B, T, K, D);
    MG_CHECK_ARG(K <= MG_MDN_MAX_COMPONENTS, "mg_masked_mdn_f32: K=%d exceeds the cap of %d components", K, MG_MDN_MAX_COMPONENTS);
    MG_CHECK_ARG((int64_t)K * D <= MG_MDN_MAX_ROW, "mg_masked_mdn_f32: K*D=%lld exceeds the cap of %d means per frame", (long long)K * D,
                 MG_MDN_MAX_ROW);
    MG_CHECK_ARG(B <= 65535, "mg_masked_mdn_f32: B=%d exceeds 65535", B);
    const int W = K * (1 + 2 * D);
    MG_CHECK_ARG(col0 >= 0 && (int64_t)ldp >= (int64_t)col0 + W, "mg_masked_mdn_f32: columns [%d, %d + %d) do not fit the row stride ldp=%d",
                 col0, col0, W, ldp);
    MG_CHECK_ARG(ldt >= D, "mg_masked_mdn_f32: the target's row stride ldt=%d is below D=%d", ldt, D);
    MG_CHECK_ARG(!grad || (gcol0 >= 0 && (int64_t)ldg >= (int64_t)gcol0 + W),
                 "mg_masked_mdn_f32: gradient columns [%d, %d + %d) do not fit the row stride ldg=%d", gcol0, gcol0, W, ldg);
    if (!workspace || workspace_bytes < mdn_ws_bytes(B, T, K, D)) {
        mg_set_error("mg_masked_mdn_f32: workspace of %zu bytes needed, got %zu", mdn_ws_bytes(B, T, K, D), workspace_bytes);
        return MG_EWORKSPACE;
    }
    const int N = K * D;
    const int chunks = (int)mg_ceil_div(T, mdn_rows_per_wg(K, D));
    hipStream_t st = (hipStream_t)stream;
    mdn_args a;
    a.pred = pred + col0;
    a.target = target;
    a.seq_len = seq_len;
    a.grad = grad ? grad + gcol0 : nullptr;
    a.partial = (float*)workspace;
    a.ldp = ldp;
    a.ldt = ldt;
    a.ldg = ldg;
    a.B = B;
    a.T = T;
    a.K = K;
    a.D = D;
    a.magic = D >= 2 ? (unsigned)((1ull << 32) / (unsigned)D) + 1u : 0u;
    a.floor = min_log_std;
    a.has_floor = has_floor != 0;
    a.grad_scale = grad_scale;
    const dim3 grid(chunks, B);
#define LAUNCH_REG(NV_)                                                                                              \
    do {                                                                                                             \
        if (D <= MDN_SMALL_D) hipLaunchKernelGGL((masked_mdn_reg_kernel<NV_, true>), grid, dim3(256), 0, st, a);     \
        else hipLaunchKernelGGL((masked_mdn_reg_kernel<NV_, false>), grid, dim3(256), 0, st, a);                     \
    } while (0)
    if (N <= 64) LAUNCH_REG(1);
    else if (N <= 128) LAUNCH_REG(2);
    else if (N <= 256) LAUNCH_REG(4);
    else if (N <= 512) LAUNCH_REG(8);
    else if (N <= MDN_REG_MAX) LAUNCH_REG(16);
    else hipLaunchKernelGGL(masked_mdn_reread_kernel, grid, dim3(256), 0, st, a);
#undef LAUNCH_REG
    MG_CHECK_LAUNCH("mg_masked_mdn_f32/rows");
    hipLaunchKernelGGL(masked_mdn_finish_kernel, dim3(1), dim3(256), 0, st, a.partial, seq_len, B, T, chunks, loss_weight, loss_keep, loss);
    MG_CHECK_LAUNCH("mg_masked_mdn_f32/finish");
    return MG_OK;
}

int mg_mdn_select_f32(const float* pred, int ldp, int col0, const int64_t* seq_len, int B, int T, int K, int D, float min_log_std,
                      int has_floor, int64_t* component, float* mean, float* variance, void* stream) {
    MG_CHECK_ARG(pred && component && mean && variance, "mg_mdn_select_f32: pred, component, mean and variance must not be NULL");
    MG_CHECK_ARG(B > 0 && T > 0 && K > 0 && D > 0, "mg_mdn_select_f32: bad shape (B=%d T=%d K=%d D=%d)", B, T, K, D);
    MG_CHECK_ARG(K <= MG_MDN_MAX_COMPONENTS, "mg_mdn_select_f32: K=%d exceeds the cap of %d components", K, MG_MDN_MAX_COMPONENTS);
    MG_CHECK_ARG((int64_t)K * D <= MG_MDN_MAX_ROW, "mg_mdn_select_f32: K*D=%lld exceeds the cap of %d means per frame", (long long)K * D,
                 MG_MDN_MAX_ROW);
    MG_CHECK_ARG(B <= 65535, "mg_mdn_select_f32: B=%d exceeds 65535", B);
    const int W = K * (1 + 2 * D);
    MG_CHECK_ARG(col0 >= 0 && (int64_t)ldp >= (int64_t)col0 + W, "mg_mdn_select_f32: columns [%d, %d + %d) do not fit the row stride ldp=%d",
                 col0, col0, W, ldp);
    hipLaunchKernelGGL(mdn_select_kernel, dim3((unsigned)mg_ceil_div(T, MDN_ROWS_SELECT), B), dim3(256), 0, (hipStream_t)stream, pred + col0,
                       ldp, seq_len, T, K, D, min_log_std, has_floor != 0, component, mean, variance);
    MG_CHECK_LAUNCH("mg_mdn_select_f32");
    return MG_OK;
}

int mg_mdn_sample_f32(const float* pred, int ldp, int col0, const int64_t* seq_len, int B, int T, int K, int D, float min_log_std,
                      int has_floor, float inv_temperature, float noise_scale, uint64_t seed, uint32_t component_site, uint32_t noise_site,
                      const uint64_t* counter, int64_t* component, float* mean, float* variance, void* stream) {
    MG_CHECK_ARG(pred && component && mean && variance, "mg_mdn_sample_f32: pred, component, mean and variance must not be NULL");
    MG_CHECK_ARG(B > 0 && T > 0 && K > 0 && D > 0, "mg_mdn_sample_f32: bad shape (B=%d T=%d K=%d D=%d)", B, T, K, D);
    MG_CHECK_ARG(K <= MG_MDN_MAX_COMPONENTS, "mg_mdn_sample_f32: K=%d exceeds the cap of %d components", K, MG_MDN_MAX_COMPONENTS);
    MG_CHECK_ARG((int64_t)K * D <= MG_MDN_MAX_ROW, "mg_mdn_sample_f32: K*D=%lld exceeds the cap of %d means per frame", (long long)K * D,
                 MG_MDN_MAX_ROW);
    MG_CHECK_ARG(B <= 65535, "mg_mdn_sample_f32: B=%d exceeds 65535", B);
    const int W = K * (1 + 2 * D);
    MG_CHECK_ARG(col0 >= 0 && (int64_t)ldp >= (int64_t)col0 + W, "mg_mdn_sample_f32: columns [%d, %d + %d) do not fit the row stride ldp=%d",
                 col0, col0, W, ldp);
    MG_CHECK_ARG(inv_temperature > 0.f && inv_temperature <= FLT_MAX, "mg_mdn_sample_f32: inv_temperature=%g must be finite and positive",
                 (double)inv_temperature);
    MG_CHECK_ARG(noise_scale >= 0.f && noise_scale <= FLT_MAX, "mg_mdn_sample_f32: noise_scale=%g must be finite and not negative",
                 (double)noise_scale);
    MG_CHECK_ARG(component_site != noise_site, "mg_mdn_sample_f32: the component and the noise site are both 0x%x: one stream for two draws",
                 (unsigned)component_site);
    const dim3 grid((unsigned)mg_ceil_div(T, MDN_ROWS_SELECT), B);
    if (noise_scale != 0.f)
        hipLaunchKernelGGL(mdn_sample_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, pred + col0, ldp, seq_len, T, K, D, min_log_std,
                           has_floor != 0, inv_temperature, noise_scale, (unsigned)seed, (unsigned)(seed >> 32), component_site, noise_site,
                           (const unsigned long long*)counter, component, mean, variance);
    else
        hipLaunchKernelGGL(mdn_sample_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, pred + col0, ldp, seq_len, T, K, D, min_log_std,
                           has_floor != 0, inv_temperature, noise_scale, (unsigned)seed, (unsigned)(seed >> 32), component_site, noise_site,
                           (const unsigned long long*)counter, component, mean, variance);
    MG_CHECK_LAUNCH("mg_mdn_sample_f32");
    return MG_OK;
}

}  // extern "C"
