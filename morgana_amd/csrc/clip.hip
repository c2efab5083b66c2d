// K21 - global gradient-norm clipping over the optimiser's flat fp32 gradient buffers
// (torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2, error_if_nonfinite=False) on the finished mean gradient).
//
// torch runs a norm per parameter, a stack, a norm of norms, a clamp and a foreach multiply over a dozen views; here the norm is one
// streaming pass per buffer and the scaling a second one, and the host never reads the norm (capturable into a HIP graph):
//
//   1. mg_grad_sumsq_f32: every workgroup sums the squares of ONE contiguous chunk of the buffer in float64 (the square of an fp32
//      value is exact there, nothing overflows, the sum is good to a few 2^-53 n) and writes one double.  No atomics: a thread takes
//      fixed elements in a fixed order, the workgroup's 256 sums meet in a fixed tree - the same bits on every call.
//   2. mg_grad_clip_scale_f32: every workgroup re-reduces ALL partials (of all buffers: one norm over all parameter groups) in the
//      same fixed order - so all of them hold the same scalar without a second hand-off -, forms norm = sqrt(sum) * inv_world and
//      coef = min(1, max_norm / (norm + 1e-6)) in float64, rounds both to fp32 and multiplies its chunk by coef in place.  coef == 1
//      exactly: nothing is written (g * 1 == g for every g, NaN included).  A NaN norm gives a NaN coef (!= 1: written, as torch
//      does), an infinite one gives 0.
//
// Both are HBM-bound streaming kernels.  Bytes: n * 4 read by (1); n * 4 read + n * 4 written by (2) when the clip bites, about
// (groups * 8 KB of partials, from L2) per workgroup when it does not.  The grid comes from n alone (clip_chunk): at most
// MG_CLIP_MAX_BLOCKS workgroups of 256 threads, chunks a multiple of 1024 floats, so that every chunk starts at the buffer's own
// misalignment and one scalar head of at most 3 elements brings each to 16-byte loads.
#include "common.h"
#include "seq_reduce.h"

#define CLIP_THREADS 256
#define CLIP_MIN_CHUNK 4096       // floats: 4 x 16 bytes per thread
#define CLIP_CHUNK_ROUND 1024     // floats: chunks keep the buffer's 16-byte phase

static inline int64_t clip_chunk(int64_t n) {
    const int64_t even = mg_ceil_div(mg_ceil_div(n, MG_CLIP_MAX_BLOCKS), CLIP_CHUNK_ROUND) * CLIP_CHUNK_ROUND;
    return even > CLIP_MIN_CHUNK ? even : CLIP_MIN_CHUNK;
}
static inline int clip_blocks(int64_t n) { return (int)mg_ceil_div(n, clip_chunk(n)); }

// [begin, end) of this workgroup's chunk, split into a scalar head up to the first 16-byte boundary, float4s and a scalar tail.
struct clip_span {
    int64_t begin, head, nvec, tail_begin, end;
};
__device__ __forceinline__ clip_span clip_span_of(const float* g, int64_t n, int64_t chunk) {
    clip_span s;
    s.begin = (int64_t)blockIdx.x * chunk;
    s.end = s.begin + chunk < n ? s.begin + chunk : n;
    const int64_t len = s.end - s.begin;
    int64_t head = (int64_t)((16u - (unsigned)((uintptr_t)(g + s.begin) & 15u)) & 15u) >> 2;
    s.head = head < len ? head : len;
    s.nvec = (len - s.head) >> 2;
    s.tail_begin = s.begin + s.head + 4 * s.nvec;
    return s;
}

__global__ __launch_bounds__(CLIP_THREADS) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n, int64_t chunk,
                                                                  double* __restrict__ partial) {
    __shared__ double red[4];
    const clip_span s = clip_span_of(g, n, chunk);
    const int tid = threadIdx.x;
    double acc = 0.0;
    if (tid < s.head) {
        const double x = (double)g[s.begin + tid];
        acc = x * x;
    }
    const f32x4* gv = (const f32x4*)(g + s.begin + s.head);
#pragma unroll 4
    for (int64_t i = tid; i < s.nvec; i += CLIP_THREADS) {
        const f32x4 v = gv[i];
        const double x0 = (double)v[0], x1 = (double)v[1], x2 = (double)v[2], x3 = (double)v[3];
        acc += (x0 * x0 + x1 * x1) + (x2 * x2 + x3 * x3);
    }
    if (s.tail_begin + tid < s.end) {
        const double x = (double)g[s.tail_begin + tid];
        acc += x * x;
    }
    const double total = mg_block_sum_f64(acc, red);
    if (tid == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(CLIP_THREADS) void grad_clip_scale_kernel(float* __restrict__ g, int64_t n, int64_t chunk,
                                                                       const double* __restrict__ partial, int n_partial, double inv_world,
                                                                       double max_norm, float* __restrict__ out) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < n_partial; i += CLIP_THREADS) acc += partial[i];
    const double norm = sqrt(mg_block_sum_f64(acc, red)) * inv_world;
    const double ratio = max_norm / (norm + 1e-6);
    const double clamped = ratio > 1.0 ? 1.0 : ratio;              // a NaN ratio stays NaN (torch.clamp(max=1.0))
    const float coef = (float)clamped;
    if (out && blockIdx.x == 0 && tid == 0) {
        out[0] = (float)norm;
        out[1] = coef;
    }
    if (coef == 1.0f) return;                                      // workgroup-uniform
    const clip_span s = clip_span_of(g, n, chunk);
    if (tid < s.head) g[s.begin + tid] *= coef;
    f32x4* gv = (f32x4*)(g + s.begin + s.head);
#pragma unroll 4
    for (int64_t i = tid; i < s.nvec; i += CLIP_THREADS) {
        f32x4 v = gv[i];
        v[0] *= coef;
        v[1] *= coef;
        v[2] *= coef;
        v[3] *= coef;
        gv[i] = v;
    }
    if (s.tail_begin + tid < s.end) g[s.tail_begin + tid] *= coef;
}

extern "C" {

int64_t mg_grad_clip_chunk(int64_t n) { return n > 0 ? clip_chunk(n) : 0; }

int mg_grad_clip_blocks(int64_t n) { return n > 0 ? clip_blocks(n) : 0; }

int mg_grad_sumsq_f32(const float* grad, int64_t n, double* partials, int offset, int n_partials, void* stream) {
    MG_CHECK_ARG(grad && partials, "mg_grad_sumsq_f32: grad and partials must not be NULL");
    MG_CHECK_ARG(n > 0, "mg_grad_sumsq_f32: n=%lld must be positive", (long long)n);
    MG_CHECK_ARG(((uintptr_t)grad & 3u) == 0 && ((uintptr_t)partials & 7u) == 0, "mg_grad_sumsq_f32: grad must be 4-byte and partials 8-byte aligned");
    MG_CHECK_ARG(n_partials > 0 && n_partials <= MG_CLIP_MAX_PARTIALS, "mg_grad_sumsq_f32: n_partials=%d must be in [1, %d]", n_partials,
                 MG_CLIP_MAX_PARTIALS);
    const int blocks = clip_blocks(n);
    MG_CHECK_ARG(offset >= 0 && (int64_t)offset + blocks <= n_partials,
                 "mg_grad_sumsq_f32: partials [%d, %d + %d) do not fit the array of %d", offset, offset, blocks, n_partials);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(CLIP_THREADS), 0, (hipStream_t)stream, grad, n, clip_chunk(n), partials + offset);
    MG_CHECK_LAUNCH("mg_grad_sumsq_f32");
    return MG_OK;
}

int mg_grad_clip_scale_f32(float* grad, int64_t n, const double* partials, int n_partials, double inv_world, double max_norm, float* out,
                           void* stream) {
    MG_CHECK_ARG(grad && partials, "mg_grad_clip_scale_f32: grad and partials must not be NULL");
    MG_CHECK_ARG(n > 0, "mg_grad_clip_scale_f32: n=%lld must be positive", (long long)n);
    MG_CHECK_ARG(((uintptr_t)grad & 3u) == 0 && ((uintptr_t)partials & 7u) == 0 && ((uintptr_t)out & 3u) == 0,
                 "mg_grad_clip_scale_f32: grad and out must be 4-byte and partials 8-byte aligned");
    MG_CHECK_ARG(n_partials > 0 && n_partials <= MG_CLIP_MAX_PARTIALS, "mg_grad_clip_scale_f32: n_partials=%d must be in [1, %d]", n_partials,
                 MG_CLIP_MAX_PARTIALS);
    MG_CHECK_ARG(max_norm > 0.0, "mg_grad_clip_scale_f32: max_norm=%g must be positive", max_norm);
    MG_CHECK_ARG(inv_world > 0.0 && inv_world <= 1.0, "mg_grad_clip_scale_f32: inv_world=%g must be in (0, 1]", inv_world);
    hipLaunchKernelGGL(grad_clip_scale_kernel, dim3(clip_blocks(n)), dim3(CLIP_THREADS), 0, (hipStream_t)stream, grad, n, clip_chunk(n), partials,
                       n_partials, inv_world, max_norm, out);
    MG_CHECK_LAUNCH("mg_grad_clip_scale_f32");
    return MG_OK;
}

}  // extern "C"
