// K24 - masked sequence mean of a feature loss and its backward: the reduction behind losses.sequence_loss
// (reference: morgana/losses.py:29-46, mask from morgana/utils.py:115-144).
//
//   loss = (1 / (B D)) sum_b ( sum_{t < T, d} x[b,t,d] m[b,t] ) / n_b,   m[b,t] = (t < n_b),   n_b = min(max(seq_len[b], 0), T)
//
// The reference runs a host-built mask, mul, two sums, div and mean, then their autograd mirrors, over whatever feature loss the
// user's loss_fn returned.  Here the forward is one streaming pass over x (4 B T D bytes read) plus a one-workgroup finish, the
// backward one streaming pass that writes the dense gradient (4 B T D bytes written); nothing is saved between the two.
//
// Summation order.  Utterance b is cut into chunks of SEQ_CHUNK consecutive elements of its (t, d) index space e = t D + d; one
// workgroup sums one chunk in float64.  Inside a chunk the element with local index i belongs to COLUMN i % 1024 and the columns
// are summed one element after the other in ascending i; the 1024 column sums meet in a fixed tree, the chunk sums of an utterance
// are added in ascending order and divided by n_b, the utterances meet in a second fixed tree, and the result is rounded to float32
// once.  This order is a function of the logical index alone: it does not depend on strides, on alignment or on which of the two
// kernels ran, so a strided view and its contiguous copy give the same bits.  No atomics, no host read.
//
//   * seq_mean_vec_kernel: rows contiguous (stride_d == 1, stride_t == D).  16-byte loads at 16-byte-ALIGNED addresses whatever the
//     chunk's own alignment: with the chunk starting a floats behind a boundary, lane register j of thread tid holds column
//     (4 tid - a + j) % 1024 - a rotation of the columns over the registers, not another order - and the two vectors that hang over
//     the chunk's ends are read element by element (the scalar head and tail).
//   * seq_mean_strided_kernel: any strides (a column slice, an expanded operand with stride 0), one element per load; thread tid
//     holds columns tid, tid + 256, tid + 512, tid + 768, so that a unit stride_d still coalesces.
//
// Every frame is read and multiplied by its mask value, as the reference does: a NaN or Inf in a pad frame makes the loss NaN, and
// n_b == 0 gives 0 / 0 = NaN.
#include "common.h"
#include "seq_reduce.h"

#define SEQ_THREADS 256
#define SEQ_COLS 1024             // 4 per thread
#define SEQ_CHUNK 8192            // elements of one utterance summed by one workgroup; a multiple of SEQ_COLS

// The 1024 column sums (cols[c], written by whichever thread held column c) -> the chunk's sum, in an order fixed by c alone.
__device__ __forceinline__ double seq_columns_sum(const double* cols, double* red) {
    __syncthreads();
    const int tid = threadIdx.x;
    const double v = (cols[tid] + cols[tid + 256]) + (cols[tid + 512] + cols[tid + 768]);
    return mg_block_sum_f64(v, red);
}

__global__ __launch_bounds__(SEQ_THREADS) void seq_mean_vec_kernel(const float* __restrict__ x, int64_t stride_b,
                                                                   const int64_t* __restrict__ seq_len, int T, int D,
                                                                   double* __restrict__ partial) {
    __shared__ double cols[SEQ_COLS];
    __shared__ double red[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t row_elems = (int64_t)T * D;
    const int64_t lo = (int64_t)blockIdx.x * SEQ_CHUNK;
    const int len = (int)(row_elems - lo < SEQ_CHUNK ? row_elems - lo : SEQ_CHUNK);
    const int64_t valid = mg_valid_frames(seq_len, b, T) * D - lo;      // local indices below it are valid frames
    const float* p = x + (int64_t)b * stride_b + lo;
    const int a = (int)(((uintptr_t)p >> 2) & 3u);                       // floats between the last 16-byte boundary and p
    const int nvec = (len + a + 3) >> 2;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int m = tid; m < nvec; m += SEQ_THREADS) {
        const int i0 = 4 * m - a;                                        // local index of register 0; p + i0 is 16-byte aligned
        if (i0 >= 0 && i0 + 4 <= len) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(p + i0);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += (double)(v[j] * (i0 + j < valid ? 1.f : 0.f));
        } else {                                                         // the vector hangs over an end of the chunk: its inside only
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i0 + j >= 0 && i0 + j < len) acc[j] += (double)(p[i0 + j] * (i0 + j < valid ? 1.f : 0.f));
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) cols[(4 * tid - a + j) & (SEQ_COLS - 1)] = acc[j];
    const double total = seq_columns_sum(cols, red);
    if (tid == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(SEQ_THREADS) void seq_mean_strided_kernel(const float* __restrict__ x, int64_t stride_b, int64_t stride_t,
                                                                       int64_t stride_d, const int64_t* __restrict__ seq_len, int T,
                                                                       int D, double* __restrict__ partial) {
    __shared__ double cols[SEQ_COLS];
    __shared__ double red[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t row_elems = (int64_t)T * D;
    const int64_t lo = (int64_t)blockIdx.x * SEQ_CHUNK;
    const int len = (int)(row_elems - lo < SEQ_CHUNK ? row_elems - lo : SEQ_CHUNK);
    const int64_t n_b = mg_valid_frames(seq_len, b, T);
    const float* p = x + (int64_t)b * stride_b;
    const int dt = SEQ_COLS / D, dd = SEQ_COLS % D;                      // (t, d) of a column moves by this from one element to the next
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = tid + SEQ_THREADS * j;
        int64_t t = (lo + c) / D;
        int d = (int)((lo + c) - t * D);
        double acc = 0.0;
        for (int i = c; i < len; i += SEQ_COLS) {
            acc += (double)(p[t * stride_t + (int64_t)d * stride_d] * (t < n_b ? 1.f : 0.f));
            t += dt;
            d += dd;
            if (d >= D) { d -= D; ++t; }
        }
        cols[c] = acc;
    }
    const double total = seq_columns_sum(cols, red);
    if (tid == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = total;
}

// One workgroup: loss = (float)( (1 / (B D)) sum_b ( sum_chunks partial[b, :] / n_b ) ), everything in float64, fixed order.
__global__ __launch_bounds__(SEQ_THREADS) void seq_mean_finish_kernel(const double* __restrict__ partial,
                                                                      const int64_t* __restrict__ seq_len, int B, int T, int D, int chunks,
                                                                      float* __restrict__ loss) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int b = threadIdx.x; b < B; b += SEQ_THREADS) {
        double s = 0.0;
        for (int c = 0; c < chunks; ++c) s += partial[(size_t)b * chunks + c];
        acc += s / (double)mg_valid_frames(seq_len, b, T);              // 0 / 0 = NaN for an utterance without a valid frame
    }
    const double total = mg_block_sum_f64(acc, red);
    if (threadIdx.x == 0) loss[0] = (float)(total / ((double)B * (double)D));
}

// grid (chunks, B): grad[b, t, :] = (float)(g / (n_b B D)) for t < n_b, 0 for pad frames, NaN everywhere when n_b == 0 (the
// reference's 0 * inf).  The gradient is contiguous; a scalar head brings each chunk to 16-byte stores, a scalar tail ends it.
__global__ __launch_bounds__(SEQ_THREADS) void seq_mean_bwd_kernel(const float* __restrict__ grad_loss, const int64_t* __restrict__ seq_len,
                                                                   int B, int T, int D, float* __restrict__ grad) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t row_elems = (int64_t)T * D;
    const int64_t lo = (int64_t)blockIdx.x * SEQ_CHUNK;
    const int len = (int)(row_elems - lo < SEQ_CHUNK ? row_elems - lo : SEQ_CHUNK);
    const int64_t n_b = mg_valid_frames(seq_len, b, T);
    const int64_t valid = n_b * D - lo;
    const float nan = __builtin_nanf("");
    const float on = n_b > 0 ? (float)((double)grad_loss[0] / ((double)n_b * (double)B * (double)D)) : nan;
    const float off = n_b > 0 ? 0.f : nan;
    float* p = grad + (int64_t)b * row_elems + lo;
    int head = (int)((4u - (unsigned)(((uintptr_t)p >> 2) & 3u)) & 3u);
    if (head > len) head = len;
    const int nvec = (len - head) >> 2;
    const int tail = head + 4 * nvec;
    if (tid < head) p[tid] = tid < valid ? on : off;
    f32x4* pv = reinterpret_cast<f32x4*>(p + head);
#pragma unroll 4
    for (int m = tid; m < nvec; m += SEQ_THREADS) {
        const int i0 = head + 4 * m;
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i0 + j < valid ? on : off;
        pv[m] = v;
    }
    if (tail + tid < len) p[tail + tid] = tail + tid < valid ? on : off;
}

static int64_t seq_chunks(int T, int D) { return mg_ceil_div((int64_t)T * D, SEQ_CHUNK); }

static size_t seq_ws_bytes(int B, int T, int D) {
    if (B <= 0 || T <= 0 || D <= 0) return 0;
    return mg_align_up((size_t)B * (size_t)seq_chunks(T, D) * sizeof(double), 256);
}

extern "C" {

int mg_seq_mean_chunk(void) { return SEQ_CHUNK; }

size_t mg_seq_mean_workspace_bytes(int B, int T, int D) { return seq_ws_bytes(B, T, D); }

int mg_seq_mean_f32(const float* x, int64_t stride_b, int64_t stride_t, int64_t stride_d, const int64_t* seq_len, int B, int T, int D,
                    float* loss, void* workspace, size_t workspace_bytes, void* stream) {
    MG_CHECK_ARG(x && loss, "mg_seq_mean_f32: x and loss must not be NULL");
    MG_CHECK_ARG(B > 0 && T > 0 && D > 0, "mg_seq_mean_f32: bad shape (B=%d T=%d D=%d)", B, T, D);
    MG_CHECK_ARG(B <= 65535, "mg_seq_mean_f32: B=%d exceeds 65535", B);
    MG_CHECK_ARG(stride_b >= 0 && stride_t >= 0 && stride_d >= 0, "mg_seq_mean_f32: negative stride (%lld, %lld, %lld)", (long long)stride_b,
                 (long long)stride_t, (long long)stride_d);
    MG_CHECK_ARG(((uintptr_t)x & 3u) == 0 && ((uintptr_t)loss & 3u) == 0 && ((uintptr_t)workspace & 7u) == 0,
                 "mg_seq_mean_f32: x and loss must be 4-byte and the workspace 8-byte aligned");
    const int64_t chunks = seq_chunks(T, D);
    MG_CHECK_ARG(chunks <= 0x7fffffff, "mg_seq_mean_f32: T * D = %lld is too large", (long long)T * D);
    if (!workspace || workspace_bytes < seq_ws_bytes(B, T, D)) {
        mg_set_error("mg_seq_mean_f32: workspace of %zu bytes needed, got %zu", seq_ws_bytes(B, T, D), workspace ? workspace_bytes : (size_t)0);
        return MG_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    double* partial = (double*)workspace;
    const dim3 grid((unsigned)chunks, (unsigned)B);
    if (stride_d == 1 && stride_t == D)
        hipLaunchKernelGGL(seq_mean_vec_kernel, grid, dim3(SEQ_THREADS), 0, st, x, stride_b, seq_len, T, D, partial);
    else
        hipLaunchKernelGGL(seq_mean_strided_kernel, grid, dim3(SEQ_THREADS), 0, st, x, stride_b, stride_t, stride_d, seq_len, T, D, partial);
    MG_CHECK_LAUNCH("mg_seq_mean_f32/sum");
    hipLaunchKernelGGL(seq_mean_finish_kernel, dim3(1), dim3(SEQ_THREADS), 0, st, partial, seq_len, B, T, D, (int)chunks, loss);
    MG_CHECK_LAUNCH("mg_seq_mean_f32/finish");
    return MG_OK;
}

int mg_seq_mean_bwd_f32(const float* grad_loss, const int64_t* seq_len, int B, int T, int D, float* grad, void* stream) {
    MG_CHECK_ARG(grad_loss && grad, "mg_seq_mean_bwd_f32: grad_loss and grad must not be NULL");
    MG_CHECK_ARG(B > 0 && T > 0 && D > 0, "mg_seq_mean_bwd_f32: bad shape (B=%d T=%d D=%d)", B, T, D);
    MG_CHECK_ARG(B <= 65535, "mg_seq_mean_bwd_f32: B=%d exceeds 65535", B);
    MG_CHECK_ARG(((uintptr_t)grad_loss & 3u) == 0 && ((uintptr_t)grad & 3u) == 0, "mg_seq_mean_bwd_f32: grad_loss and grad must be 4-byte aligned");
    const int64_t chunks = seq_chunks(T, D);
    MG_CHECK_ARG(chunks <= 0x7fffffff, "mg_seq_mean_bwd_f32: T * D = %lld is too large", (long long)T * D);
    hipLaunchKernelGGL(seq_mean_bwd_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(SEQ_THREADS), 0, (hipStream_t)stream, grad_loss, seq_len,
                       B, T, D, grad);
    MG_CHECK_LAUNCH("mg_seq_mean_bwd_f32");
    return MG_OK;
}

}  // extern "C"
