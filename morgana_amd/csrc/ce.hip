// K18 - seq_len-masked categorical cross entropy, forward + backward (reference: morgana/losses.py:29-46 wrapping :59-61 -
// F.cross_entropy(predictions.transpose(1, 2), targets, reduction='none'), the mask of morgana/utils.py:115-144).
//
// The reference runs a transpose, log_softmax, nll_loss, a host-built mask, mul, two sums, a div and a mean, then their autograd
// mirrors; here ONE pass reads each frame's C logits once, writes their gradient (and the predicted class) and leaves one partial
// per workgroup, and a one-workgroup pass finishes the per-utterance normalisation in a fixed order (no float atomics: the same bits
// on every call).  HBM-bound.  Algorithmic bytes: B*T*C*4 read + B*T*C*4 written (gradient) + B*T*8 (targets) [+ B*T*8 argmax].
//
//   C <= CE_REG_MAX (1024): one WAVE per frame row, lanes stride the classes, the row stays in registers (NV = 1..16 values per
//       lane, a template parameter): max, sum of exp and the gradient come from the one read.  Four waves per workgroup, each
//       takes every fourth row of the workgroup's CE_ROWS_REG frames.
//   C <= MG_CE_MAX_CLASSES (65536): one WORKGROUP per row, three sweeps (max, sum of exp, gradient).  A row is at most 256 KB: the
//       second and third sweep hit the L2, HBM still sees one read.  (An online max/sum would save the middle sweep's L2 reads but
//       rescales the running sum at every new maximum; the plain form keeps the sum a blocked sum of exp(x - max): tests/ce_ref64.py.)
// Pad frames (t >= n_b) read nothing: their gradient row is written as zero, their argmax as 0, their targets are never looked at.
#include "common.h"
#include "seq_reduce.h"

#define CE_REG_MAX 1024      // widest row of the register path (16 values per lane)
#define CE_ROWS_REG 16       // frames per workgroup, register path (4 per wave)
#define CE_ROWS_WIDE 4       // frames per workgroup, wide path (one after the other)
#define CE_IGNORE (-100)     // F.cross_entropy's default ignore_index

static inline int ce_rows_per_wg(int C) { return C <= CE_REG_MAX ? CE_ROWS_REG : CE_ROWS_WIDE; }

struct ce_args {
    const float* pred;
    const int64_t* target;
    const int64_t* seq_len;
    float* grad;
    int64_t* argmax;
    float* partial;
    int ldp, ldg, B, T, C;
    float grad_scale;
};

// The target of a valid frame: 0 = score it, 1 = ignore_index (loss and gradient 0), 2 = outside [0, C) (NaN loss, zero gradient)
__device__ __forceinline__ int ce_target_class(int64_t y, int C) { return y == CE_IGNORE ? 1 : (y < 0 || y >= C) ? 2 : 0; }

// Register path.  grid (ceil(T / CE_ROWS_REG), B), 256 threads.  partial[b * gridDim.x + chunk] = sum of the chunk's frame losses.
template <int NV>
__global__ __launch_bounds__(256) void masked_ce_reg_kernel(ce_args a) {
    __shared__ float red[4];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C = a.C;
    const int64_t n_b = mg_valid_frames(a.seq_len, b, a.T);
    const float coef = a.grad_scale / ((float)n_b * (float)a.B);
    const int t0 = blockIdx.x * CE_ROWS_REG;
    float acc = 0.f;
    for (int r = wave; r < CE_ROWS_REG; r += 4) {
        const int t = t0 + r;
        if (t >= a.T) break;
        const size_t row = (size_t)b * a.T + t;
        float* g = a.grad ? a.grad + row * a.ldg : nullptr;
        if (t >= n_b) {                                   // pad frame: zeros out, nothing in
            if (g) {
#pragma unroll
                for (int j = 0; j < NV; ++j)
                    if (lane + 64 * j < C) g[lane + 64 * j] = 0.f;
            }
            if (a.argmax && lane == 0) a.argmax[row] = 0;
            continue;
        }
        const float* x = a.pred + row * a.ldp;
        float v[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = lane + 64 * j < C ? x[lane + 64 * j] : -INFINITY;
        float m = v[0];
        int im = lane;                                    // lane 0 always holds class 0; lanes past C hold -inf and lose every merge
#pragma unroll
        for (int j = 1; j < NV; ++j)
            if (v[j] > m) {
                m = v[j];
                im = lane + 64 * j;
            }
        float mx = mg_wave_max(m);
        if (a.argmax) {
            mg_wave_argmax(m, im);
            if (lane == 0) a.argmax[row] = im < C ? im : C - 1;
        }
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            v[j] = expf(v[j] - mx);                       // exp(-inf) = 0: a -inf logit (and a lane past C) adds nothing
            s += v[j];
        }
        s = mg_wave_sum(s);
        const int64_t y = a.target[row];
        const int kind = ce_target_class(y, C);
        if (kind == 0) acc += (mx + logf(s)) - x[y];
        else if (kind == 2) acc += __builtin_nanf("");
        if (g) {
            const float inv = 1.f / s;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int c = lane + 64 * j;
                if (c < C) g[c] = kind == 0 ? (v[j] * inv - (c == (int)y ? 1.f : 0.f)) * coef : 0.f;
            }
        }
    }
    if (lane == 0) red[wave] = acc;                       // acc is wave-uniform
    __syncthreads();
    if (threadIdx.x == 0) a.partial[(size_t)b * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// Wide path.  grid (ceil(T / CE_ROWS_WIDE), B), 256 threads, the workgroup's rows one after the other.
__global__ __launch_bounds__(256) void masked_ce_wide_kernel(ce_args a) {
    __shared__ float red_m[4];
    __shared__ int red_i[4];
    __shared__ float red_s[4];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C;
    const int64_t n_b = mg_valid_frames(a.seq_len, b, a.T);
    const float coef = a.grad_scale / ((float)n_b * (float)a.B);
    const int t0 = blockIdx.x * CE_ROWS_WIDE;
    float acc = 0.f;
    for (int r = 0; r < CE_ROWS_WIDE; ++r) {
        const int t = t0 + r;
        if (t >= a.T) break;
        const size_t row = (size_t)b * a.T + t;
        float* g = a.grad ? a.grad + row * a.ldg : nullptr;
        if (t >= n_b) {
            if (g)
                for (int c = tid; c < C; c += 256) g[c] = 0.f;
            if (a.argmax && tid == 0) a.argmax[row] = 0;
            continue;
        }
        const float* x = a.pred + row * a.ldp;
        float m = -INFINITY;
        int im = 0x7fffffff;
        for (int c = tid; c < C; c += 256) {              // C > CE_REG_MAX: every thread owns at least four classes
            const float xv = x[c];
            if (xv > m || c == tid) {
                m = xv;
                im = c;
            }
        }
        mg_wave_argmax(m, im);
        __syncthreads();                                  // the previous row's readers of red_* are done
        if (lane == 0) {
            red_m[wave] = m;
            red_i[wave] = im;
        }
        __syncthreads();
        m = red_m[0];
        im = red_i[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) mg_argmax_merge(m, im, red_m[w], red_i[w]);
        const float mx = m;
        if (a.argmax && tid == 0) a.argmax[row] = im < C ? im : C - 1;
        float s = 0.f;
        for (int c = tid; c < C; c += 256) s += expf(x[c] - mx);
        s = mg_wave_sum(s);
        if (lane == 0) red_s[wave] = s;
        __syncthreads();
        s = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
        const int64_t y = a.target[row];
        const int kind = ce_target_class(y, C);
        if (kind == 0) acc += (mx + logf(s)) - x[y];
        else if (kind == 2) acc += __builtin_nanf("");
        if (g) {
            const float inv = 1.f / s;
            for (int c = tid; c < C; c += 256)
                g[c] = kind == 0 ? (expf(x[c] - mx) * inv - (c == (int)y ? 1.f : 0.f)) * coef : 0.f;
        }
    }
    if (tid == 0) a.partial[(size_t)b * gridDim.x + blockIdx.x] = acc;      // acc is workgroup-uniform
}

// One workgroup: loss = loss_weight * (1/B) sum_b ( sum_chunks partial[b,:] / n_b ) + loss_keep * loss, fixed summation order.
__global__ __launch_bounds__(256) void masked_ce_finish_kernel(const float* __restrict__ partial, const int64_t* __restrict__ seq_len, int B,
                                                               int T, int chunks, float loss_weight, float loss_keep,
                                                               float* __restrict__ loss) {
    __shared__ float red[256];
    const float sum = mg_utterance_mean_sum(partial, seq_len, B, T, chunks, red);
    if (threadIdx.x == 0) {
        const float l = loss_weight * (sum / (float)B);
        loss[0] = loss_keep != 0.f ? l + loss_keep * loss[0] : l;
    }
}

static size_t ce_ws_bytes(int B, int T, int C) {
    if (B <= 0 || T <= 0 || C <= 0) return 256;
    const int64_t chunks = mg_ceil_div(T, ce_rows_per_wg(C));
    return mg_align_up((size_t)B * (size_t)chunks * sizeof(float), 256);
}

extern "C" {

size_t mg_masked_ce_workspace_bytes(int B, int T, int C) { return ce_ws_bytes(B, T, C); }

int mg_masked_ce_f32(const float* pred, int ldp, int col0, const int64_t* target, const int64_t* seq_len, int B, int T, int C,
                     float grad_scale, float loss_weight, float loss_keep, float* loss, float* grad, int ldg, int gcol0, int64_t* argmax,
                     void* workspace, size_t workspace_bytes, void* stream) {
    MG_CHECK_ARG(pred && target && loss, "mg_masked_ce_f32: pred, target and loss must not be NULL");
    MG_CHECK_ARG(B > 0 && T > 0 && C > 0, "mg_masked_ce_f32: bad shape (B=%d T=%d C=%d)", B, T, C);
    MG_CHECK_ARG(C <= MG_CE_MAX_CLASSES, "mg_masked_ce_f32: C=%d exceeds the cap of %d classes", C, MG_CE_MAX_CLASSES);
    MG_CHECK_ARG(B <= 65535, "mg_masked_ce_f32: B=%d exceeds 65535", B);
    MG_CHECK_ARG(col0 >= 0 && (int64_t)ldp >= (int64_t)col0 + C, "mg_masked_ce_f32: columns [%d, %d + %d) do not fit the row stride ldp=%d",
                 col0, col0, C, ldp);
    MG_CHECK_ARG(!grad || (gcol0 >= 0 && (int64_t)ldg >= (int64_t)gcol0 + C),
                 "mg_masked_ce_f32: gradient columns [%d, %d + %d) do not fit the row stride ldg=%d", gcol0, gcol0, C, ldg);
    if (!workspace || workspace_bytes < ce_ws_bytes(B, T, C)) {
        mg_set_error("mg_masked_ce_f32: workspace of %zu bytes needed, got %zu", ce_ws_bytes(B, T, C), workspace_bytes);
        return MG_EWORKSPACE;
    }
    const int chunks = (int)mg_ceil_div(T, ce_rows_per_wg(C));
    hipStream_t st = (hipStream_t)stream;
    ce_args a;
    a.pred = pred + col0;
    a.target = target;
    a.seq_len = seq_len;
    a.grad = grad ? grad + gcol0 : nullptr;
    a.argmax = argmax;
    a.partial = (float*)workspace;
    a.ldp = ldp;
    a.ldg = ldg;
    a.B = B;
    a.T = T;
    a.C = C;
    a.grad_scale = grad_scale;
    const dim3 grid(chunks, B);
#define LAUNCH_REG(NV_) hipLaunchKernelGGL((masked_ce_reg_kernel<NV_>), grid, dim3(256), 0, st, a)
    if (C <= 64) LAUNCH_REG(1);
    else if (C <= 128) LAUNCH_REG(2);
    else if (C <= 256) LAUNCH_REG(4);
    else if (C <= 512) LAUNCH_REG(8);
    else if (C <= CE_REG_MAX) LAUNCH_REG(16);
    else hipLaunchKernelGGL(masked_ce_wide_kernel, grid, dim3(256), 0, st, a);
#undef LAUNCH_REG
    MG_CHECK_LAUNCH("mg_masked_ce_f32/rows");
    hipLaunchKernelGGL(masked_ce_finish_kernel, dim3(1), dim3(256), 0, st, a.partial, seq_len, B, T, chunks, loss_weight, loss_keep, loss);
    MG_CHECK_LAUNCH("mg_masked_ce_f32/finish");
    return MG_OK;
}

}  // extern "C"
