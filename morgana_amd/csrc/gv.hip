// K26 - global-variance loss and its backward: losses.gv / losses.global_variance (Toda & Tokuda 2007; the reference has none).
//
//   m[b,d] = mean_{t < n_b} x[b,t,d],   v[b,d] = mean_{t < n_b} (x[b,t,d] - m[b,d])^2,   f(v) = log(v + eps) | v,
//   loss   = (1 / (B D)) sum_{b,d} ( f(v_pred[b,d]) - f(v_tgt[b,d]) )^2,                  n_b = min(max(seq_len[b], 0), T)
//   grad[b,t,d] = g c[b,d] (x[b,t,d] - m_pred[b,d]),   c = (2 / (B D)) (f(v_pred) - f(v_tgt)) f'(v_pred) (2 / n_b)
//
// Composed of torch ops this is a mask, two means, two centred squares, two more means, two logs, a difference, a square and a mean
// over two (B, T, D) operands, then their autograd mirrors.  Here the forward is one streaming pass over the valid frames of both
// operands plus a finish over the (b, d) pairs, the backward one streaming pass that reads the predictions and writes the dense gradient;
// what is kept between the two is (m_pred, c): 16 B D bytes.
//
// Numerics (moments.h: the accumulator, the streaming pass and the tree are shared with colstats.hip).  No sum of raw squares: an
// accumulator sums d = x - k and d^2 in float64 for at most MG_MOMENTS_FLUSH values, k being the first value it saw, turns them into
// (n, mean, M2 = s2 - s1^2 / n) and folds that into its running triple by Chan's update.  Means travel as mean - anchor, anchor = x[b,0,d] (0 when that is not finite): held in full a
// mean would be rounded relative to the column's offset at every merge, and the delta^2 terms would inherit it.  The anchor comes
// back once, in the finish.  A constant column gives s1 = s2 = 0 and delta = 0 at every merge: v == 0.0 exactly.
//
// Summation order.  Launch 1, grid (chunks, B, operands): a workgroup owns frames [c CF, (c + 1) CF) of utterance b of one operand,
// CF = GV_CHUNK_FRAMES, cut to the valid ones and read as a flat array of len D elements in steps of W = R D elements (R whole frames; W the largest such
// multiple of 4 up to GV_STEP, so that narrow features fill the lanes).  ENTRY e of a step (frame e / D of the step, column e % D)
// has one accumulator, which takes the elements m W + e in ascending m; the R entries of a column then meet in a fixed halving tree
// in LDS, the chunks of an utterance in ascending order (launch 2), the (b, d) terms of the loss in a fixed tree.  All of it is a
// function of (b, t, d) alone, not of strides, alignment or the kernel path: R and W depend on D only, and the two paths differ in
// which thread holds an entry, not in what an entry sums.  Floating-point contraction is off in this file so that the two paths
// cannot be compiled into different roundings of the same expression.
//
//   * vec path (stride_d == 1, stride_t == D, W % 4 == 0): 16-byte loads at 16-byte-aligned addresses whatever the chunk's own
//     alignment: with the chunk starting `pre` floats behind a boundary, register j of quad q holds entry 4 q - pre + j; the quads
//     across the ends of a step or of the chunk load their valid elements one by one.  Nothing outside the valid frames is read.
//   * generic path (any strides; also contiguous rows whose D leaves no step that is a multiple of 4, D odd and above 256): one
//     element per load, thread q + 256 p holds entry q + 256 p, so a unit stride_d still coalesces.
//
// Pad frames are never read (losses.mdn's rule): a NaN there changes nothing.  No float atomics (one integer ticket per workgroup of
// the finish), no host read, capturable.
#include "common.h"

#pragma clang fp contract(off)
#include "moments.h"          // after the pragma, on purpose: the shared pass is compiled without contraction here
#include "seq_reduce.h"

#define GV_THREADS 256
#define GV_CHUNK_FRAMES 256        // frames of one utterance per workgroup of launch 1
#define GV_STEP 1024               // elements per step, at most (D <= GV_STEP)
#define GV_FINISH_THREADS 256       // one (b, d) item per thread of the finish
#define GV_FINISH_BATCH 4          // chunks whose records it loads at once
#define GV_BWD_CHUNK 8192          // gradient elements of one utterance per workgroup of the backward

struct gv_plan {
    int vec_ok;    // W % 4 == 0: contiguous rows may take the 16-byte path
    int R, W;      // frames and elements per step
};

static inline gv_plan gv_plan_of(int D) {
    gv_plan p;
    const int q = D % 4 == 0 ? 1 : D % 2 == 0 ? 2 : 4;       // R must be a multiple of it for W % 4 == 0
    int R = GV_STEP / D;
    if (R > GV_CHUNK_FRAMES) R = GV_CHUNK_FRAMES;
    R -= R % q;
    p.vec_ok = R >= 1;
    if (!p.vec_ok) R = GV_STEP / D > 1 ? GV_STEP / D : 1;
    p.R = R;
    p.W = R * D;
    return p;
}

static inline int64_t gv_chunks(int T) { return mg_ceil_div(T, GV_CHUNK_FRAMES); }

// The workspace, each part behind a 256-byte boundary: records [op][b][c][2][D] float64, the merge weights [b][c][2] float64, the
// finish's partial sums [workgroup] float64 and its arrival counter (one 32-bit word).
static inline size_t gv_finish_groups(int B, int D) { return (size_t)mg_ceil_div((int64_t)B * D, GV_FINISH_THREADS); }
static inline size_t gv_records_bytes(int B, int T, int D) {
    return mg_align_up((size_t)2 * (size_t)B * (size_t)gv_chunks(T) * 2 * (size_t)D * sizeof(double), 256);
}
static inline size_t gv_weights_bytes(int B, int T) { return mg_align_up((size_t)B * (size_t)gv_chunks(T) * 2 * sizeof(double), 256); }
static inline size_t gv_partials_bytes(int B, int D) { return mg_align_up(gv_finish_groups(B, D) * sizeof(double), 256); }

static size_t gv_ws_bytes(int B, int T, int D) {
    if (B <= 0 || T <= 0 || D <= 0 || D > MG_GV_MAX_D) return 0;
    return gv_records_bytes(B, T, D) + gv_weights_bytes(B, T) + gv_partials_bytes(B, D) + 256;
}

__device__ __forceinline__ double gv_anchor(const float* first, int64_t stride_d, int col) {
    const float v = first[(int64_t)col * stride_d];
    return __builtin_isfinite(v) ? (double)v : 0.0;
}

// Workgroup (c, b, operand): `len` >= 1 valid frames from `base` on -> rec[0 .. D) = mean - anchor, rec[D .. 2 D) = M2.
template <int VEC>
__device__ __forceinline__ void gv_chunk_moments(const float* __restrict__ base, int64_t stride_t, int64_t stride_d,
                                                 const float* __restrict__ first, int len, int D, int R, int W, double* s_mean,
                                                 double* s_m2, int* s_n, double* __restrict__ rec) {
    mg_stream_moments<VEC, false>(
        base, stride_t, stride_d, len, D, R, W, 0, 1, [&](int col) { return gv_anchor(first, stride_d, col); }, [](int, float, float) {},
        s_mean, s_m2, s_n);
    mg_fold_step_frames(R, D, s_mean, s_m2, s_n);
    for (int d = threadIdx.x; d < D; d += GV_THREADS) {
        rec[d] = s_mean[d];
        rec[D + d] = s_m2[d];
    }
}

// Launch 1, grid (chunks, B, operands).  records [op][b][c][2][D] float64; a chunk without a valid frame writes nothing (the finish
// knows its count is 0).  The workgroup of operand 0 also leaves the two weights of Chan's update with which the finish folds chunk
// c onto the chunks before it - nb / n and na nb / n, functions of (b, c) alone - so that the finish divides nothing per column.
__global__ __launch_bounds__(GV_THREADS) void gv_partial_kernel(const float* __restrict__ pred, int64_t p_sb, int64_t p_st, int64_t p_sd,
                                                                int p_vec, const float* __restrict__ tgt, int64_t t_sb, int64_t t_st,
                                                                int64_t t_sd, int t_vec, const int64_t* __restrict__ seq_len, int T, int D,
                                                                int R, int W, double* __restrict__ records,
                                                                double* __restrict__ weights, unsigned* __restrict__ arrivals) {
    extern __shared__ __attribute__((aligned(16))) double s_gv[];
    double* s_mean = s_gv;                                   // [W]
    double* s_m2 = s_gv + W;                                 // [W]
    int* s_n = (int*)(s_gv + 2 * (size_t)W);                 // [W]
    const int b = blockIdx.y, c = blockIdx.x, B = gridDim.y, CH = gridDim.x;
    if (b == 0 && c == 0 && blockIdx.z == 0 && threadIdx.x == 0) arrivals[0] = 0u;      // the finish counts its workgroups from 0
    const int64_t n_b = mg_valid_frames(seq_len, b, T);
    const int64_t t0 = (int64_t)c * GV_CHUNK_FRAMES;
    if (n_b <= t0) return;                                   // workgroup-uniform: only pad frames here
    const int len = (int)(n_b - t0 < GV_CHUNK_FRAMES ? n_b - t0 : GV_CHUNK_FRAMES);
    const int op = blockIdx.z;
    if (op == 0 && threadIdx.x == 0) {
        const double na = (double)t0, nb = (double)len, n = na + nb;
        weights[((size_t)b * CH + c) * 2] = nb / n;
        weights[((size_t)b * CH + c) * 2 + 1] = na * nb / n;
    }
    const float* x = op ? tgt : pred;
    const int64_t sb = op ? t_sb : p_sb, st = op ? t_st : p_st, sd = op ? t_sd : p_sd;
    const float* first = x + (int64_t)b * sb;
    double* rec = records + (((size_t)op * B + b) * CH + c) * 2 * (size_t)D;
    if (op ? t_vec : p_vec)
        gv_chunk_moments<4>(first + t0 * st, st, 1, first, len, D, R, W, s_mean, s_m2, s_n, rec);      // vec: sd == 1
    else
        gv_chunk_moments<1>(first + t0 * st, st, sd, first, len, D, R, W, s_mean, s_m2, s_n, rec);
}

// Launch 2, the finish, one thread per (b, d): chunks merged in ascending order with the weights of launch 1 (the update of
// moments.h, the same operations; the records of GV_FINISH_BATCH chunks of both operands are loaded at once, ahead of the first
// merge), f in float64, state and variances.  The loss: a workgroup sums its 256 terms in a fixed tree, publishes the sum and takes
// a ticket (one integer add, release / acquire at device scope); the workgroup that draws the last ticket - every other sum was
// published before its add - sums the workgroups' sums in index order and a fixed tree and rounds once.  WHICH workgroup that is
// depends on timing, WHAT it computes does not.  Nobody waits for anybody: no spin, no float atomics.  (With one workgroup for all
// of it, B D = 11 520 items took 55 - 85 us on one compute unit: two float64 logs and three divisions per item.)
__global__ __launch_bounds__(GV_FINISH_THREADS) void gv_finish_kernel(const float* __restrict__ pred, int64_t p_sb, int64_t p_sd,
                                                                      const float* __restrict__ tgt, int64_t t_sb, int64_t t_sd,
                                                                      const int64_t* __restrict__ seq_len, int B, int T, int D, int CH,
                                                                      const double* __restrict__ records,
                                                                      const double* __restrict__ weights, int log_variance, double eps,
                                                                      float* __restrict__ loss, double* __restrict__ state,
                                                                      float* __restrict__ v_pred, float* __restrict__ v_tgt,
                                                                      double* partials, unsigned* arrivals) {
    __shared__ double red[GV_FINISH_THREADS / 64];
    __shared__ int s_last;
    const double nan = __builtin_nan("");
    const int64_t items = (int64_t)B * D;
    const int n_ops = tgt ? 2 : 1;
    double acc = 0.0;
    const int64_t i = (int64_t)blockIdx.x * GV_FINISH_THREADS + threadIdx.x;
    if (i < items) {
        const int b = (int)(i / D), d = (int)(i - (int64_t)b * D);
        const int64_t n_b = mg_valid_frames(seq_len, b, T);
        const int nch = (int)((n_b + GV_CHUNK_FRAMES - 1) / GV_CHUNK_FRAMES);      // chunks that hold frames: the ones launch 1 wrote
        const double* w = weights + (size_t)b * CH * 2;
        const double* rec[2];
        double ma[2] = {0.0, 0.0}, Ma[2] = {0.0, 0.0}, anchor[2] = {0.0, 0.0};
#pragma unroll
        for (int op = 0; op < 2; ++op) {
            rec[op] = records + ((size_t)(op < n_ops ? op : 0) * B + b) * CH * 2 * (size_t)D + d;
            if (nch > 0 && op < n_ops) {
                ma[op] = rec[op][0];
                Ma[op] = rec[op][D];
                anchor[op] = op ? gv_anchor(tgt + (int64_t)b * t_sb, t_sd, d) : gv_anchor(pred + (int64_t)b * p_sb, p_sd, d);
            }
        }
        for (int c0 = 1; c0 < nch; c0 += GV_FINISH_BATCH) {
            double mb[2][GV_FINISH_BATCH], Mb[2][GV_FINISH_BATCH], w1[GV_FINISH_BATCH], w2[GV_FINISH_BATCH];
#pragma unroll
            for (int u = 0; u < GV_FINISH_BATCH; ++u) {
                const int c = c0 + u < nch ? c0 + u : 0;      // chunk 0 stands in for one that is not there
                w1[u] = w[2 * c];
                w2[u] = w[2 * c + 1];
#pragma unroll
                for (int op = 0; op < 2; ++op) {
                    mb[op][u] = rec[op][(size_t)c * 2 * D];
                    Mb[op][u] = rec[op][(size_t)c * 2 * D + D];
                }
            }
#pragma unroll
            for (int u = 0; u < GV_FINISH_BATCH; ++u) {
                if (c0 + u >= nch) continue;
#pragma unroll
                for (int op = 0; op < 2; ++op) {
                    const double delta = mb[op][u] - ma[op];
                    ma[op] = ma[op] + delta * w1[u];
                    Ma[op] = Ma[op] + Mb[op][u] + delta * delta * w2[u];
                }
            }
        }
        double f[2] = {0.0, 0.0}, v[2] = {nan, nan};
#pragma unroll
        for (int op = 0; op < 2; ++op) {
            if (op >= n_ops) continue;
            if (n_b > 0) v[op] = Ma[op] / (double)n_b;
            f[op] = log_variance ? log(v[op] + eps) : v[op];
        }
        if (v_pred) v_pred[i] = (float)v[0];
        if (tgt) {
            if (v_tgt) v_tgt[i] = (float)v[1];
            const double delta = f[0] - f[1];
            const double slope = log_variance ? 1.0 / (v[0] + eps) : 1.0;
            state[2 * i] = n_b > 0 ? anchor[0] + ma[0] : nan;
            state[2 * i + 1] = n_b > 0 ? (2.0 / ((double)B * (double)D)) * delta * slope * (2.0 / (double)n_b) : nan;
            acc = delta * delta;
        }
    }
    if (!tgt) return;
    const double mine = mg_block_sum_f64(acc, red);
    if (threadIdx.x == 0) {
        __hip_atomic_store(&partials[blockIdx.x], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned ticket = __hip_atomic_fetch_add(arrivals, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = ticket == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    double sum = 0.0;
    for (unsigned j = threadIdx.x; j < gridDim.x; j += GV_FINISH_THREADS)
        sum += __hip_atomic_load(&partials[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double total = mg_block_sum_f64(sum, red);
    if (threadIdx.x == 0) loss[0] = (float)(total / ((double)B * (double)D));
}

// grid (chunks of GV_BWD_CHUNK elements, B): grad[b, t, d] = (float)(g c[b,d] (x[b,t,d] - m[b,d])) for t < n_b, 0 for pad frames
// (not read), NaN everywhere when n_b == 0.  The gradient is contiguous: a scalar head brings each chunk to 16-byte stores, a scalar
// tail ends it; a quad of contiguous predictions that is itself 16-byte aligned and wholly valid is loaded as one.
__global__ __launch_bounds__(GV_THREADS) void gv_bwd_kernel(const float* __restrict__ grad_loss, const double* __restrict__ state,
                                                            const float* __restrict__ pred, int64_t sb, int64_t st, int64_t sd,
                                                            const int64_t* __restrict__ seq_len, int T, int D, float* __restrict__ grad) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t row_elems = (int64_t)T * D;
    const int64_t lo = (int64_t)blockIdx.x * GV_BWD_CHUNK;
    const int len = (int)(row_elems - lo < GV_BWD_CHUNK ? row_elems - lo : GV_BWD_CHUNK);
    const int64_t n_b = mg_valid_frames(seq_len, b, T);
    const int64_t valid = n_b * D - lo;                      // local indices below it are valid frames
    const float off = n_b > 0 ? 0.f : __builtin_nanf("");
    const double g = (double)grad_loss[0];
    const float* xb = pred + (int64_t)b * sb;
    const double* sbd = state + (size_t)b * 2 * (size_t)D;
    const bool contiguous = sd == 1 && st == D;
    float* p = grad + (int64_t)b * row_elems + lo;

    auto one = [&](int i) -> float {                         // local index i -> its gradient
        if (i >= valid) return off;
        const int64_t e = lo + i;
        const int64_t t = e / D;
        const int d = (int)(e - t * D);
        const double x = (double)xb[t * st + (int64_t)d * sd];
        return (float)(g * sbd[2 * d + 1] * (x - sbd[2 * d]));
    };

    int head = (int)((4u - (unsigned)(((uintptr_t)p >> 2) & 3u)) & 3u);
    if (head > len) head = len;
    const int nvec = (len - head) >> 2;
    const int tail = head + 4 * nvec;
    if (tid < head) p[tid] = one(tid);
    f32x4* pv = reinterpret_cast<f32x4*>(p + head);
    for (int m = tid; m < nvec; m += GV_THREADS) {
        const int i0 = head + 4 * m;
        f32x4 v;
        if (i0 >= valid) {
            v[0] = v[1] = v[2] = v[3] = off;
        } else {
            const int64_t e0 = lo + i0;
            int64_t t = e0 / D;
            int d = (int)(e0 - t * D);
            float x[4];
            const bool whole = i0 + 4 <= valid;
            if (whole && contiguous && (((uintptr_t)(xb + e0)) & 15u) == 0) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(xb + e0);
#pragma unroll
                for (int j = 0; j < 4; ++j) x[j] = xv[j];
            } else {
                int64_t tt = t;
                int dd = d;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    x[j] = i0 + j < valid ? xb[tt * st + (int64_t)dd * sd] : 0.f;
                    if (++dd == D) { dd = 0; ++tt; }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = i0 + j < valid ? (float)(g * sbd[2 * d + 1] * ((double)x[j] - sbd[2 * d])) : off;
                if (++d == D) d = 0;
            }
        }
        pv[m] = v;
    }
    if (tail + tid < len) p[tail + tid] = one(tail + tid);
}

extern "C" {

int mg_gv_chunk_frames(void) { return GV_CHUNK_FRAMES; }

size_t mg_gv_workspace_bytes(int B, int T, int D) { return gv_ws_bytes(B, T, D); }

int mg_gv_f32(const float* pred, int64_t pred_stride_b, int64_t pred_stride_t, int64_t pred_stride_d, const float* tgt,
              int64_t tgt_stride_b, int64_t tgt_stride_t, int64_t tgt_stride_d, const int64_t* seq_len, int B, int T, int D,
              int log_variance, double eps, float* loss, double* state, float* v_pred, float* v_tgt, void* workspace,
              size_t workspace_bytes, void* stream) {
    MG_CHECK_ARG(pred, "mg_gv_f32: pred must not be NULL");
    MG_CHECK_ARG(tgt ? (loss && state) : (v_pred != NULL),
                 "mg_gv_f32: loss and state must not be NULL (without tgt: v_pred must not be NULL)");
    MG_CHECK_ARG(B > 0 && T > 0 && D > 0, "mg_gv_f32: bad shape (B=%d T=%d D=%d)", B, T, D);
    MG_CHECK_ARG(B <= 65535, "mg_gv_f32: B=%d exceeds 65535", B);
    MG_CHECK_ARG(D <= MG_GV_MAX_D, "mg_gv_f32: D=%d exceeds %d (MG_GV_MAX_D)", D, MG_GV_MAX_D);
    MG_CHECK_ARG(pred_stride_b >= 0 && pred_stride_t >= 0 && pred_stride_d >= 0 && tgt_stride_b >= 0 && tgt_stride_t >= 0 && tgt_stride_d >= 0,
                 "mg_gv_f32: negative stride (pred %lld, %lld, %lld; tgt %lld, %lld, %lld)", (long long)pred_stride_b,
                 (long long)pred_stride_t, (long long)pred_stride_d, (long long)tgt_stride_b, (long long)tgt_stride_t, (long long)tgt_stride_d);
    MG_CHECK_ARG(!log_variance || eps >= 0.0, "mg_gv_f32: eps=%g must not be negative", eps);
    MG_CHECK_ARG(((uintptr_t)pred & 3u) == 0 && ((uintptr_t)tgt & 3u) == 0 && ((uintptr_t)loss & 3u) == 0 && ((uintptr_t)v_pred & 3u) == 0 &&
                     ((uintptr_t)v_tgt & 3u) == 0 && ((uintptr_t)state & 7u) == 0 && ((uintptr_t)workspace & 7u) == 0 &&
                     ((uintptr_t)seq_len & 7u) == 0,
                 "mg_gv_f32: pred, tgt, loss, v_pred and v_tgt must be 4-byte, state, seq_len and the workspace 8-byte aligned");
    if (!workspace || workspace_bytes < gv_ws_bytes(B, T, D)) {
        mg_set_error("mg_gv_f32: workspace of %zu bytes needed, got %zu", gv_ws_bytes(B, T, D), workspace ? workspace_bytes : (size_t)0);
        return MG_EWORKSPACE;
    }
    const gv_plan p = gv_plan_of(D);
    const int p_vec = p.vec_ok && pred_stride_d == 1 && pred_stride_t == D;
    const int t_vec = p.vec_ok && tgt && tgt_stride_d == 1 && tgt_stride_t == D;
    const int chunks = (int)gv_chunks(T);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    double* records = (double*)ws;
    double* weights = (double*)(ws + gv_records_bytes(B, T, D));
    double* partials = (double*)(ws + gv_records_bytes(B, T, D) + gv_weights_bytes(B, T));
    unsigned* arrivals = (unsigned*)(ws + gv_records_bytes(B, T, D) + gv_weights_bytes(B, T) + gv_partials_bytes(B, D));
    hipLaunchKernelGGL(gv_partial_kernel, dim3((unsigned)chunks, (unsigned)B, tgt ? 2u : 1u), dim3(GV_THREADS), (size_t)20 * p.W, st, pred,
                       pred_stride_b, pred_stride_t, pred_stride_d, p_vec, tgt, tgt_stride_b, tgt_stride_t, tgt_stride_d, t_vec, seq_len, T, D,
                       p.R, p.W, records, weights, arrivals);
    MG_CHECK_LAUNCH("mg_gv_f32/moments");
    hipLaunchKernelGGL(gv_finish_kernel, dim3((unsigned)gv_finish_groups(B, D)), dim3(GV_FINISH_THREADS), 0, st, pred, pred_stride_b,
                       pred_stride_d, tgt, tgt_stride_b, tgt_stride_d, seq_len, B, T, D, chunks, (const double*)records,
                       (const double*)weights, log_variance, eps, loss, state, v_pred, v_tgt, partials, arrivals);
    MG_CHECK_LAUNCH("mg_gv_f32/finish");
    return MG_OK;
}

int mg_gv_bwd_f32(const float* grad_loss, const double* state, const float* pred, int64_t pred_stride_b, int64_t pred_stride_t,
                  int64_t pred_stride_d, const int64_t* seq_len, int B, int T, int D, float* grad, void* stream) {
    MG_CHECK_ARG(grad_loss && state && pred && grad, "mg_gv_bwd_f32: grad_loss, state, pred and grad must not be NULL");
    MG_CHECK_ARG(B > 0 && T > 0 && D > 0, "mg_gv_bwd_f32: bad shape (B=%d T=%d D=%d)", B, T, D);
    MG_CHECK_ARG(B <= 65535, "mg_gv_bwd_f32: B=%d exceeds 65535", B);
    MG_CHECK_ARG(D <= MG_GV_MAX_D, "mg_gv_bwd_f32: D=%d exceeds %d (MG_GV_MAX_D)", D, MG_GV_MAX_D);
    MG_CHECK_ARG(pred_stride_b >= 0 && pred_stride_t >= 0 && pred_stride_d >= 0, "mg_gv_bwd_f32: negative stride (%lld, %lld, %lld)",
                 (long long)pred_stride_b, (long long)pred_stride_t, (long long)pred_stride_d);
    MG_CHECK_ARG(((uintptr_t)grad_loss & 3u) == 0 && ((uintptr_t)pred & 3u) == 0 && ((uintptr_t)grad & 3u) == 0 &&
                     ((uintptr_t)state & 7u) == 0 && ((uintptr_t)seq_len & 7u) == 0,
                 "mg_gv_bwd_f32: grad_loss, pred and grad must be 4-byte, state and seq_len 8-byte aligned");
    const int64_t chunks = mg_ceil_div((int64_t)T * D, GV_BWD_CHUNK);
    MG_CHECK_ARG(chunks <= 0x7fffffff, "mg_gv_bwd_f32: T * D = %lld is too large", (long long)T * D);
    hipLaunchKernelGGL(gv_bwd_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(GV_THREADS), 0, (hipStream_t)stream, grad_loss, state, pred,
                       pred_stride_b, pred_stride_t, pred_stride_d, seq_len, T, D, grad);
    MG_CHECK_LAUNCH("mg_gv_bwd_f32");
    return MG_OK;
}

}  // extern "C"
