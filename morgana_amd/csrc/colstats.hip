// K22 - per-column corpus statistics (count, mean, M2 = sum (x - mean)^2, min, max) over the valid frames of a batch, added to a
// running float64 state on the device: what the normaliser parameter files ({name}_mvn.json, {name}_minmax.json) are made of.
// The reference takes those files from the un-vendored tts_data_tools; nothing in it computes them.
//
// Numerics.  No sum of raw squares: an accumulator sums d = x - k and d^2 in float64 for at most MG_MOMENTS_FLUSH values, k being
// the first value it saw (x - k is exact or rounded once in float64, and small: the column's spread, not its offset), turns the sums
// into (n, mean = k + s1 / n, M2 = s2 - s1^2 / n) and folds that chunk into its running (n, mean, M2) by Chan's update
//     delta = mean_b - mean_a,   mean = mean_a + delta n_b / n,   M2 = M2_a + M2_b + delta^2 n_a n_b / n.
// Everything after the chunk is that update in float64 in a fixed order: the accumulators of a workgroup over a tree in LDS, the
// workgroups' records in job order (second launch), the state last.  n == 0 partials are skipped, never divided by.  A constant
// column gives s1 = s2 = 0 and delta = 0 at every merge: mean == c and M2 == 0.0 exactly.  A NaN or an infinity makes its column's
// mean and M2 non-finite (inf - inf); the count still counts the frame and the other columns never see it.  min / max ignore NaNs.
//
// No float atomics, the same bits on every call: a thread takes fixed elements in a fixed order.  The only atomics are integer
// min / max on an order-preserving key of the float in LDS, whose result does not depend on the order of arrival.
//
// Memory.  One streaming pass, every byte read once.  Launch 1, grid (chunks, B): workgroup (c, b) works on item b alone (one
// group), on the steps c, c + chunks, ... of the item - a step is W contiguous elements = W / D whole frames, W the largest multiple
// of lcm(D, 4) up to 1024 (of D up to 256 on the scalar path), so that a thread's elements keep their columns from step to step
// and narrow features (D = 1, 3, 5) fill the lanes: the item is read as a flat array, the column is (index mod W) mod D.  With
// ld == D the loads are 16 bytes wide from the 16-byte boundary below the item's first element, whatever D: the quads that
// straddle the ends of a step or of the item (at most two per step) load their valid elements one by one and nothing outside
// [first, last) is read.  Wide odd features (lcm(D, 4) > 1024: D = 609 -> W = 2436) take several quads per thread, one after the
// other.  Launch 2 reads the job records (8 + 24 D bytes each, at most COLSTATS_MAX_JOBS of them) and the state.
#include "common.h"
#include "item_norm.h"
#include "moments.h"      // the accumulator, the streaming pass, the tree and Chan's update; no fp pragma in front of it, on purpose

#define COLSTATS_THREADS 256
#define COLSTATS_MAX_JOBS 1024     // workgroups of launch 1 when B allows: four per CU
#define COLSTATS_MIN_STEPS 16      // steps per workgroup before an item is cut into more chunks
#define COLSTATS_LDS_BYTES 65536
#define COLSTATS_MERGE_COLS 4      // launch 2: 4 columns x 64 job lanes per workgroup (the lanes' runs of records are its latency)
#define COLSTATS_MERGE_LANES 64

struct colstats_plan {
    int vec;       // 4: 16-byte loads over the flat item (ld == D); 1: one element per load, any ld
    int W;         // elements per step, a multiple of D (and of 4 when vec == 4)
};

static inline int colstats_gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

static inline colstats_plan colstats_plan_of(int D, bool contiguous) {
    colstats_plan p;
    const int64_t unit = (int64_t)D * 4 / colstats_gcd(D, 4);
    if (contiguous && 20 * unit + 8 * (int64_t)D <= COLSTATS_LDS_BYTES) {
        p.vec = 4;
        p.W = (int)(unit <= 1024 ? unit * (1024 / unit) : unit);
    } else {
        p.vec = 1;
        p.W = D <= COLSTATS_THREADS ? D * (COLSTATS_THREADS / D) : D;
    }
    return p;
}

static inline size_t colstats_lds_bytes(int W, int D) { return (size_t)20 * W + (size_t)8 * D; }
static inline size_t colstats_job_stride(int D) { return 8 + (size_t)24 * D; }

// chunks per item: from the longest item, so that a workgroup has COLSTATS_MIN_STEPS steps and there are at most COLSTATS_MAX_JOBS jobs
static inline int colstats_chunks(int B, int64_t max_rows, int D) {
    const colstats_plan p = colstats_plan_of(D, true);
    const int64_t steps = mg_ceil_div(max_rows, p.W / D);
    int64_t ch = mg_ceil_div(steps, COLSTATS_MIN_STEPS);
    const int64_t cap = COLSTATS_MAX_JOBS / B > 1 ? COLSTATS_MAX_JOBS / B : 1;
    if (ch > cap) ch = cap;
    return ch < 1 ? 1 : (int)ch;
}

// order-preserving key of a float (not a NaN) and back
__device__ __forceinline__ unsigned colstats_key(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float colstats_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// Means travel as (mean - anchor), anchor = the column's value in the first frame of the batch (0 if that is not finite): a mean
// held in full would be rounded to 2^-53 |mean| at every merge, and the delta^2 terms would inherit that - relative to the
// column's offset, not to its spread.  The anchor comes back once, where the batch meets the state.
__device__ __forceinline__ const float* colstats_anchor_row(const float* x, int64_t ld, int B, int T, const int64_t* offsets,
                                                            const int64_t* seq_len) {
    for (int b = 0; b < B; ++b) {
        if (offsets) {
            if (offsets[b + 1] > offsets[b]) return x + offsets[b] * ld;
        } else if (T > 0 && seq_len[b] > 0) {
            return x + (int64_t)b * T * ld;
        }
    }
    return nullptr;
}
__device__ __forceinline__ double colstats_anchor(const float* row, int col) {
    if (!row) return 0.0;
    const float v = row[col];
    return __builtin_isfinite(v) ? (double)v : 0.0;
}

// Launch 1.  Job (b, c) writes one record: n, (mean - anchor)[D], M2[D] (float64), min[D], max[D] (float32) of its share of item b.
template <int VEC>
__global__ __launch_bounds__(COLSTATS_THREADS) void colstats_partial_kernel(const float* __restrict__ x, int64_t ld, int D, int T,
                                                                            const int64_t* __restrict__ offsets,
                                                                            const int64_t* __restrict__ seq_len, int W,
                                                                            unsigned char* __restrict__ records, size_t job_stride) {
    extern __shared__ __attribute__((aligned(16))) double s_colstats[];
    double* s_mean = s_colstats;                             // [W]
    double* s_m2 = s_colstats + W;                           // [W]
    int* s_n = (int*)(s_colstats + 2 * (size_t)W);           // [W]
    unsigned* s_min = (unsigned*)(s_n + W);                  // [D]
    unsigned* s_max = s_min + D;                             // [D]

    const int tid = threadIdx.x;
    const int b = blockIdx.y, c = blockIdx.x, CH = gridDim.x;
    unsigned char* rec = records + ((size_t)b * CH + c) * job_stride;
    double* rec_mean = (double*)(rec + 8);
    double* rec_m2 = rec_mean + D;
    float* rec_min = (float*)(rec_m2 + D);
    float* rec_max = rec_min + D;

    int64_t lo, len;
    mg_item_rows(offsets, seq_len, T, b, lo, len);
    const int RS = W / D;                                    // frames per step
    const int64_t NS = (len + RS - 1) / RS;                  // steps of the item
    if (c >= NS) {                                           // workgroup-uniform: nothing of this item is ours
        if (tid == 0) *(double*)rec = 0.0;
        return;
    }
    const float* base = x + lo * ld;
    const float* anchor_row = colstats_anchor_row(x, ld, gridDim.y, T, offsets, seq_len);

    for (int d = tid; d < D; d += COLSTATS_THREADS) {
        s_min[d] = colstats_key(__builtin_inff());
        s_max[d] = colstats_key(-__builtin_inff());
    }
    __syncthreads();

    // the steps c, c + CH, ... of the item (VEC == 4: ld == D)
    mg_stream_moments<VEC, true>(
        base, ld, 1, len, D, RS, W, (int64_t)c, (int64_t)CH, [&](int col) { return colstats_anchor(anchor_row, col); },
        [&](int col, float mn, float mx) {
            atomicMin(&s_min[col], colstats_key(mn));
            atomicMax(&s_max[col], colstats_key(mx));
        },
        s_mean, s_m2, s_n);
    mg_fold_step_frames(RS, D, s_mean, s_m2, s_n);
    for (int d = tid; d < D; d += COLSTATS_THREADS) {
        rec_mean[d] = s_mean[d];
        rec_m2[d] = s_m2[d];
        rec_min[d] = colstats_unkey(s_min[d]);
        rec_max[d] = colstats_unkey(s_max[d]);
    }
    if (tid == 0) *(double*)rec = (double)s_n[0];            // every column of a job has the job's frame count
}

// Launch 2, grid (ceil(D / 4), S): the records of the items of group s, folded in job order - 64 lanes take consecutive runs of jobs,
// their results meet pairwise in lane order - and the state last.  An item whose item_row is outside [0, S) matches no group.
__global__ __launch_bounds__(COLSTATS_THREADS) void colstats_merge_kernel(const float* __restrict__ x, int64_t ld, int B, int T,
                                                                          const int64_t* __restrict__ offsets,
                                                                          const int64_t* __restrict__ seq_len,
                                                                          const unsigned char* __restrict__ records, size_t job_stride,
                                                                          int n_jobs, int CH, int D, const int32_t* __restrict__ item_row,
                                                                          double* __restrict__ state) {
    __shared__ double s_n[COLSTATS_MERGE_LANES][COLSTATS_MERGE_COLS], s_mean[COLSTATS_MERGE_LANES][COLSTATS_MERGE_COLS],
        s_m2[COLSTATS_MERGE_LANES][COLSTATS_MERGE_COLS];
    __shared__ float s_mn[COLSTATS_MERGE_LANES][COLSTATS_MERGE_COLS], s_mx[COLSTATS_MERGE_LANES][COLSTATS_MERGE_COLS];
    const int tid = threadIdx.x;
    const int cl = tid % COLSTATS_MERGE_COLS, lane = tid / COLSTATS_MERGE_COLS;
    const int col = blockIdx.x * COLSTATS_MERGE_COLS + cl;
    const int s = blockIdx.y;
    const bool live = col < D;
    const int ccol = live ? col : 0;
    const int per = (n_jobs + COLSTATS_MERGE_LANES - 1) / COLSTATS_MERGE_LANES;
    const int begin = lane * per;
    const int end = begin + per < n_jobs ? begin + per : n_jobs;

    double rn = 0.0, rmean = 0.0, rm2 = 0.0;
    float rmn = __builtin_inff(), rmx = -__builtin_inff();
    for (int j0 = begin; j0 < end; j0 += 4) {
        double n[4], me[4], m2[4];
        float mn[4], mx[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jj = j0 + u < end ? j0 + u : end - 1;   // a valid record either way; the extra copies are zeroed below
            const unsigned char* rec = records + (size_t)jj * job_stride;
            const double* rec_mean = (const double*)(rec + 8);
            const float* rec_min = (const float*)(rec_mean + 2 * (size_t)D);
            const bool match = item_row ? item_row[jj / CH] == s : true;
            n[u] = (j0 + u < end && match && live) ? *(const double*)rec : 0.0;
            me[u] = rec_mean[ccol];
            m2[u] = rec_mean[D + ccol];
            mn[u] = rec_min[ccol];
            mx[u] = rec_min[D + ccol];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (n[u] == 0.0) continue;                        // an empty job's other fields were never written
            mg_chan_merge(rn, rmean, rm2, n[u], me[u], m2[u]);
            rmn = fminf(rmn, mn[u]);
            rmx = fmaxf(rmx, mx[u]);
        }
    }
    s_n[lane][cl] = rn;
    s_mean[lane][cl] = rmean;
    s_m2[lane][cl] = rm2;
    s_mn[lane][cl] = rmn;
    s_mx[lane][cl] = rmx;
    __syncthreads();
    for (int st = 1; st < COLSTATS_MERGE_LANES; st <<= 1) {
        if (lane % (2 * st) == 0) {
            double na = s_n[lane][cl], ma = s_mean[lane][cl], Ma = s_m2[lane][cl];
            mg_chan_merge(na, ma, Ma, s_n[lane + st][cl], s_mean[lane + st][cl], s_m2[lane + st][cl]);
            s_n[lane][cl] = na;
            s_mean[lane][cl] = ma;
            s_m2[lane][cl] = Ma;
            s_mn[lane][cl] = fminf(s_mn[lane][cl], s_mn[lane + st][cl]);
            s_mx[lane][cl] = fmaxf(s_mx[lane][cl], s_mx[lane + st][cl]);
        }
        __syncthreads();
    }
    if (lane != 0 || !live) return;
    const double nb = s_n[0][cl];
    if (nb == 0.0) return;                                   // nothing of this group in the batch: the state stays as it is
    double* st_row = state + (size_t)s * MG_COLSTATS_FIELDS * D + col;
    double na = st_row[0], ma = st_row[(size_t)D], Ma = st_row[2 * (size_t)D];
    double mn = (double)s_mn[0][cl], mx = (double)s_mx[0][cl];
    if (na != 0.0) {                                         // count == 0: the other fields of the state are ignored
        mn = fmin(st_row[3 * (size_t)D], mn);
        mx = fmax(st_row[4 * (size_t)D], mx);
    }
    const double anchor = colstats_anchor(colstats_anchor_row(x, ld, B, T, offsets, seq_len), col);
    const double mb = s_mean[0][cl], Mb = s_m2[0][cl];       // mb: the batch's mean - anchor
    if (na == 0.0) {
        na = nb;
        ma = anchor + mb;
        Ma = Mb;
    } else {
        const double n = na + nb;
        const double delta = (anchor - ma) + mb;
        ma = ma + delta * (nb / n);
        Ma = Ma + Mb + delta * delta * (na * nb / n);
        na = n;
    }
    st_row[0] = na;
    st_row[(size_t)D] = ma;
    st_row[2 * (size_t)D] = Ma;
    st_row[3 * (size_t)D] = mn;
    st_row[4 * (size_t)D] = mx;
}

extern "C" {

size_t mg_column_stats_workspace_bytes(int B, int64_t max_rows, int D) {
    if (B <= 0 || D <= 0 || D > MG_COLSTATS_MAX_D || max_rows < 0) return 0;
    return (size_t)B * colstats_chunks(B, max_rows, D) * colstats_job_stride(D);
}

int mg_column_stats_f32(const float* x, int64_t ld, int D, int B, int T, const int64_t* offsets, const int64_t* seq_len,
                        const int32_t* item_row, int S, double* state, void* workspace, size_t workspace_bytes, void* stream) {
    MG_CHECK_ONE_LAYOUT("mg_column_stats_f32", offsets, seq_len, "(B, T, D)");
    MG_CHECK_ARG(D > 0 && D <= MG_COLSTATS_MAX_D, "mg_column_stats_f32: D=%d not in 1..%d", D, MG_COLSTATS_MAX_D);
    MG_CHECK_ARG(S > 0 && S <= 65535, "mg_column_stats_f32: S=%d groups not in 1..65535", S);
    MG_CHECK_ARG(S == 1 || item_row, "mg_column_stats_f32: S=%d groups need item_row", S);
    MG_CHECK_ARG(state, "mg_column_stats_f32: state must not be NULL");
    MG_CHECK_ARG(B >= 0 && B <= 65535, "mg_column_stats_f32: B=%d not in 0..65535", B);
    MG_CHECK_ARG(ld >= D, "mg_column_stats_f32: row stride ld=%lld is below D=%d", (long long)ld, D);
    MG_CHECK_ARG(offsets || T >= 0, "mg_column_stats_f32: T=%d must not be negative", T);
    if (B == 0) return MG_OK;
    MG_CHECK_ARG(x && workspace, "mg_column_stats_f32: x and workspace must not be NULL");
    MG_CHECK_ARG(((uintptr_t)x & 3u) == 0 && ((uintptr_t)item_row & 3u) == 0 && ((uintptr_t)state & 7u) == 0 &&
                     ((uintptr_t)workspace & 7u) == 0 && ((uintptr_t)offsets & 7u) == 0 && ((uintptr_t)seq_len & 7u) == 0,
                 "mg_column_stats_f32: x and item_row must be 4-byte, state, workspace, offsets and seq_len 8-byte aligned");
    const size_t stride = colstats_job_stride(D);
    int ch;
    if (seq_len) {
        ch = colstats_chunks(B, T, D);
    } else {                                                  // the longest item is known to the caller alone: it sized the workspace for it
        const int64_t cap = COLSTATS_MAX_JOBS / B > 1 ? COLSTATS_MAX_JOBS / B : 1;
        const size_t fit = workspace_bytes / stride / (size_t)B;
        ch = (int)(fit < (size_t)cap ? fit : (size_t)cap);
    }
    if (ch < 1 || (size_t)B * ch * stride > workspace_bytes) {
        mg_set_error("mg_column_stats_f32: workspace of %zu bytes is too small (mg_column_stats_workspace_bytes: %zu for rows of one item)",
                     workspace_bytes, (size_t)B * (seq_len ? colstats_chunks(B, T, D) : 1) * stride);
        return MG_EWORKSPACE;
    }
    if (seq_len && T == 0) return MG_OK;
    const colstats_plan p = colstats_plan_of(D, ld == D);
    const size_t lds = colstats_lds_bytes(p.W, D);
    const dim3 grid((unsigned)ch, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (p.vec == 4)
        hipLaunchKernelGGL((colstats_partial_kernel<4>), grid, dim3(COLSTATS_THREADS), lds, st, x, ld, D, T, offsets, seq_len, p.W,
                           (unsigned char*)workspace, stride);
    else
        hipLaunchKernelGGL((colstats_partial_kernel<1>), grid, dim3(COLSTATS_THREADS), lds, st, x, ld, D, T, offsets, seq_len, p.W,
                           (unsigned char*)workspace, stride);
    MG_CHECK_LAUNCH("mg_column_stats_f32");
    hipLaunchKernelGGL(colstats_merge_kernel, dim3((unsigned)mg_ceil_div(D, COLSTATS_MERGE_COLS), (unsigned)S), dim3(COLSTATS_THREADS), 0, st,
                       x, ld, B, T, offsets, seq_len, (const unsigned char*)workspace, stride, B * ch, ch, D, item_row, state);
    MG_CHECK_LAUNCH("mg_column_stats_f32");
    return MG_OK;
}

}  // extern "C"
