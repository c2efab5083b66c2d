// Shifted float64 moments of the columns of a frame-major array, in one streaming pass: what colstats.hip (corpus statistics) and
// gv.hip (per-utterance variances) are built on.
//
//   * mg_chan_merge: Chan's update of a running (n, mean, M2 = sum (x - mean)^2) by another one.  Counts travel as doubles (exact
//     below 2^53); an empty side is skipped, never divided by, and two equal means leave the mean and M2 untouched (delta == 0: a
//     constant column keeps M2 == 0.0).
//   * mg_moments_acc: sums d = x - k and d^2 for at most MG_MOMENTS_FLUSH values, k being the first value it saw, turns them into
//     (n, mean - anchor, M2 = s2 - s1^2 / n) and folds that into its running triple; with MINMAX it also keeps min and max.
//   * mg_stream_moments: the pass.  The array is read in steps of W = R D elements (R whole frames); ENTRY e of a step (frame e / D
//     of the step, column e % D) has one accumulator, which takes its element of the steps first, first + stride, ... in ascending
//     order; results land in LDS by entry.
//   * mg_fold_step_frames: the halving tree in which the R entries of a column meet.
//
// All of it is a fixed order of float64 operations on the logical indices alone.  This header sets no floating-point pragma: it
// is compiled under what its includer has set where it includes it (gv.hip: contraction off; colstats.hip: the compiler's default),
// and each keeps its own rounding that way.  Workgroups are 256 threads.
#pragma once

#define MG_MOMENTS_THREADS 256
#define MG_MOMENTS_FLUSH 32        // values per shifted chunk (a multiple of 4)

__device__ __forceinline__ void mg_chan_merge(double& na, double& ma, double& Ma, double nb, double mb, double Mb) {
    if (nb == 0.0) return;
    if (na == 0.0) {
        na = nb;
        ma = mb;
        Ma = Mb;
        return;
    }
    const double n = na + nb;
    const double delta = mb - ma;
    ma = ma + delta * (nb / n);
    Ma = Ma + Mb + delta * delta * (na * nb / n);
    na = n;
}

template <bool MINMAX>
struct mg_moments_acc {
    double anchor;             // means are held as mean - anchor
    double k, s1, s2;          // the open chunk: shift, sum (x - k), sum (x - k)^2
    int cnt;
    double rn, rmean, rm2;     // the chunks folded so far
    float mn, mx;              // MINMAX only

    __device__ __forceinline__ void init(double anchor_) {
        anchor = anchor_;
        k = s1 = s2 = 0.0;
        cnt = 0;
        rn = rmean = rm2 = 0.0;
        if constexpr (MINMAX) {
            mn = __builtin_inff();
            mx = -__builtin_inff();
        }
    }

    __device__ __forceinline__ void add(float x) {
        const double v = (double)x;
        if (cnt == 0) k = v;
        const double d = v - k;
        s1 += d;
        s2 += d * d;
        cnt += 1;
        if constexpr (MINMAX) {
            mn = fminf(mn, x);
            mx = fmaxf(mx, x);
        }
    }

    __device__ __forceinline__ void flush() {
        if (cnt == 0) return;
        const double n = (double)cnt;
        const double mean = (k - anchor) + s1 / n;
        double m2 = s2 - s1 * s1 / n;
        if (m2 < 0.0) m2 = 0.0;                                  // rounding only; a NaN stays
        mg_chan_merge(rn, rmean, rm2, n, mean, m2);
        s1 = s2 = 0.0;
        cnt = 0;
    }
};

// `len` frames of D columns from `base` on, read in the steps first, first + stride, ... below ceil(len / R), W = R D elements each
// -> s_mean[e] = mean - anchor, s_m2[e] = M2, s_n[e] = count of entry e in [0, W).  IDX is the type steps and frames are counted in.
// anchor_of(col) gives a column's anchor; with MINMAX, minmax(col, mn, mx) takes the extremes of an entry (min / max ignore NaNs).
//   * VEC == 4: contiguous frames (stride_t == D, stride_d == 1), W % 4 == 0.  16-byte loads at 16-byte-aligned addresses whatever
//     the alignment of base: with base `pre` floats behind a boundary, register j of quad q holds entry 4 q - pre + j; the quads
//     across the ends of a step or of the array load their valid elements one by one.  Nothing outside [base, base + len D) is read.
//   * VEC == 1: any strides, one element per load; thread q + 256 p holds entry q + 256 p, so a unit stride_d still coalesces.
// Ends with a workgroup barrier: the entries are ready for mg_fold_step_frames.
template <int VEC, bool MINMAX, typename IDX, typename AnchorFn, typename MinMaxFn>
__device__ __forceinline__ void mg_stream_moments(const float* __restrict__ base, int64_t stride_t, int64_t stride_d, IDX len, int D, int R,
                                                  int W, IDX first, IDX stride, AnchorFn anchor_of, MinMaxFn minmax, double* s_mean,
                                                  double* s_m2, int* s_n) {
    const int tid = threadIdx.x;
    const int64_t E = (int64_t)len * D;                      // elements of the array (VEC == 4)
    const IDX NS = (len + R - 1) / R;                        // its steps
    if constexpr (VEC == 4) {
        const int pre = (int)(((uintptr_t)base >> 2) & 3u);  // elements between the 16-byte boundary below and base
        const int quads = W / 4 + (pre ? 1 : 0);
        for (int q = tid; q < quads; q += MG_MOMENTS_THREADS) {
            // element j of quad q of step m is element m W + ent0 + j, for 0 <= ent0 + j < W
            const int ent0 = 4 * q - pre;
            const bool inner = ent0 >= 0 && ent0 + 3 < W;
            mg_moments_acc<MINMAX> acc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {                     // (an entry outside [0, W) never gets an element: any column will do)
                const int ent = ent0 + j;
                acc[j].init(anchor_of(ent >= 0 && ent < W ? ent % D : 0));
            }
            const float* src = base + ent0;
            int since = 0;
            IDX m = first;
            if (inner) {
                const IDX mfull = E >= (int64_t)ent0 + 4 ? (IDX)((E - ent0 - 4) / W) + 1 : 0;      // steps whose whole quad is valid
                for (; m + 3 * stride < mfull; m += 4 * stride) {
                    f32x4 v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(src + (int64_t)(m + (IDX)u * stride) * W);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[j].add(v[u][j]);
                    }
                    since += 4;
                    if (since >= MG_MOMENTS_FLUSH) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[j].flush();
                        since = 0;
                    }
                }
                for (; m < mfull; m += stride) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(src + (int64_t)m * W);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j].add(v[j]);
                    if (++since >= MG_MOMENTS_FLUSH) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[j].flush();
                        since = 0;
                    }
                }
            }
            for (; m < NS; m += stride) {                     // quads across an end of the step or of the array: element by element
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ent = ent0 + j;
                    const int64_t e = (int64_t)m * W + ent;
                    if (ent >= 0 && ent < W && e < E) acc[j].add(base[e]);
                }
                if (++since >= MG_MOMENTS_FLUSH) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j].flush();
                    since = 0;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ent = ent0 + j;
                if (ent < 0 || ent >= W) continue;
                acc[j].flush();
                s_mean[ent] = acc[j].rmean;
                s_m2[ent] = acc[j].rm2;
                s_n[ent] = (int)acc[j].rn;
                if constexpr (MINMAX) minmax(ent % D, acc[j].mn, acc[j].mx);
            }
        }
    } else {
        for (int ent = tid; ent < W; ent += MG_MOMENTS_THREADS) {
            const int erow = ent / D, col = ent - erow * D;
            mg_moments_acc<MINMAX> acc;
            acc.init(anchor_of(col));
            const float* src = base + (int64_t)erow * stride_t + (int64_t)col * stride_d;
            const int64_t row_step = (int64_t)R * stride_t;
            const IDX mfull = len > erow ? (len - erow - 1) / R + 1 : 0;       // steps in which frame m R + erow exists
            int since = 0;
            IDX m = first;
            for (; m + 3 * stride < mfull; m += 4 * stride) {
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = src[(int64_t)(m + (IDX)u * stride) * row_step];
#pragma unroll
                for (int u = 0; u < 4; ++u) acc.add(v[u]);
                since += 4;
                if (since >= MG_MOMENTS_FLUSH) {
                    acc.flush();
                    since = 0;
                }
            }
            for (; m < mfull; m += stride) {
                acc.add(src[(int64_t)m * row_step]);
                if (++since >= MG_MOMENTS_FLUSH) {
                    acc.flush();
                    since = 0;
                }
            }
            acc.flush();
            s_mean[ent] = acc.rmean;
            s_m2[ent] = acc.rm2;
            s_n[ent] = (int)acc.rn;
            if constexpr (MINMAX) minmax(col, acc.mn, acc.mx);
        }
    }
    __syncthreads();
}

// Entries e and e + k D hold the same column: fold the upper half of the R frames of a step onto the lower, level by level.  After
// it entry d in [0, D) holds column d.  Ends with a workgroup barrier (R > 1).
__device__ __forceinline__ void mg_fold_step_frames(int R, int D, double* s_mean, double* s_m2, int* s_n) {
    const int tid = threadIdx.x;
    for (int rows = R; rows > 1;) {
        const int half = (rows + 1) >> 1;
        const int n_pairs = (rows - half) * D;
        for (int i = tid; i < n_pairs; i += MG_MOMENTS_THREADS) {
            const int o = i + half * D;
            double na = (double)s_n[i], ma = s_mean[i], Ma = s_m2[i];
            mg_chan_merge(na, ma, Ma, (double)s_n[o], s_mean[o], s_m2[o]);
            s_n[i] = (int)na;
            s_mean[i] = ma;
            s_m2[i] = Ma;
        }
        __syncthreads();
        rows = half;
    }
}
