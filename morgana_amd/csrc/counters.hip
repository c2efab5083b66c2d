// K30 - frame-level positional features ("counters") from durations: what the un-vendored tts_data_tools writes as the `counters` files
// the acoustic models of the reference read (models/RNN_SPSS.py:65).  d[b, p, s] are integer durations in frames, P phones of S
// sub-phone states each (S = 1: a phone-level alignment); a negative duration owns no frame, as in upsample.hip.  With
//
//   start[p, s] = the sum of all durations before (p, s) in (p, s) order         n_s = d[p, s]
//   n_p = sum_s d[p, s]                                                          i = t - start[p, s]
//   frame t lies in the one segment with start <= t < start + d                  j = t - start[p, 0]
//
// kind MG_COUNTERS_FULL (Merlin's subphone_feats='full'), 9 columns:
//   0 (i + 1) / n_s   1 (n_s - i) / n_s   2 n_s   3 s + 1   4 S - s   5 n_p   6 n_s / n_p   7 (n_p - j) / n_p   8 (j + 1) / n_p
// kind MG_COUNTERS_PHONE (Merlin's 'minimal_phoneme'), 3 columns: (j + 1) / n_p, (n_p - j) / n_p, n_p.
// Every quotient is one float64 division of the two integers, rounded once to float32: for lengths below 2^24 the correctly rounded
// float32 of the exact rational (double rounding through 53 bits is innocuous for a quotient of two 24-bit operands).  A frame's
// segment has d >= 1, so no denominator is zero.  Contraction is off; the NumPy restatement (data.frame_counters) has none.
//
// Mapping.  Grid (frame chunks, items).  A workgroup scans its item's P * S clamped durations into LDS (inclusive, int32, the scheme of
// block_scan_durations in upsample.hip, read through element strides) and then takes a contiguous range of the item's T * C OUTPUT
// ELEMENTS, thread = element: a wave stores 256 contiguous bytes per instruction whatever C is.  An element finds its segment by an
// upper-bound search in the scan (zero-length segments are stepped over); the C threads of a frame repeat the search, which is
// log2(P S) LDS reads each and cheaper than staging rows.  Every chunk of an item repeats the scan (P S * 8 bytes from L2).  Pad frames
// - past min(T, total, seq_len) - are exact zeros by the same launch.  No workspace, no atomics; an element is a function of its
// item's durations alone: the same bits on every call.
#include "common.h"

#pragma clang fp contract(off)

#define CNT_THREADS 256
#define CNT_MAX_SEGMENTS 12288    // MG_MAX_PHONES of upsample.hip: the scan lives in LDS, 4 bytes a segment + 1 KB
#define CNT_MAX_ITEM_BLOCKS 65535
#define CNT_CHUNK_ELEMS 768       // output elements of one workgroup by default, three per thread: measured, DESIGN.md 4.27

#include "item_norm.h"      // after the pragma: the normalised twin is mg_normalise_f32's float arithmetic on the rounded counter

__device__ __forceinline__ float cnt_ratio(int num, int den) { return (float)((double)num / (double)den); }

// Inclusive scan of the n = P_used * S clamped durations of one item into cum[0:n] (LDS, int32, saturating at INT32_MAX).
__device__ __forceinline__ void cnt_scan(const int64_t* __restrict__ dur, int64_t sp, int64_t ss, int S, int n, int* cum, int* scratch) {
    const int tid = threadIdx.x;
    const int per = (n + CNT_THREADS - 1) / CNT_THREADS;
    const int lo = min(tid * per, n), hi = min(lo + per, n);
    int64_t local = 0;
    for (int k = lo; k < hi; ++k) {
        const int64_t d = dur[(int64_t)(k / S) * sp + (int64_t)(k % S) * ss];
        local += d > 0 ? (d < INT32_MAX ? d : INT32_MAX) : 0;
    }
    scratch[tid] = (int)(local < INT32_MAX ? local : INT32_MAX);
    __syncthreads();
    for (int off = 1; off < CNT_THREADS; off <<= 1) {
        const int64_t v = tid >= off ? (int64_t)scratch[tid - off] : 0;
        __syncthreads();
        const int64_t w = (int64_t)scratch[tid] + v;
        scratch[tid] = (int)(w < INT32_MAX ? w : INT32_MAX);
        __syncthreads();
    }
    int64_t run = tid > 0 ? scratch[tid - 1] : 0;
    for (int k = lo; k < hi; ++k) {
        const int64_t d = dur[(int64_t)(k / S) * sp + (int64_t)(k % S) * ss];
        run += d > 0 ? (d < INT32_MAX ? d : INT32_MAX) : 0;
        if (run > INT32_MAX) run = INT32_MAX;
        cum[k] = (int)run;
    }
    __syncthreads();
}

template <int C>
__global__ __launch_bounds__(CNT_THREADS) void frame_counters_kernel(const int64_t* __restrict__ dur, int B, int P, int S, int64_t sb, int64_t sp,
                                                                     int64_t ss, const int64_t* __restrict__ n_phones,
                                                                     const int64_t* __restrict__ seq_len, int T, const float* __restrict__ p0,
                                                                     const float* __restrict__ p1, const int32_t* __restrict__ item_row,
                                                                     int n_rows, int norm_kind, float* __restrict__ raw_out,
                                                                     float* __restrict__ norm_out) {
    extern __shared__ __attribute__((aligned(16))) int cnt_smem[];
    int* scratch = cnt_smem;
    int* cum = cnt_smem + CNT_THREADS;
    const int tid = threadIdx.x;
    const int64_t elems = (int64_t)T * C;                                     // of one item
    // this workgroup's contiguous range of every item's elements (whole multiples of the workgroup, so that rows stay coalesced)
    int64_t per = (elems + gridDim.x - 1) / gridDim.x;
    per = (per + CNT_THREADS - 1) / CNT_THREADS * CNT_THREADS;
    const int64_t e_lo = min((int64_t)blockIdx.x * per, elems), e_hi = min(e_lo + per, elems);
    if (e_lo >= e_hi) return;                                                 // uniform for the workgroup
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        int used = P;                                                         // phones that count: the first n_phones[b]
        if (n_phones) {
            const int64_t np = n_phones[b];
            used = np < 0 ? 0 : (np < P ? (int)np : P);
        }
        const int n = used * S;                                               // <= CNT_MAX_SEGMENTS
        __syncthreads();                                                      // (the previous item's readers of cum are done)
        cnt_scan(dur + (int64_t)b * sb, sp, ss, S, n, cum, scratch);
        int64_t valid = n > 0 ? cum[n - 1] : 0;                               // frames of the item that are written as counters
        if (valid > T) valid = T;
        if (seq_len) {
            const int64_t len = seq_len[b];
            if (len < valid) valid = len < 0 ? 0 : len;
        }
        const float *q0 = p0, *q1 = p1;
        const bool row_ok = !norm_out || mg_item_param_rows(item_row, b, n_rows, C, q0, q1);      // false: NaN in the valid frames
        const int64_t base = (int64_t)b * elems;
        for (int64_t e = e_lo + tid; e < e_hi; e += CNT_THREADS) {
            const int t = (int)(e / C), c = (int)(e - (int64_t)t * C);
            float v = 0.f, w = 0.f;
            if (t < valid) {
                int lo = 0, hi = n - 1;                                       // the first k with cum[k] > t: t < valid <= cum[n - 1]
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (cum[mid] > t) hi = mid; else lo = mid + 1;
                }
                const int p = lo / S, s = lo - p * S;
                const int start = lo ? cum[lo - 1] : 0;
                const int p_start = p ? cum[p * S - 1] : 0;
                const int n_s = cum[lo] - start, n_p = cum[p * S + S - 1] - p_start;
                const int i = t - start, j = t - p_start;
                if (C == MG_COUNTERS_FULL_COLS) {
                    switch (c) {
                        case 0: v = cnt_ratio(i + 1, n_s); break;
                        case 1: v = cnt_ratio(n_s - i, n_s); break;
                        case 2: v = (float)n_s; break;
                        case 3: v = (float)(s + 1); break;
                        case 4: v = (float)(S - s); break;
                        case 5: v = (float)n_p; break;
                        case 6: v = cnt_ratio(n_s, n_p); break;
                        case 7: v = cnt_ratio(n_p - j, n_p); break;
                        default: v = cnt_ratio(j + 1, n_p); break;
                    }
                } else {
                    v = c == 0 ? cnt_ratio(j + 1, n_p) : (c == 1 ? cnt_ratio(n_p - j, n_p) : (float)n_p);
                }
                if (norm_out) w = row_ok ? mg_norm_forward(v, q0[c], q1[c], norm_kind) : __builtin_nanf("");
            }
            if (raw_out) raw_out[base + e] = v;
            if (norm_out) norm_out[base + e] = w;
        }
    }
}

extern "C" {

int mg_frame_counters_f32(const int64_t* dur, int B, int P, int S, int64_t stride_b, int64_t stride_p, int64_t stride_s, const int64_t* n_phones,
                          const int64_t* seq_len, int T, int counters_kind, const float* p0, const float* p1, const int32_t* item_row, int n_rows,
                          int norm_kind, float* raw_out, float* norm_out, int blocks_per_item, void* stream) {
    MG_CHECK_ARG(counters_kind == MG_COUNTERS_FULL || counters_kind == MG_COUNTERS_PHONE, "mg_frame_counters_f32: unknown kind %d", counters_kind);
    MG_CHECK_ARG(B >= 0 && P > 0 && S > 0 && T >= 0, "mg_frame_counters_f32: bad shape (B=%d P=%d S=%d T=%d)", B, P, S, T);
    MG_CHECK_ARG((int64_t)P * S <= CNT_MAX_SEGMENTS, "mg_frame_counters_f32: P=%d x S=%d exceeds %d segments per item", P, S, CNT_MAX_SEGMENTS);
    MG_CHECK_ARG(stride_b >= 0 && stride_p >= 0 && stride_s >= 0, "mg_frame_counters_f32: negative strides (%lld, %lld, %lld)",
                 (long long)stride_b, (long long)stride_p, (long long)stride_s);
    MG_CHECK_ARG(raw_out || norm_out, "mg_frame_counters_f32: no output requested");
    MG_CHECK_NORM_TWIN("mg_frame_counters_f32", norm_out, p0, p1, norm_kind);
    MG_CHECK_PARAM_ROWS("mg_frame_counters_f32", "n_rows", item_row, n_rows);
    MG_CHECK_ARG(blocks_per_item >= 0, "mg_frame_counters_f32: blocks_per_item=%d must not be negative (0: the library's choice)", blocks_per_item);
    const int C = counters_kind == MG_COUNTERS_FULL ? MG_COUNTERS_FULL_COLS : MG_COUNTERS_PHONE_COLS;
    MG_CHECK_ARG(B == 0 || T == 0 || (int64_t)T <= INT64_MAX / 4 / C / B, "mg_frame_counters_f32: B=%d x T=%d x C=%d overflow 64 bits", B, T, C);
    if (B == 0 || T == 0) return MG_OK;
    MG_CHECK_ARG(dur, "mg_frame_counters_f32: dur must not be NULL");
    MG_CHECK_ARG((((uintptr_t)raw_out | (uintptr_t)norm_out | (uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)item_row) & 3u) == 0 &&
                     (((uintptr_t)dur | (uintptr_t)n_phones | (uintptr_t)seq_len) & 7u) == 0,
                 "mg_frame_counters_f32: the outputs, the parameters and item_row must be 4-byte, dur, n_phones and seq_len 8-byte aligned");
    const int64_t elems = (int64_t)T * C;
    int64_t chunks = blocks_per_item > 0 ? blocks_per_item : mg_ceil_div(elems, CNT_CHUNK_ELEMS);
    const int64_t most = mg_ceil_div(elems, CNT_THREADS);                     // a chunk is at least one element per thread
    if (chunks > most) chunks = most;
    if (chunks > 65535) chunks = 65535;
    const unsigned items = (unsigned)(B < CNT_MAX_ITEM_BLOCKS ? B : CNT_MAX_ITEM_BLOCKS);
    const size_t lds = (size_t)(CNT_THREADS + (size_t)P * S) * sizeof(int);
    hipStream_t st = (hipStream_t)stream;
    if (C == MG_COUNTERS_FULL_COLS)
        hipLaunchKernelGGL(frame_counters_kernel<MG_COUNTERS_FULL_COLS>, dim3((unsigned)chunks, items), dim3(CNT_THREADS), lds, st, dur, B, P, S,
                           stride_b, stride_p, stride_s, n_phones, seq_len, T, p0, p1, item_row, n_rows, norm_kind, raw_out, norm_out);
    else
        hipLaunchKernelGGL(frame_counters_kernel<MG_COUNTERS_PHONE_COLS>, dim3((unsigned)chunks, items), dim3(CNT_THREADS), lds, st, dur, B, P, S,
                           stride_b, stride_p, stride_s, n_phones, seq_len, T, p0, p1, item_row, n_rows, norm_kind, raw_out, norm_out);
    MG_CHECK_LAUNCH("mg_frame_counters_f32");
    return MG_OK;
}

}  // extern "C"
