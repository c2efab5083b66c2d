// What the kernels with PACKED DESTINATION ROWS share (unpad, deltas, vocoder, analysis): the scan of a padded input's clamped lengths
// to the items' first packed rows, and - vocoder and analysis - the way from a packed row back to its source frame.  Each is a fixed
// order of operations on its arguments alone.  Workgroups are 256 threads.  The header carries no floating-point pragma: it is
// compiled under whatever its includer has set at that point.
#pragma once

#include "item_norm.h"

// Exclusive scan of len_b = min(max(seq_len[b], 0), T) over the workgroup: s_off[b] = sum of the lengths before item b,
// s_off[B] = all of them.  Thread t owns items [t per, (t + 1) per).  s_off: B + 1, s_part: 256 entries of LDS.
__device__ __forceinline__ void mg_clamped_length_scan(const int64_t* __restrict__ seq_len, int B, int64_t T, int64_t* s_off,
                                                       int64_t* s_part) {
    const int tid = threadIdx.x;
    const int per = (B + 255) / 256;
    const int lo = tid * per < B ? tid * per : B, hi = lo + per < B ? lo + per : B;
    int64_t sum = 0;
    for (int b = lo; b < hi; ++b) {
        const int64_t len = seq_len[b];
        sum += len < 0 ? 0 : len > T ? T : len;
    }
    s_part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int64_t v = tid >= off ? s_part[tid - off] : 0;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    int64_t run = s_part[tid] - sum;
    for (int b = lo; b < hi; ++b) {
        const int64_t len = seq_len[b];
        s_off[b] = run;
        run += len < 0 ? 0 : len > T ? T : len;
    }
    if (tid == 255) s_off[B] = s_part[tid];
    __syncthreads();
}

// Dynamic LDS of a launch whose workgroups of `threads` scan a padded input (offsets NULL): [B + 1] first rows, [threads] partials.
// A packed input brings its first rows along and needs none.
static inline size_t mg_packed_scan_bytes(const int64_t* offsets_or_null, int B, int threads) {
    return offsets_or_null ? 0 : ((size_t)B + 1 + threads) * sizeof(int64_t);
}

// first packed row of item b (b == B: all rows)
__device__ __forceinline__ int64_t mg_packed_first_row(int b, const int64_t* __restrict__ offsets, const int64_t* s_cum) {
    return offsets ? offsets[b] : s_cum[b];
}

// the source frame (row of the input as the item's layout counts it) of packed row r, or -1: no item holds it
__device__ __forceinline__ int64_t mg_packed_source_row(int64_t r, int64_t rows_end, int B, const int64_t* __restrict__ offsets,
                                                        const int64_t* __restrict__ seq_len, int64_t T_in, const int64_t* s_cum) {
    if (r >= rows_end) return -1;
    if (offsets) return r >= offsets[0] ? r : -1;              // packed rows are their own source: [offsets[0], offsets[B]), no search
    const auto first_of = [&](int b) { return mg_packed_first_row(b, offsets, s_cum); };
    const int b = mg_item_at(B, r, first_of);
    if (b >= B) return -1;
    int64_t first, len;
    mg_item_rows(offsets, seq_len, T_in, b, first, len);
    const int64_t t = r - first_of(b);
    return t >= 0 && t < len ? first + t : -1;
}

// The prologue of a tiled kernel: the scan of a padded input, then the end of the rows any tile has to look at.
__device__ __forceinline__ int64_t mg_packed_rows_end(const int64_t* __restrict__ offsets, const int64_t* __restrict__ seq_len, int64_t T_in,
                                                      int B, int64_t packed_rows, int64_t* s_cum) {
    if (!offsets) mg_clamped_length_scan(seq_len, B, T_in, s_cum, s_cum + B + 1);
    const int64_t all = mg_packed_first_row(B, offsets, s_cum);
    return all < packed_rows ? all : packed_rows;
}
