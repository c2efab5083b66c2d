// What the data-path kernels share (loss_norm's normalisers and pad passes, items_norm, colstats, f0, counters, durations, and - through
// packed_rows.h, which includes this header - unpad, deltas, vocoder, analysis): the normaliser arithmetic, the guarded parameter row
// of an item, the rows of an item and the search from a chunk of destination rows to its first item.  Each is a fixed order of
// operations on its arguments alone, so "the same bits as mg_normalise_f32" is kept here, once.  The header carries no floating-point
// pragma: it is compiled under whatever its includer has set at that point (f0.hip, counters.hip and durations.hip include it after
// their `fp contract(off)`; loss_norm.hip and items_norm.hip set nothing, and there the inverse kinds' `v * fac + off` is contracted
// into one fma).
#pragma once

// ---- the normaliser arithmetic (reference: morgana/data.py:533-538, 579-590)
// The divisor (forward kinds) or multiplier (inverse kinds) that `kind` derives from a column's two parameters: (mean, std_dev) or
// (min, max).  A forward-only caller passes MG_NORM_MVN or MG_NORM_MINMAX.
__device__ __forceinline__ float mg_norm_factor(float a, float b, int kind) {
    if (kind == MG_NORM_MVN) return b + 1e-8f;
    if (kind == MG_DENORM_MVN) return b;
    float scale = b - a;
    if (fabsf(scale) <= 1e-8f) scale = 1.f;
    return scale;
}

__device__ __forceinline__ bool mg_norm_inverse(int kind) { return kind == MG_DENORM_MVN || kind == MG_DENORM_MINMAX; }

// one element: off = the column's first parameter, fac = mg_norm_factor of the column
__device__ __forceinline__ float mg_norm_elem(float v, float off, float fac, bool inverse) {
    return inverse ? v * fac + off : (v - off) / fac;
}

// One value without a staged factor, kind MG_NORM_MVN or MG_NORM_MINMAX.  (deltas.hip keeps these operations in a function of its
// own: with any form of this one, hipcc allocates deltas_kernel<4, *> other registers than it had.)
__device__ __forceinline__ float mg_norm_forward(float v, float a, float b, int kind) {
    return mg_norm_elem(v, a, mg_norm_factor(a, b, kind), false);
}
// ... and any of the four kinds: a dispatch on the (uniform) kind with the kind a constant in every arm, the branches - and with them
// the registers - normalise_kernel had.
__device__ __forceinline__ float mg_norm_any(float v, float a, float b, int kind) {
    if (kind == MG_NORM_MVN) return mg_norm_elem(v, a, mg_norm_factor(a, b, MG_NORM_MVN), false);
    if (kind == MG_DENORM_MVN) return mg_norm_elem(v, a, mg_norm_factor(a, b, MG_DENORM_MVN), true);
    return mg_norm_elem(v, a, mg_norm_factor(a, b, MG_NORM_MINMAX), kind != MG_NORM_MINMAX);
}

// ---- the parameter row of an item
// item_row[b] if it names one of the S rows, else -1: an index outside [0, S) never becomes an index (the host cannot look at a
// device index without a synchronisation)
__device__ __forceinline__ int mg_item_row(const int32_t* __restrict__ item_row, int b, int S) {
    const int row = item_row[b];
    return row >= 0 && row < S ? row : -1;
}

// q0 / q1 (the vectors, or the (S, width) tables when item_row is given) moved to the row of item b.  false: the item names no row,
// q0 / q1 stay where they were and the caller writes NaN in the item's valid frames.
__device__ __forceinline__ bool mg_item_param_rows(const int32_t* __restrict__ item_row, int b, int S, int64_t width, const float*& q0,
                                                   const float*& q1) {
    if (!item_row) return true;
    const int row = mg_item_row(item_row, b, S);
    const int64_t at = row >= 0 ? (int64_t)row * width : 0;
    q0 += at;
    q1 += at;
    return row >= 0;
}

// ---- the rows of item b: its first row and its length, never negative.  Packed: offsets (B + 1); padded (B, T_in, D): seq_len (B)
// clamped to T_in.
__device__ __forceinline__ void mg_item_rows(const int64_t* __restrict__ offsets, const int64_t* __restrict__ seq_len, int64_t T_in, int b,
                                             int64_t& first, int64_t& len) {
    if (offsets) {
        first = offsets[b];
        len = offsets[b + 1] - first;
    } else {
        first = (int64_t)b * T_in;
        len = seq_len[b];
        if (len > T_in) len = T_in;
    }
    if (len < 0) len = 0;
}

// ---- from a chunk of destination positions that starts at c_lo to its first item: the smallest b whose positions end behind c_lo.
// first_of(b): the first destination position of item b, ascending in b, first_of(B) = all positions.  The caller walks on from b
// while first_of(b) lies below the chunk's end, cutting [first_of(b), first_of(b + 1)) to the chunk and stepping over empty items.
template <typename F>
__device__ __forceinline__ int mg_item_at(int B, int64_t c_lo, F first_of) {
    int b = 0, top = B;
    while (b < top) {
        const int mid = (b + top) >> 1;
        if (first_of(mid + 1) <= c_lo) b = mid + 1; else top = mid;
    }
    return b;
}
