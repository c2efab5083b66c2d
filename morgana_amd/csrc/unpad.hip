// Ragged pack of padded sequence features (reference: utils.detach_batched_seqs / batched_masked_select, morgana/utils.py:66-102,
// :147-166 - there a host slice per item of the whole padded tensor) and the both-voiced mask (utils.py:169-172).
//
// mg_unpad_rows: up to MG_UNPAD_MAX features [B, T_f, row_bytes_f] -> one byte buffer holding, per feature, the valid frames of
// every item back to back.  The launch moves bytes and knows no element type.  Grid (chunks, features): every workgroup scans the
// clamped lengths of its feature once (LDS), then walks fixed 16 KiB chunks of the feature's DESTINATION bytes; a chunk finds its
// first item by a binary search in the scanned lengths and copies the item pieces that fall inside it.  Source and destination of
// one piece are contiguous, so the piece is copied at the widest access their RELATIVE alignment allows (16, 4 or 1 bytes), with the
// few bytes in front of and behind the aligned body moved one by one.
#include "common.h"
#include "item_norm.h"
#include "packed_rows.h"

#define UNPAD_THREADS 256
#define UNPAD_CHUNK (UNPAD_THREADS * 16 * 4)        // destination bytes per chunk: four 16-byte trips per thread

struct UnpadBatch {
    int count;
    mg_unpad_desc d[MG_UNPAD_MAX];
};

struct NonzeroBatch {
    int count;
    const float* x[MG_ALL_NONZERO_MAX];
};

// n bytes src -> dst, all 256 threads of the workgroup; W = access width of the body (src and dst congruent modulo W)
template <int W, typename V>
__device__ __forceinline__ void unpad_copy_piece(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t n) {
    const int tid = threadIdx.x;
    int64_t head = (int64_t)((W - ((uintptr_t)dst & (W - 1))) & (W - 1));
    if (head > n) head = n;
    if (tid < head) dst[tid] = src[tid];
    const int64_t body = (n - head) / W;
    const V* s = (const V*)(src + head);
    V* d = (V*)(dst + head);
    for (int64_t i = tid; i < body; i += UNPAD_THREADS) d[i] = s[i];
    const int64_t done = head + body * W;
    if (tid < n - done) dst[done + tid] = src[done + tid];
}

__global__ __launch_bounds__(UNPAD_THREADS) void unpad_rows_kernel(UnpadBatch batch, const int64_t* __restrict__ seq_len, int B,
                                                                  uint8_t* __restrict__ dst) {
    __shared__ int64_t s_off[MG_UNPAD_MAX_ITEMS + 1];      // first packed row of item b; s_off[B] = all rows
    __shared__ int64_t s_part[UNPAD_THREADS];
    const mg_unpad_desc& f = batch.d[blockIdx.y];
    const int64_t T = f.T, rb = f.row_bytes;
    if (f.block_bytes < rb || T == 0) return;              // nothing of this feature moves (uniform for the workgroup)
    if ((int64_t)blockIdx.x * UNPAD_CHUNK >= f.block_bytes) return;
    const int tid = threadIdx.x;

    mg_clamped_length_scan(seq_len, B, T, s_off, s_part);

    // rows that do not fit the block are dropped: nothing is written at or beyond dst_offset + block_bytes
    int64_t rows = s_off[B];
    if (rows > f.block_bytes / rb) rows = f.block_bytes / rb;
    const int64_t n_bytes = rows * rb;
    const uint8_t* src = (const uint8_t*)f.src;
    uint8_t* out = dst + f.dst_offset;
    for (int64_t c_lo = (int64_t)blockIdx.x * UNPAD_CHUNK; c_lo < n_bytes; c_lo += (int64_t)gridDim.x * UNPAD_CHUNK) {
        const int64_t c_hi = c_lo + UNPAD_CHUNK < n_bytes ? c_lo + UNPAD_CHUNK : n_bytes;
        // the item that holds byte c_lo: the largest b with s_off[b] * rb <= c_lo < s_off[b + 1] * rb
        int b = mg_item_at(B, c_lo, [&](int i) { return s_off[i] * rb; });
        for (; b < B; ++b) {
            const int64_t i_lo = s_off[b] * rb, i_hi = s_off[b + 1] * rb;
            if (i_lo >= c_hi) break;
            const int64_t p_lo = i_lo > c_lo ? i_lo : c_lo, p_hi = i_hi < c_hi ? i_hi : c_hi;
            if (p_hi <= p_lo) continue;                    // an empty item
            const uint8_t* s = src + (int64_t)b * T * rb + (p_lo - i_lo);
            uint8_t* d = out + p_lo;
            const uintptr_t rel = (uintptr_t)s ^ (uintptr_t)d;
            if ((rel & 15) == 0) unpad_copy_piece<16, uint4>(s, d, p_hi - p_lo);
            else if ((rel & 3) == 0) unpad_copy_piece<4, uint32_t>(s, d, p_hi - p_lo);
            else unpad_copy_piece<1, uint8_t>(s, d, p_hi - p_lo);
        }
    }
}

// out[i] = all_k (x_k[i] != 0): NaN != 0 holds, -0.0 != 0 does not (~torch.eq(x, 0.)).  Output encoding as sequence_mask_kernel.
__global__ __launch_bounds__(256) void all_nonzero_kernel(NonzeroBatch batch, int64_t n, void* __restrict__ out, int elem_size, int as_float) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        bool on = true;
        for (int k = 0; k < batch.count; ++k) on = on && (batch.x[k][i] != 0.f);
        if (elem_size == 1) ((uint8_t*)out)[i] = on ? 1 : 0;
        else if (elem_size == 4) {
            if (as_float) ((float*)out)[i] = on ? 1.f : 0.f; else ((int32_t*)out)[i] = on ? 1 : 0;
        } else {
            if (as_float) ((double*)out)[i] = on ? 1.0 : 0.0; else ((int64_t*)out)[i] = on ? 1 : 0;
        }
    }
}

// four elements per thread: one 16-byte load per input, one store of 4 / 16 / 32 bytes (all pointers 16-byte aligned, n % 4 == 0)
__global__ __launch_bounds__(256) void all_nonzero_x4_kernel(NonzeroBatch batch, int64_t n4, void* __restrict__ out, int elem_size, int as_float) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        bool on[4] = {true, true, true, true};
        for (int k = 0; k < batch.count; ++k) {
            const f32x4 v = ((const f32x4*)batch.x[k])[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) on[j] = on[j] && (v[j] != 0.f);
        }
        if (elem_size == 1) {
            ((uint32_t*)out)[i] = (on[0] ? 1u : 0u) | (on[1] ? 0x100u : 0u) | (on[2] ? 0x10000u : 0u) | (on[3] ? 0x1000000u : 0u);
        } else if (elem_size == 4) {
            if (as_float) {
                f32x4 r = {on[0] ? 1.f : 0.f, on[1] ? 1.f : 0.f, on[2] ? 1.f : 0.f, on[3] ? 1.f : 0.f};
                ((f32x4*)out)[i] = r;
            } else {
                int4 r = make_int4(on[0] ? 1 : 0, on[1] ? 1 : 0, on[2] ? 1 : 0, on[3] ? 1 : 0);
                ((int4*)out)[i] = r;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (as_float) ((double*)out)[4 * i + j] = on[j] ? 1.0 : 0.0; else ((int64_t*)out)[4 * i + j] = on[j] ? 1 : 0;
            }
        }
    }
}

extern "C" {

int mg_unpad_rows(const mg_unpad_desc* descs, int count, const int64_t* seq_len, int B, void* dst, int64_t dst_bytes, void* stream) {
    MG_CHECK_ARG(descs && count >= 1 && count <= MG_UNPAD_MAX, "mg_unpad_rows: count %d not in 1..%d", count, MG_UNPAD_MAX);
    MG_CHECK_ARG(B >= 0 && B <= MG_UNPAD_MAX_ITEMS, "mg_unpad_rows: B=%d not in 0..%d", B, MG_UNPAD_MAX_ITEMS);
    MG_CHECK_ARG(dst_bytes >= 0, "mg_unpad_rows: dst_bytes=%lld is negative", (long long)dst_bytes);
    UnpadBatch batch;
    batch.count = count;
    int64_t most = 0;
    for (int i = 0; i < count; ++i) {
        const mg_unpad_desc& d = descs[i];
        MG_CHECK_ARG(d.row_bytes > 0, "mg_unpad_rows: descriptor %d: row_bytes=%lld must be positive", i, (long long)d.row_bytes);
        MG_CHECK_ARG(d.T >= 0, "mg_unpad_rows: descriptor %d: T=%lld is negative", i, (long long)d.T);
        MG_CHECK_ARG(d.T == 0 || B == 0 || d.row_bytes <= INT64_MAX / d.T / B,
                     "mg_unpad_rows: descriptor %d: B=%d x T=%lld x row_bytes=%lld overflows 64 bits", i, B, (long long)d.T, (long long)d.row_bytes);
        MG_CHECK_ARG(d.dst_offset >= 0 && d.dst_offset % 16 == 0, "mg_unpad_rows: descriptor %d: dst_offset=%lld must be a non-negative multiple of 16",
                     i, (long long)d.dst_offset);
        MG_CHECK_ARG(d.block_bytes >= 0 && d.block_bytes <= dst_bytes && d.dst_offset <= dst_bytes - d.block_bytes,
                     "mg_unpad_rows: descriptor %d: block_bytes=%lld at dst_offset=%lld does not lie inside dst_bytes=%lld", i,
                     (long long)d.block_bytes, (long long)d.dst_offset, (long long)dst_bytes);
        for (int j = 0; j < i; ++j) {
            const mg_unpad_desc& e = descs[j];
            MG_CHECK_ARG(d.block_bytes == 0 || e.block_bytes == 0 || d.dst_offset >= e.dst_offset + e.block_bytes ||
                             e.dst_offset >= d.dst_offset + d.block_bytes,
                         "mg_unpad_rows: the blocks of descriptors %d and %d overlap", j, i);
        }
        const bool moves = B > 0 && d.T > 0 && d.block_bytes >= d.row_bytes;
        MG_CHECK_ARG(!moves || d.src, "mg_unpad_rows: descriptor %d: src is NULL", i);
        MG_CHECK_ARG(!moves || dst, "mg_unpad_rows: dst is NULL");
        MG_CHECK_ARG(!moves || seq_len, "mg_unpad_rows: seq_len is NULL");
        if (moves && d.block_bytes > most) most = d.block_bytes;
        batch.d[i] = d;
    }
    if (most == 0) return MG_OK;
    int64_t chunks = mg_ceil_div(most, UNPAD_CHUNK);
    if (chunks > 4096) chunks = 4096;
    hipLaunchKernelGGL(unpad_rows_kernel, dim3((unsigned)chunks, count), dim3(UNPAD_THREADS), 0, (hipStream_t)stream, batch, seq_len, B,
                       (uint8_t*)dst);
    MG_CHECK_LAUNCH("mg_unpad_rows");
    return MG_OK;
}

int mg_all_nonzero_f32(const float* const* xs, int count, int64_t n, void* out, int elem_size, int as_float, void* stream) {
    MG_CHECK_ARG(xs && count >= 1 && count <= MG_ALL_NONZERO_MAX, "mg_all_nonzero_f32: count %d not in 1..%d", count, MG_ALL_NONZERO_MAX);
    MG_CHECK_ARG(n >= 0, "mg_all_nonzero_f32: n=%lld is negative", (long long)n);
    MG_CHECK_ARG(elem_size == 1 || elem_size == 4 || elem_size == 8, "mg_all_nonzero_f32: elem_size %d not in {1,4,8}", elem_size);
    if (n == 0) return MG_OK;
    MG_CHECK_ARG(out, "mg_all_nonzero_f32: out is NULL");
    NonzeroBatch batch;
    batch.count = count;
    uintptr_t bits = (uintptr_t)out;
    for (int k = 0; k < count; ++k) {
        MG_CHECK_ARG(xs[k], "mg_all_nonzero_f32: input %d is NULL", k);
        batch.x[k] = xs[k];
        bits |= (uintptr_t)xs[k];
    }
    if (n % 4 == 0 && bits % 16 == 0) {
        int64_t blocks = mg_ceil_div(n / 4, 256);
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(all_nonzero_x4_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, batch, n / 4, out, elem_size, as_float);
    } else {
        int64_t blocks = mg_ceil_div(n, 256);
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(all_nonzero_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, batch, n, out, elem_size, as_float);
    }
    MG_CHECK_LAUNCH("mg_all_nonzero_f32");
    return MG_OK;
}

}  // extern "C"
