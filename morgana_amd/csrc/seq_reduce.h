// What the one-pass loss and statistics kernels share (ce, mdn, gv, vq, seqmean, segpool, clip, the masked losses of loss_norm):
// the valid-frame count of an utterance and the wave and workgroup reductions.  Each is a fixed order of operations on its arguments
// alone - "the same bits on every call" is kept here, once.  Workgroups are 256 threads (four waves of 64).  The header carries no
// floating-point pragma: it is compiled under whatever its includer has set at that point.  (The scan of the clamped lengths, which
// only the data-path kernels use, is in packed_rows.h.)
#pragma once

// n_b = min(max(seq_len[b], 0), T); without seq_len every frame is valid
__device__ __forceinline__ int64_t mg_valid_frames(const int64_t* __restrict__ seq_len, int b, int T) {
    int64_t n_b = seq_len ? seq_len[b] : (int64_t)T;
    if (n_b > T) n_b = T;
    if (n_b < 0) n_b = 0;
    return n_b;
}

__device__ __forceinline__ float mg_wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// (value, index) of the maximum, the LOWEST index among equal maxima (torch.argmax on NaN-free rows)
__device__ __forceinline__ void mg_argmax_merge(float& m, int& i, float om, int oi) {
    if (om > m || (om == m && oi < i)) {
        m = om;
        i = oi;
    }
}

__device__ __forceinline__ void mg_wave_argmax(float& m, int& i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float om = __shfl_xor(m, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        mg_argmax_merge(m, i, om, oi);
    }
}

// float64 sum over the workgroup, the same value in every thread: xor butterfly inside each wave, then the four wave sums in a
// fixed order.  red: 4 doubles of LDS.
__device__ __forceinline__ double mg_block_sum_f64(double v, double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// The body of a one-workgroup finish: sum_b ( sum_c partial[b, c] ) / n_b in float32, chunks in ascending order, utterances
// b, b + 256, ... per thread and then a halving tree over red (256 floats of LDS).  Thread 0 gets the tree's red[0]; the caller's
// last line rounds it its own way.  0 / 0 = NaN for an utterance without a valid frame (reference behaviour).
__device__ __forceinline__ float mg_utterance_mean_sum(const float* __restrict__ partial, const int64_t* __restrict__ seq_len, int B, int T,
                                                       int chunks, float* red) {
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        float s = 0.f;
        for (int c = 0; c < chunks; ++c) s += partial[(size_t)b * chunks + c];
        acc += s / (float)mg_valid_frames(seq_len, b, T);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    return red[0];
}
