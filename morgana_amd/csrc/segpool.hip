// K27 - ragged segment pooling and its backward: utils.pool_segments, the way back from frame rate to segment rate.
//
//   out[b, s, f] = pool_{t in [start_s, start_s + m_s)} x[b, t, f],   start_s = sum_{j < s} max(len_j, 0),
//   m_s = max(min(start_s + max(len_s, 0), n_b) - min(start_s, n_b), 0),   n_b = min(max(seq_len[b], 0), T)
//
// pool = sum | mean | max | min; m_s == 0 gives +0 (and frame index -1).  A frame outside every range is never read.  The reference
// ships split_to_segments (morgana/utils.py:231-285) and leaves the reduction over its zero-padded (B, S, L_max, F) block to the
// user; here one pass reads the valid frames once and the block is never written.  No host read, no atomics, no workspace.
//
// Order of operations.  A segment is cut, from ITS OWN first frame, into chunks of POOL_CHUNK consecutive frames.  One chunk is
// reduced front to back (float64 adds starting from +0; or (value, frame) pairs, an earlier frame winning every tie), and the chunk
// results of a segment are merged in ascending chunk order, ((c0 + c1) + c2) + ...  The float64 total is rounded to float32 once
// ('mean': divided by m_s in float64 first).  This order is a function of m_s and the position inside the segment alone: it does
// not depend on b, s, B, S, T, the strides, the launch geometry or which of the two load paths ran.
//
// Work mapping (one kernel, three regimes).  A workgroup of 256 threads takes `sg` consecutive segments of one utterance and one
// column tile; its threads form LC slots of LF lanes, LF * LC == 256.  The lanes of a slot run along F (a 16-byte load per lane
// where base and strides allow, else one float), the slots take the workgroup's chunks - ALL chunks of its segments, numbered
// through by a scan of the chunk counts in LDS - LC at a time; after each round the slots' results meet in LDS and the first slot
// of every segment in the round merges that segment's run in ascending order, a segment that crosses the round's end leaving a
// carry for the next round.
//   * wide rows, short segments (F >= 256): LF = 64, a wave reads whole 1 KiB (16-byte path) or 256-byte row pieces, its four
//     waves take four chunks at a time; 16 segments per workgroup, so a 64 x 80-segment batch is 640 workgroups per column tile.
//   * narrow rows (F = 1..4): LF = 1, 2 or 4, so 64 to 256 slots: the lanes run over (chunk, column) pairs, all of them busy while
//     the workgroup has that many chunks left.
//   * one long segment (S == 1): the same loop - LC chunks of the one segment are in flight per round and the longest dependent
//     chain is POOL_CHUNK adds per round plus one merge add per chunk, not m adds.
// LF is the smallest power of two that covers the row (in 16-byte or 4-byte lanes), at most 64, so nothing changes abruptly
// between these.
// Every workgroup sums the lengths in front of its first segment itself: about S^2 / (2 sg) loads of seg_lens per utterance, nothing
// at 80 phones, 4.7 million at the limit of POOL_MAX_S segments (a scan once per utterance would be the form for such tables).
//
// Backward: one launch, grid (frame tiles, B), writes every element of the dense (B, T, F) gradient exactly once.  Every workgroup
// scans the utterance's lengths in LDS (as K1 does), the first threads binary-search the segment of the tile's frames, then all
// threads stream the tile: g (sum), (float)((double)g / m) (mean), g where the saved frame index equals t (max / min), +0 on
// frames outside every range.
#include "common.h"
#include "seq_reduce.h"

#pragma clang fp contract(off)

#define POOL_THREADS 256
#define POOL_CHUNK 32             // frames of one segment reduced front to back by one slot
#define POOL_MAX_SEGS 256         // segments per forward workgroup, at most
#define POOL_MAX_S 12288          // segments per utterance (MG_MAX_PHONES of upsample.hip: the backward's scan lives in LDS)
#define POOL_BWD_FRAMES 256       // frames per backward workgroup, at most
#define POOL_BWD_ELEMS 8192       // elements per backward workgroup, about

__device__ __forceinline__ int64_t pool_clamp_len(int64_t len, int T) { return len < 0 ? 0 : len > T ? T : len; }

// Inclusive scan of v (an integer: no order to keep) over the 256 threads: a shuffle scan inside each wave, then the totals of the
// waves in front.  s_wave: 4 entries of LDS that hold the four wave totals until the next call; barriers in front and behind.
__device__ __forceinline__ int64_t pool_block_scan(int64_t v, int64_t* s_wave) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    __syncthreads();
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    for (int w = 0; w < wave; ++w) v += s_wave[w];
    return v;
}
__device__ __forceinline__ int64_t pool_scan_total(const int64_t* s_wave) { return (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]); }

// (value, frame) of an extremum as one 64-bit word for LDS
__device__ __forceinline__ unsigned long long pool_pack(float v, int t) {
    return ((unsigned long long)(unsigned)t << 32) | (unsigned long long)__float_as_uint(v);
}
__device__ __forceinline__ float pool_value(unsigned long long w) { return __uint_as_float((unsigned)w); }
__device__ __forceinline__ int pool_frame(unsigned long long w) { return (int)(unsigned)(w >> 32); }

// a: the earlier frames, b: the later ones.  The first NaN wins; otherwise a strictly better later value replaces the earlier one,
// so equal values (-0 against +0 among them) keep the lowest frame.
template <bool IS_MAX>
__device__ __forceinline__ void pool_ext_merge(float& av, int& at, float bv, int bt) {
    const bool better = IS_MAX ? bv > av : bv < av;
    if (!(av != av) && ((bv != bv) || better)) {
        av = bv;
        at = bt;
    }
}

template <bool VEC, bool EXT, bool IS_MAX>
__global__ __launch_bounds__(POOL_THREADS) void segment_pool_kernel(const float* __restrict__ x, int64_t stride_b, int64_t stride_t,
                                                                    int64_t stride_f, const int64_t* __restrict__ seg_lens,
                                                                    const int64_t* __restrict__ seq_len, int S, int T, int F, int mean,
                                                                    int lf_shift, int sg, float* __restrict__ out, int32_t* __restrict__ arg) {
    constexpr int NV = VEC ? 4 : 1;
    __shared__ int64_t s_part[4];
    __shared__ int s_start[POOL_MAX_SEGS];               // first frame, frame count and inclusive chunk count of the workgroup's segments
    __shared__ int s_m[POOL_MAX_SEGS];
    __shared__ int s_cch[POOL_MAX_SEGS];
    __shared__ int s_seg[POOL_THREADS];                  // the local segment of slot j's chunk in this round, -1 for none
    __shared__ unsigned long long s_val[POOL_THREADS * NV];   // the slots' chunk results: float64 sums or (value, frame) words
    __shared__ unsigned long long s_carry[64 * NV];      // the merged front of the segment that crosses the round's end, per column
    const int tid = threadIdx.x, b = blockIdx.y;
    const int s_lo = blockIdx.x * sg;
    const int n_seg = S - s_lo < sg ? S - s_lo : sg;
    const int64_t n_b = mg_valid_frames(seq_len, b, T);
    const int64_t* lens = seg_lens + (int64_t)b * S;

    // frames in front of the workgroup's first segment, then the scan of its own lengths
    int64_t before = 0;
    for (int s = tid; s < s_lo; s += POOL_THREADS) before += pool_clamp_len(lens[s], T);
    pool_block_scan(before, s_part);
    before = pool_scan_total(s_part);
    const int64_t len = tid < n_seg ? pool_clamp_len(lens[s_lo + tid], T) : 0;
    const int64_t end = before + pool_block_scan(len, s_part);
    const int64_t lo = end - len < n_b ? end - len : n_b, hi = end < n_b ? end : n_b;
    const int m_own = (int)(hi - lo);
    const int64_t cch = pool_block_scan((m_own + POOL_CHUNK - 1) / POOL_CHUNK, s_part);
    if (tid < n_seg) {
        s_start[tid] = (int)lo;
        s_m[tid] = m_own;
        s_cch[tid] = (int)cch;
    }
    __syncthreads();
    const int n_chunks = s_cch[n_seg - 1];

    const int LF = 1 << lf_shift, LC = POOL_THREADS >> lf_shift;
    const int tile_shift = lf_shift + (VEC ? 2 : 0);
    const int64_t col0 = (int64_t)blockIdx.z << tile_shift;
    const int64_t out0 = ((int64_t)b * S + s_lo) * F;

    // empty segments: +0 and frame -1
    for (int e = tid; e < (n_seg << tile_shift); e += POOL_THREADS) {
        const int i = e >> tile_shift;
        const int64_t c = col0 + (e & ((1 << tile_shift) - 1));
        if (c < F && s_m[i] == 0) {
            out[out0 + (int64_t)i * F + c] = 0.f;
            if (EXT) arg[out0 + (int64_t)i * F + c] = -1;
        }
    }

    const int j = tid >> lf_shift, l = tid & (LF - 1);
    const int64_t col = col0 + (int64_t)l * NV;
    const bool live = col < F;                            // VEC: F % 4 == 0, so the lane's four columns are inside together
    const float* xb = x + (int64_t)b * stride_b + col * stride_f;
    for (int k0 = 0; k0 < n_chunks; k0 += LC) {
        const int k = k0 + j;
        int i = -1, c = 0;
        if (k < n_chunks) {                               // the segment of chunk k: the first i with s_cch[i] > k
            int a = 0, z = n_seg - 1;
            while (a < z) {
                const int mid = (a + z) >> 1;
                if (s_cch[mid] > k) z = mid; else a = mid + 1;
            }
            i = a;
            c = k - (i ? s_cch[i - 1] : 0);
        }
        if (l == 0) s_seg[j] = i;
        // Slot 0 continues the segment that crossed the last round's end: its carry is taken NOW, in front of the round's first
        // barrier.  It was written before the barrier that ended the last round, and the slot that leaves this round's carry (the
        // first slot of a later segment, possibly another wave) writes the same entry only behind the barrier below.
        const bool continues = i >= 0 && live && c > 0 && j == 0;
        unsigned long long carried[NV];
        if (continues) {
#pragma unroll
            for (int q = 0; q < NV; ++q) carried[q] = s_carry[l * NV + q];
        }
        double acc[NV];
        float ev[NV];
        int et[NV];
        if (i >= 0 && live) {
            const int ta = s_start[i] + c * POOL_CHUNK;
            const int seg_end = s_start[i] + s_m[i];
            const int tb = ta + POOL_CHUNK < seg_end ? ta + POOL_CHUNK : seg_end;
            const float* p = xb + (int64_t)ta * stride_t;
            if (EXT) {
                if (VEC) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
                    for (int q = 0; q < NV; ++q) { ev[q] = v[q]; et[q] = ta; }
                } else {
                    ev[0] = *p;
                    et[0] = ta;
                }
                p += stride_t;
#pragma unroll 4
                for (int t = ta + 1; t < tb; ++t, p += stride_t) {
                    if (VEC) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
                        for (int q = 0; q < NV; ++q) pool_ext_merge<IS_MAX>(ev[q], et[q], v[q], t);
                    } else {
                        pool_ext_merge<IS_MAX>(ev[0], et[0], *p, t);
                    }
                }
#pragma unroll
                for (int q = 0; q < NV; ++q) s_val[tid * NV + q] = pool_pack(ev[q], et[q]);
            } else {
#pragma unroll
                for (int q = 0; q < NV; ++q) acc[q] = 0.0;
#pragma unroll 4
                for (int t = ta; t < tb; ++t, p += stride_t) {
                    if (VEC) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
                        for (int q = 0; q < NV; ++q) acc[q] += (double)v[q];
                    } else {
                        acc[0] += (double)*p;
                    }
                }
#pragma unroll
                for (int q = 0; q < NV; ++q) s_val[tid * NV + q] = (unsigned long long)__double_as_longlong(acc[q]);
            }
        }
        __syncthreads();
        // the first slot of a segment in this round merges the segment's run; c > 0 there means j == 0: the run continues a carry
        if (i >= 0 && live && (j == 0 || c == 0)) {
            if (continues) {
#pragma unroll
                for (int q = 0; q < NV; ++q) {
                    const unsigned long long w = carried[q];
                    if (EXT) {
                        const float bv = ev[q];
                        const int bt = et[q];
                        ev[q] = pool_value(w);
                        et[q] = pool_frame(w);
                        pool_ext_merge<IS_MAX>(ev[q], et[q], bv, bt);
                    } else {
                        acc[q] = __longlong_as_double((long long)w) + acc[q];
                    }
                }
            }
            int jj = j + 1;
            for (; jj < LC && s_seg[jj] == i; ++jj) {
#pragma unroll
                for (int q = 0; q < NV; ++q) {
                    const unsigned long long w = s_val[((jj << lf_shift) + l) * NV + q];
                    if (EXT) pool_ext_merge<IS_MAX>(ev[q], et[q], pool_value(w), pool_frame(w));
                    else acc[q] += __longlong_as_double((long long)w);
                }
            }
            const int m = s_m[i];
            if (c + (jj - j) == (m + POOL_CHUNK - 1) / POOL_CHUNK) {      // the run reached the segment's last chunk
                const int64_t o = out0 + (int64_t)i * F + col;
#pragma unroll
                for (int q = 0; q < NV; ++q) {
                    if (EXT) {
                        out[o + q] = ev[q];
                        arg[o + q] = et[q];
                    } else {
                        out[o + q] = mean ? (float)(acc[q] / (double)m) : (float)acc[q];
                    }
                }
            } else {
#pragma unroll
                for (int q = 0; q < NV; ++q)
                    s_carry[l * NV + q] = EXT ? pool_pack(ev[q], et[q]) : (unsigned long long)__double_as_longlong(acc[q]);
            }
        }
        __syncthreads();
    }
}

// grid (frame tiles, B); dynamic LDS: S ints (the inclusive scan of the clamped lengths, saturated at T)
template <bool VEC>
__global__ __launch_bounds__(POOL_THREADS) void segment_pool_bwd_kernel(const float* __restrict__ go, const int64_t* __restrict__ seg_lens,
                                                                        const int64_t* __restrict__ seq_len, const int32_t* __restrict__ arg,
                                                                        int S, int T, int F, int mode, int tile, float* __restrict__ grad) {
    extern __shared__ __attribute__((aligned(16))) int s_cum[];
    __shared__ int64_t s_part[4];
    __shared__ int s_seg[POOL_BWD_FRAMES];               // segment of the tile's frames (-1: outside every range) and its frame count
    __shared__ int s_m[POOL_BWD_FRAMES];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t n_b = mg_valid_frames(seq_len, b, T);
    const int64_t* lens = seg_lens + (int64_t)b * S;
    const int per = (S + POOL_THREADS - 1) / POOL_THREADS;
    const int p_lo = tid * per < S ? tid * per : S, p_hi = p_lo + per < S ? p_lo + per : S;
    int64_t own = 0;
    for (int s = p_lo; s < p_hi; ++s) own += pool_clamp_len(lens[s], T);
    int64_t run = pool_block_scan(own, s_part) - own;
    for (int s = p_lo; s < p_hi; ++s) {
        run += pool_clamp_len(lens[s], T);
        s_cum[s] = (int)(run < T ? run : T);
    }
    __syncthreads();

    const int t0 = blockIdx.x * tile;
    const int nt = T - t0 < tile ? T - t0 : tile;
    if (tid < nt) {
        const int t = t0 + tid;
        int seg = -1, m = 0;
        if (t < n_b && S > 0 && t < s_cum[S - 1]) {       // the first s with s_cum[s] > t
            int a = 0, z = S - 1;
            while (a < z) {
                const int mid = (a + z) >> 1;
                if (s_cum[mid] > t) z = mid; else a = mid + 1;
            }
            seg = a;
            const int64_t start = a ? s_cum[a - 1] : 0, end = s_cum[a] < n_b ? s_cum[a] : n_b;
            m = (int)(end - start);
        }
        s_seg[tid] = seg;
        s_m[tid] = m;
    }
    __syncthreads();

    float* gp = grad + ((int64_t)b * T + t0) * F;
    const int64_t go0 = (int64_t)b * S * F;
    constexpr int NV = VEC ? 4 : 1;
    const int n = nt * F / NV;                            // VEC: F % 4 == 0
    for (int e = tid; e < n; e += POOL_THREADS) {
        const int i = (e * NV) / F, f = e * NV - i * F;
        const int seg = s_seg[i];
        float v[NV];
#pragma unroll
        for (int q = 0; q < NV; ++q) v[q] = 0.f;
        if (seg >= 0) {
            const int64_t o = go0 + (int64_t)seg * F + f;
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const float g = go[o + q];
                if (mode == MG_POOL_SUM) v[q] = g;
                else if (mode == MG_POOL_MEAN) v[q] = (float)((double)g / (double)s_m[i]);
                else v[q] = arg[o + q] == t0 + i ? g : 0.f;
            }
        }
        if (VEC) {
            const f32x4 w = {v[0], v[1], v[2], v[3]};
            reinterpret_cast<f32x4*>(gp)[e] = w;
        } else {
            gp[e] = v[0];
        }
    }
}

static bool pool_mode_known(int mode) { return mode >= MG_POOL_SUM && mode <= MG_POOL_MIN; }

extern "C" {

int mg_segment_pool_chunk(void) { return POOL_CHUNK; }

int mg_segment_pool_f32(const float* x, int64_t stride_b, int64_t stride_t, int64_t stride_f, const int64_t* seg_lens, const int64_t* seq_len,
                        int B, int S, int T, int F, int mode, float* out, int32_t* arg, void* stream) {
    MG_CHECK_ARG(pool_mode_known(mode), "mg_segment_pool_f32: unknown mode %d", mode);
    MG_CHECK_ARG(F >= 1, "mg_segment_pool_f32: F=%d must be at least 1", F);
    MG_CHECK_ARG(B >= 0 && S >= 0 && T >= 0, "mg_segment_pool_f32: negative size (B=%d S=%d T=%d)", B, S, T);
    MG_CHECK_ARG(B <= 65535, "mg_segment_pool_f32: B=%d exceeds 65535", B);
    MG_CHECK_ARG(S <= POOL_MAX_S, "mg_segment_pool_f32: S=%d exceeds %d segments per utterance", S, POOL_MAX_S);
    MG_CHECK_ARG(stride_b >= 0 && stride_t >= 0 && stride_f >= 0, "mg_segment_pool_f32: negative stride (%lld, %lld, %lld)",
                 (long long)stride_b, (long long)stride_t, (long long)stride_f);
    if (B == 0 || S == 0) return MG_OK;
    const bool ext = mode == MG_POOL_MAX || mode == MG_POOL_MIN;
    MG_CHECK_ARG(seg_lens && out, "mg_segment_pool_f32: seg_lens and out must not be NULL");
    MG_CHECK_ARG(x || T == 0, "mg_segment_pool_f32: x must not be NULL");
    MG_CHECK_ARG(!ext || arg, "mg_segment_pool_f32: max and min need the frame-index output arg");
    MG_CHECK_ARG(((uintptr_t)x & 3u) == 0 && ((uintptr_t)out & 3u) == 0 && ((uintptr_t)arg & 3u) == 0 && ((uintptr_t)seg_lens & 7u) == 0 &&
                     ((uintptr_t)seq_len & 7u) == 0,
                 "mg_segment_pool_f32: x, out and arg must be 4-byte, seg_lens and seq_len 8-byte aligned");
    const bool vec = stride_f == 1 && F % 4 == 0 && ((uintptr_t)x & 15u) == 0 && stride_t % 4 == 0 && stride_b % 4 == 0;
    const int lanes = vec ? F / 4 : F;                    // lanes a whole row takes
    int lf_shift = 0;
    while (lf_shift < 6 && (1 << lf_shift) < lanes) ++lf_shift;
    const int lc = POOL_THREADS >> lf_shift;
    const int sg = lc < 16 ? 16 : lc;                     // <= POOL_MAX_SEGS
    const int64_t tiles = mg_ceil_div(lanes, 1 << lf_shift);
    MG_CHECK_ARG(tiles <= 65535, "mg_segment_pool_f32: F=%d is too wide", F);
    const dim3 grid((unsigned)mg_ceil_div(S, sg), (unsigned)B, (unsigned)tiles);
    hipStream_t st = (hipStream_t)stream;
    const int mean = mode == MG_POOL_MEAN;
#define POOL_LAUNCH(V, E, M)                                                                                                          \
    hipLaunchKernelGGL((segment_pool_kernel<V, E, M>), grid, dim3(POOL_THREADS), 0, st, x, stride_b, stride_t, stride_f, seg_lens, seq_len, \
                       S, T, F, mean, lf_shift, sg, out, arg)
    if (vec) {
        if (!ext) POOL_LAUNCH(true, false, false);
        else if (mode == MG_POOL_MAX) POOL_LAUNCH(true, true, true);
        else POOL_LAUNCH(true, true, false);
    } else {
        if (!ext) POOL_LAUNCH(false, false, false);
        else if (mode == MG_POOL_MAX) POOL_LAUNCH(false, true, true);
        else POOL_LAUNCH(false, true, false);
    }
#undef POOL_LAUNCH
    MG_CHECK_LAUNCH("mg_segment_pool_f32");
    return MG_OK;
}

int mg_segment_pool_bwd_f32(const float* grad_out, const int64_t* seg_lens, const int64_t* seq_len, const int32_t* arg, int B, int S, int T,
                            int F, int mode, float* grad, void* stream) {
    MG_CHECK_ARG(pool_mode_known(mode), "mg_segment_pool_bwd_f32: unknown mode %d", mode);
    MG_CHECK_ARG(F >= 1, "mg_segment_pool_bwd_f32: F=%d must be at least 1", F);
    MG_CHECK_ARG(B >= 0 && S >= 0 && T >= 0, "mg_segment_pool_bwd_f32: negative size (B=%d S=%d T=%d)", B, S, T);
    MG_CHECK_ARG(B <= 65535, "mg_segment_pool_bwd_f32: B=%d exceeds 65535", B);
    MG_CHECK_ARG(S <= POOL_MAX_S, "mg_segment_pool_bwd_f32: S=%d exceeds %d segments per utterance", S, POOL_MAX_S);
    if (B == 0 || T == 0) return MG_OK;
    const bool ext = mode == MG_POOL_MAX || mode == MG_POOL_MIN;
    MG_CHECK_ARG(grad, "mg_segment_pool_bwd_f32: grad must not be NULL");
    MG_CHECK_ARG(S == 0 || (grad_out && seg_lens), "mg_segment_pool_bwd_f32: grad_out and seg_lens must not be NULL");
    MG_CHECK_ARG(S == 0 || !ext || arg, "mg_segment_pool_bwd_f32: max and min need the forward's frame index arg");
    MG_CHECK_ARG(((uintptr_t)grad_out & 3u) == 0 && ((uintptr_t)grad & 3u) == 0 && ((uintptr_t)arg & 3u) == 0 &&
                     ((uintptr_t)seg_lens & 7u) == 0 && ((uintptr_t)seq_len & 7u) == 0,
                 "mg_segment_pool_bwd_f32: grad_out, grad and arg must be 4-byte, seg_lens and seq_len 8-byte aligned");
    int tile = POOL_BWD_ELEMS / F;
    tile = tile < 1 ? 1 : tile > POOL_BWD_FRAMES ? POOL_BWD_FRAMES : tile;
    MG_CHECK_ARG((int64_t)tile * F <= 0x7fffffff / 4, "mg_segment_pool_bwd_f32: F=%d is too wide", F);
    const dim3 grid((unsigned)mg_ceil_div(T, tile), (unsigned)B);
    const size_t lds = (size_t)S * sizeof(int);
    const bool vec = F % 4 == 0 && ((uintptr_t)grad & 15u) == 0;      // the loads of grad_out and arg stay 4 bytes wide
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(segment_pool_bwd_kernel<true>, grid, dim3(POOL_THREADS), lds, st, grad_out, seg_lens, seq_len, arg, S, T, F, mode,
                           tile, grad);
    else
        hipLaunchKernelGGL(segment_pool_bwd_kernel<false>, grid, dim3(POOL_THREADS), lds, st, grad_out, seg_lens, seq_len, arg, S, T, F, mode,
                           tile, grad);
    MG_CHECK_LAUNCH("mg_segment_pool_bwd_f32");
    return MG_OK;
}

}  // extern "C"
