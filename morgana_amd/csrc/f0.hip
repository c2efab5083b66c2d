// K29 - continuous log-F0 and voicing from an extractor's raw F0 track: what the un-vendored tts_data_tools writes as the `lf0` and `vuv`
// files every F0 model of the reference reads (models/f0_test_model.py, models/RNN_SPSS.py).  Per item of n frames and per column d:
//
//   voiced[t] = x[t, d] > voiced_above                              (a NaN is unvoiced)
//   l[t]      = log((double)x[t, d])   or, log_input, (double)x[t, d]
//   lf0[t]    = (float)l[t]                                         voiced
//             = (float)( l[a] + (l[b] - l[a]) * w ),  w = (double)(t - a) / (double)(b - a)
//                                                                   unvoiced, a < t < b the nearest voiced frames on either side
//             = (float)l[b] / (float)l[a]                           no voiced frame before / after t (np.interp's convention)
//             = fill                                                no voiced frame in the item
//   vuv[t]    = voiced[t] ? 1 : 0
//
// all in float64 in exactly this order, rounded once; floating-point contraction is off, as the NumPy restatement
// (data.continuous_lf0 on an array) has none.  The normalised twin is mg_normalise_f32's float arithmetic (csrc/item_norm.h) on the
// rounded value.
//
// Mapping.  ONE WORKGROUP PER ITEM (grid-stride over the items); its four waves take the item column by column in trips of
// F0_CHUNK_ROWS = 4 x 64 frames, one wave per 64-frame segment, lane = frame.  A wave ballots `voiced` over its segment; a lane finds
// its neighbours inside the segment from the mask (clz / ctz).  A segment whose first (last) run is unvoiced walks outward from its
// edge, one ballot of 64 frames at a time, until the first voiced frame or the ITEM's boundary: the walk is indexed inside the item,
// so it cannot reach the neighbouring item of a packed batch.  Neighbour VALUES are read again from memory (L1 / L2) and their
// logarithm recomputed: the same function of the same input, so the same bits as the voiced frame's own output.  Nothing is staged in
// LDS, there is no carry between segments, no workspace and no atomics; every output element is a function of the item alone: the
// same bits on every call.
//
// Accepted worst case: an all-unvoiced item of n frames costs each of its n / 64 segments about n / 64 ballots (n^2 / 4096 loads of
// 64 frames per column, all from cache): 16 x 16 for a 1000-frame utterance.  An item is one workgroup's work whatever its length:
// a batch of few, very long items does not fill the device.  D > 1 reads with a stride of D floats per lane; D is 1 for F0.
//
// The only LDS is the fixed 256-entry reduction that gives a padded input's item its first packed row (the sum of the clamped lengths
// in front of it) when a packed output is asked for.
#include "common.h"

#pragma clang fp contract(off)

#define F0_THREADS 256
#define F0_WAVE 64
#define F0_WAVES (F0_THREADS / F0_WAVE)
#define F0_CHUNK_ROWS (F0_WAVES * F0_WAVE)
#define F0_MAX_BLOCKS 65536

#include "item_norm.h"      // after the pragma: a forward kind is a subtraction and a division, nothing to contract

__device__ __forceinline__ double f0_log(float x, int log_input) { return log_input ? (double)x : log((double)x); }

__global__ __launch_bounds__(F0_THREADS) void continuous_lf0_kernel(const float* __restrict__ x, const int64_t* __restrict__ offsets,
                                                                    const int64_t* __restrict__ seq_len, int64_t T_in, int B, int D,
                                                                    int log_input, float voiced_above, float fill,
                                                                    const float* __restrict__ p0, const float* __restrict__ p1,
                                                                    const int32_t* __restrict__ item_row, int S, int kind,
                                                                    int64_t out_rows, int64_t packed_rows, float* __restrict__ packed_out,
                                                                    float* __restrict__ padded_out, float* __restrict__ norm_out,
                                                                    float* __restrict__ vuv_out, int vuv_packed) {
    __shared__ int64_t s_part[F0_THREADS];
    const int tid = threadIdx.x;
    const int lane = tid & (F0_WAVE - 1), wave = tid / F0_WAVE;
    const bool want_packed_rows = packed_out || (vuv_out && vuv_packed);
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        // the item: uniform for the workgroup
        int64_t first, len;
        mg_item_rows(offsets, seq_len, T_in, b, first, len);
        int64_t pfirst = offsets ? first : 0;
        if (!offsets && want_packed_rows) {                    // a padded item's first packed row: the clamped lengths in front of it
            int64_t part = 0;
            for (int i = tid; i < b; i += F0_THREADS) {
                int64_t n = seq_len[i];
                if (n > T_in) n = T_in;
                if (n > 0) part += n;
            }
            __syncthreads();                                   // (the previous item's readers of s_part are done)
            s_part[tid] = part;
            __syncthreads();
            for (int half = F0_THREADS / 2; half > 0; half >>= 1) {
                if (tid < half) s_part[tid] += s_part[tid + half];
                __syncthreads();
            }
            pfirst = s_part[0];
        }
        const float* src = x + first * D;
        const float *q0 = p0, *q1 = p1;
        const bool row_ok = !norm_out || mg_item_param_rows(item_row, b, S, D, q0, q1);      // false: NaN in the valid frames
        const int64_t n_seg = (len + F0_WAVE - 1) / F0_WAVE;
        for (int d = 0; d < D; ++d) {
            for (int64_t s = wave; s < n_seg; s += F0_WAVES) {       // uniform for the wave: every ballot below is taken by all 64 lanes
                const int64_t t = s * F0_WAVE + lane;
                const bool valid = t < len;
                const float xv = valid ? src[t * D + d] : 0.f;
                const bool voiced = valid && xv > voiced_above;
                const uint64_t m = __ballot(voiced);
                const int64_t in_seg = len - s * F0_WAVE < F0_WAVE ? len - s * F0_WAVE : F0_WAVE;      // >= 1
                const int f = m ? __builtin_ctzll(m) : F0_WAVE;            // the segment's first voiced lane
                const int g = m ? 63 - __builtin_clzll(m) : -1;            // ... and its last
                int64_t a_out = -1, b_out = -1;                            // the nearest voiced frames outside the segment
                if (f > 0) {
                    for (int64_t ss = s - 1; ss >= 0; --ss) {              // whole segments of the item: every lane's frame exists
                        const float y = src[(ss * F0_WAVE + lane) * D + d];
                        const uint64_t mm = __ballot(y > voiced_above);
                        if (mm) {
                            a_out = ss * F0_WAVE + 63 - __builtin_clzll(mm);
                            break;
                        }
                    }
                }
                if (g < in_seg - 1) {
                    for (int64_t ss = s + 1; ss < n_seg; ++ss) {
                        const int64_t tt = ss * F0_WAVE + lane;
                        const bool ok = tt < len;
                        const float y = ok ? src[tt * D + d] : 0.f;
                        const uint64_t mm = __ballot(ok && y > voiced_above);
                        if (mm) {
                            b_out = ss * F0_WAVE + __builtin_ctzll(mm);
                            break;
                        }
                    }
                }
                if (!valid) continue;
                float v;
                if (voiced) {
                    v = (float)f0_log(xv, log_input);
                } else {
                    const uint64_t below = m & ((1ull << lane) - 1ull);
                    const uint64_t above = m & ~((2ull << lane) - 1ull);
                    const int64_t a = below ? s * F0_WAVE + 63 - __builtin_clzll(below) : a_out;
                    const int64_t c = above ? s * F0_WAVE + __builtin_ctzll(above) : b_out;
                    if (a < 0 && c < 0) {
                        v = fill;
                    } else if (a < 0) {
                        v = (float)f0_log(src[c * D + d], log_input);
                    } else if (c < 0) {
                        v = (float)f0_log(src[a * D + d], log_input);
                    } else {
                        const double la = f0_log(src[a * D + d], log_input), lb = f0_log(src[c * D + d], log_input);
                        const double w = (double)(t - a) / (double)(c - a);
                        v = (float)(la + (lb - la) * w);
                    }
                }
                const float flag = voiced ? 1.f : 0.f;
                const bool in_packed = pfirst + t < packed_rows, in_padded = t < out_rows;
                const int64_t at_packed = (pfirst + t) * D + d, at_padded = ((int64_t)b * out_rows + t) * D + d;
                if (packed_out && in_packed) packed_out[at_packed] = v;
                if (padded_out && in_padded) padded_out[at_padded] = v;
                if (norm_out && in_padded) norm_out[at_padded] = row_ok ? mg_norm_forward(v, q0[d], q1[d], kind) : __builtin_nanf("");
                if (vuv_out) {
                    if (vuv_packed) {
                        if (in_packed) vuv_out[at_packed] = flag;
                    } else if (in_padded) {
                        vuv_out[at_padded] = flag;
                    }
                }
            }
        }
        // the pad frames of the padded outputs: exact zeros, by the same launch
        if (len < out_rows && (padded_out || norm_out || (vuv_out && !vuv_packed))) {
            const int64_t lo = ((int64_t)b * out_rows + len) * D, hi = ((int64_t)b + 1) * out_rows * D;
            for (int64_t e = lo + tid; e < hi; e += F0_THREADS) {
                if (padded_out) padded_out[e] = 0.f;
                if (norm_out) norm_out[e] = 0.f;
                if (vuv_out && !vuv_packed) vuv_out[e] = 0.f;
            }
        }
    }
}

extern "C" {

int mg_continuous_lf0_chunk_rows(void) { return F0_CHUNK_ROWS; }

int mg_continuous_lf0_f32(const float* x, int D, int B, const int64_t* offsets, const int64_t* seq_len, int T_in, int log_input,
                          float voiced_above, float fill, const float* p0, const float* p1, const int32_t* item_row, int S, int kind,
                          int64_t out_rows, int64_t packed_rows, float* packed_out, float* padded_out, float* norm_out, float* vuv_out,
                          int vuv_form, void* stream) {
    MG_CHECK_ONE_LAYOUT("mg_continuous_lf0_f32", offsets, seq_len, "(B, T_in, D)");
    MG_CHECK_ARG(D > 0, "mg_continuous_lf0_f32: D=%d must be positive", D);
    MG_CHECK_ARG(B >= 0, "mg_continuous_lf0_f32: B=%d must not be negative", B);
    MG_CHECK_ARG(offsets || T_in >= 0, "mg_continuous_lf0_f32: T_in=%d must not be negative", T_in);
    MG_CHECK_ARG(voiced_above == voiced_above, "mg_continuous_lf0_f32: voiced_above is NaN: no frame would be voiced");
    MG_CHECK_ARG(packed_out || padded_out || norm_out || vuv_out, "mg_continuous_lf0_f32: no output requested");
    MG_CHECK_ARG(!vuv_out || vuv_form == MG_F0_VUV_PADDED || vuv_form == MG_F0_VUV_PACKED, "mg_continuous_lf0_f32: unknown vuv form %d",
                 vuv_form);
    const bool vuv_packed = vuv_out && vuv_form == MG_F0_VUV_PACKED;
    const bool any_padded = padded_out || norm_out || (vuv_out && !vuv_packed), any_packed = packed_out || vuv_packed;
    MG_CHECK_ARG(!any_padded || (out_rows >= 0 && out_rows <= INT32_MAX),
                 "mg_continuous_lf0_f32: out_rows=%lld (frames per item of the padded outputs) out of range", (long long)out_rows);
    MG_CHECK_ARG(!any_packed || (packed_rows >= 0 && packed_rows <= INT64_MAX / 4 / D),
                 "mg_continuous_lf0_f32: packed_rows=%lld (rows of the packed outputs) out of range", (long long)packed_rows);
    MG_CHECK_NORM_TWIN("mg_continuous_lf0_f32", norm_out, p0, p1, kind);
    MG_CHECK_PARAM_ROWS("mg_continuous_lf0_f32", "S", item_row, S);
    MG_CHECK_ARG(!any_padded || B == 0 || out_rows == 0 || out_rows <= INT64_MAX / 4 / D / B,
                 "mg_continuous_lf0_f32: B=%d x T=%lld x D=%d overflow 64 bits", B, (long long)out_rows, D);
    MG_CHECK_ARG(offsets || B == 0 || T_in == 0 || (int64_t)T_in <= INT64_MAX / 4 / D / B,
                 "mg_continuous_lf0_f32: B=%d x T_in=%d x D=%d overflow 64 bits", B, T_in, D);
    if (B == 0) return MG_OK;
    MG_CHECK_ARG(x, "mg_continuous_lf0_f32: x must not be NULL");
    MG_CHECK_ARG((((uintptr_t)x | (uintptr_t)packed_out | (uintptr_t)padded_out | (uintptr_t)norm_out | (uintptr_t)vuv_out | (uintptr_t)p0 |
                   (uintptr_t)p1 | (uintptr_t)item_row) & 3u) == 0 && (((uintptr_t)offsets | (uintptr_t)seq_len) & 7u) == 0,
                 "mg_continuous_lf0_f32: x, the outputs, the parameters and item_row must be 4-byte, offsets and seq_len 8-byte aligned");
    const unsigned blocks = (unsigned)(B < F0_MAX_BLOCKS ? B : F0_MAX_BLOCKS);
    hipLaunchKernelGGL(continuous_lf0_kernel, dim3(blocks), dim3(F0_THREADS), 0, (hipStream_t)stream, x, offsets, seq_len, (int64_t)T_in, B, D,
                       log_input ? 1 : 0, voiced_above, fill, p0, p1, item_row, S, kind, any_padded ? out_rows : 0,
                       any_packed ? packed_rows : 0, packed_out, padded_out, norm_out, vuv_out, vuv_packed ? 1 : 0);
    MG_CHECK_LAUNCH("mg_continuous_lf0_f32");
    return MG_OK;
}

}  // extern "C"
