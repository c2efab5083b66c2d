// K31 - integer durations from a duration model's real-valued prediction: the quantiser between models.DurationModel and everything
// that reads `dur` (upsample.hip, counters.hip, the acoustic models).  pred[b, p, s] is a float32 prediction in the normalised space of
// the `dur` normaliser, P phones of S sub-phone states.  Segments i = 0 .. n-1 run in (p, s) order over the valid phones of one item:
//
//   x_i = (double)pred * (double)p1[s] + (double)p0[s]      (the product of two float32 is exact in float64: one rounding)
//         exp(x_i) if log_input;  x_i * scale;  a non-finite or negative x_i -> 0 (flag bit 0);  min(x_i, hi)
//   q_i = floor(x_i * 65536 + 0.5) as int64                 16 fractional bits; everything from here on is integer
//   total != NULL:  Q = sum q_i;  Q > 0 and total_b > 0:  q_i = min(floor((double)q_i * ((double)(total_b << 16) / (double)Q) + 0.5), hi << 16)
//                   else the step is left out (flag bit 1)
//   MG_DUR_NEAREST: d_i = max(lo, (q_i + 32768) >> 16)
//   MG_DUR_CARRY:   C_i = q_0 + .. + q_i,  R_i = (C_i + 32768) >> 16,  E_i = (i + 1) lo + max(0, max_{j <= i}(R_j - (j + 1) lo)),
//                   d_i = E_i - E_{i-1} (E_{-1} = 0): the closed form of "emit max(lo, R_i - the frames emitted so far)".
//                   Flag bit 2: E_{n-1} != (C_{n-1} + 32768) >> 16, the minimum pushed the length out.
//
// Contraction is off; the NumPy restatement (data.quantise_durations) has none.
//
// Mapping.  One workgroup per item.  It walks the item's n segments in chunks of DQ_THREADS, thread = segment, so that a wave stores
// 512 contiguous bytes of `dur` per instruction.  Per chunk: an inclusive int64 sum scan of q (wave shuffles, the four wave totals
// through LDS) on top of the carried sum of the chunks before, then an inclusive int64 max scan of R_i - (i + 1) lo on top of the
// carried maximum; the chunk's E_i go to LDS, where a thread finds E_{i-1} and the last state of a phone finds the E before its
// phone (carried in a register when that lies in an earlier chunk).  With `total` a first walk sums q (a block reduction per item)
// and the second walk recomputes q_i from pred.  All scans are integer: the bits depend on the values alone, not on the chunking.
// The tail of the item (segments n .. P S - 1, phones used .. P - 1) is written as zeros by the same launch; phones at or past
// n_phones[b] are never read.  No workspace, no atomics, no host read.
#include "common.h"

#pragma clang fp contract(off)

#define DQ_THREADS 256
#define DQ_WAVES (DQ_THREADS / 64)
#define DQ_MAX_ITEMS 65535
#define DQ_MAX_SEGMENTS (1 << 24)      // exclusive
#define DQ_MAX_FRAMES MG_DUR_MAX_FRAMES    // hi

#include "item_norm.h"      // after the pragma (mg_item_param_rows only: the de-normalisation here is float64)

struct DqParams {
    const float* pred;
    int64_t sb, sp, ss;
    int P, S;
    const float *p0, *p1;
    int log_input;
    double scale;
    int64_t lo, hi;
};

// q_i of segment i of item b (q0 / q1: the item's parameter rows or NULL); sets bit 0 of `flags` when the value had to be replaced
__device__ __forceinline__ int64_t dq_fixed(const DqParams& a, int b, int i, const float* q0, const float* q1, int& flags) {
    const int p = i / a.S, s = i - p * a.S;
    const float v = a.pred[(int64_t)b * a.sb + (int64_t)p * a.sp + (int64_t)s * a.ss];
    double x = (double)v;
    if (q0) x = (double)v * (double)q1[s] + (double)q0[s];
    if (a.log_input) x = exp(x);
    x = x * a.scale;
    if (!(x >= 0.0) || x > 1.7976931348623157e308) {      // NaN, negative, infinite
        x = 0.0;
        flags |= MG_DUR_FLAG_INVALID;
    }
    const double top = (double)a.hi;
    if (x > top) x = top;
    return (int64_t)floor(x * 65536.0 + 0.5);             // <= 2^36
}

__device__ __forceinline__ int64_t dq_fit(int64_t q, double ratio, int64_t hi) {
    double y = floor((double)q * ratio + 0.5);
    const double top = (double)(hi << 16);
    if (y > top) y = top;                                 // in float64, before the conversion: the product may exceed int64
    return (int64_t)y;
}

template <bool MAX>
__device__ __forceinline__ int64_t dq_combine(int64_t a, int64_t b) {
    return MAX ? (a > b ? a : b) : a + b;
}

// Inclusive scan of one value per thread over the workgroup; `identity`: what an absent thread holds.  wave_tot: DQ_WAVES slots of
// LDS.  Returns the scan; `all` takes the combination of the whole workgroup (the same in every thread).
template <bool MAX>
__device__ __forceinline__ int64_t dq_block_scan(int64_t v, int64_t identity, int64_t* wave_tot, int64_t& all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t o = __shfl_up((long long)v, off);
        if (lane >= off) v = dq_combine<MAX>(v, o);
    }
    __syncthreads();                                      // the previous readers of wave_tot are done
    if (lane == 63) wave_tot[wave] = v;
    __syncthreads();
    int64_t before = identity;
    all = identity;
    for (int w = 0; w < DQ_WAVES; ++w) {
        const int64_t t = wave_tot[w];
        if (w < wave) before = dq_combine<MAX>(before, t);
        all = dq_combine<MAX>(all, t);
    }
    return dq_combine<MAX>(before, v);
}

__global__ __launch_bounds__(DQ_THREADS) void quantise_durations_kernel(DqParams a, int B, const int64_t* __restrict__ n_phones,
                                                                        const int32_t* __restrict__ item_row, int n_rows, int rounding,
                                                                        const int64_t* __restrict__ total, int64_t* __restrict__ dur,
                                                                        int64_t* __restrict__ phone_dur, int64_t* __restrict__ n_frames,
                                                                        int32_t* __restrict__ flags_out) {
    __shared__ int64_t wave_tot[DQ_WAVES];
    __shared__ int64_t ends[DQ_THREADS];                  // E_i of the chunk
    __shared__ int flag_bits[DQ_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;                             // < B: the grid is B workgroups
    const int S = a.S, all_segments = a.P * S;            // < 2^24
    int used = a.P;
    if (n_phones) {
        const int64_t np = n_phones[b];
        used = np < 0 ? 0 : (np < a.P ? (int)np : a.P);
    }
    const float *q0 = a.p0, *q1 = a.p1;
    const bool row_ok = !a.p0 || mg_item_param_rows(item_row, b, n_rows, S, q0, q1);
    const int n = row_ok ? used * S : 0;
    int flags = 0;                                        // bit 0 per thread, merged at the end
    int item_flags = row_ok ? 0 : MG_DUR_FLAG_NO_ROW;     // uniform

    // -- the fit to `total`: Q first
    bool fit = false;
    double ratio = 1.0;
    if (total && row_ok) {
        int64_t local = 0;
        int unused = 0;
        for (int i = tid; i < n; i += DQ_THREADS) local += dq_fixed(a, b, i, q0, q1, unused);
        for (int off = 32; off > 0; off >>= 1) local += __shfl_xor((long long)local, off);
        if (lane == 0) wave_tot[wave] = local;
        __syncthreads();
        int64_t Q = 0;
        for (int w = 0; w < DQ_WAVES; ++w) Q += wave_tot[w];
        const int64_t want = total[b];
        if (Q > 0 && want > 0) {
            fit = true;
            ratio = ((double)want * 65536.0) / (double)Q;
        } else {
            item_flags |= MG_DUR_FLAG_NO_FIT;
        }
    }

    // -- the walk: carried over the chunks, the same in every thread
    int64_t carry_c = 0;                                  // C of the last segment before the chunk
    int64_t carry_m = 0;                                  // max(0, max_j (R_j - (j + 1) lo)) before the chunk
    int64_t carry_e = 0;                                  // E of the last segment before the chunk
    int64_t phone_base = 0;                               // E of the last phone end before the chunk
    int64_t* out = dur + (int64_t)b * all_segments;
    for (int c0 = 0; c0 < n; c0 += DQ_THREADS) {
        const int i = c0 + tid;
        const bool live = i < n;
        int64_t q = 0;
        if (live) {
            q = dq_fixed(a, b, i, q0, q1, flags);
            if (fit) q = dq_fit(q, ratio, a.hi);
        }
        int64_t e, chunk_c, chunk_x;
        const int64_t c = carry_c + dq_block_scan<false>(q, 0, wave_tot, chunk_c);
        if (rounding == MG_DUR_CARRY) {
            const int64_t r = (c + 32768) >> 16;
            const int64_t m = live ? r - (int64_t)(i + 1) * a.lo : INT64_MIN;
            int64_t x = dq_block_scan<true>(m, INT64_MIN, wave_tot, chunk_x);
            if (x < carry_m) x = carry_m;
            if (chunk_x > carry_m) carry_m = chunk_x;
            e = (int64_t)(i + 1) * a.lo + x;
        } else {
            int64_t d = (q + 32768) >> 16;
            if (d < a.lo) d = a.lo;
            e = carry_e + dq_block_scan<false>(live ? d : 0, 0, wave_tot, chunk_x);
        }
        carry_c += chunk_c;
        ends[tid] = e;
        __syncthreads();
        const int last = min(n - c0, DQ_THREADS) - 1;     // the chunk's last live thread
        if (live) {
            out[i] = e - (tid ? ends[tid - 1] : carry_e);
            if (i % S == S - 1) phone_dur[(int64_t)b * a.P + i / S] = e - (i - S >= c0 ? ends[tid - S] : phone_base);
        }
        const int last_i = c0 + last;
        const int last_end = (last_i + 1) / S * S - 1;    // the last phone end at or before last_i (-1: none)
        const int64_t next_e = ends[last];
        const int64_t next_base = last_end >= c0 ? ends[last_end - c0] : phone_base;
        __syncthreads();                                  // every read of ends is done before the next chunk writes it
        carry_e = next_e;
        phone_base = next_base;
    }
    // -- the item's tail: zeros
    for (int i = n + tid; i < all_segments; i += DQ_THREADS) out[i] = 0;
    for (int p = n / S + tid; p < a.P; p += DQ_THREADS) phone_dur[(int64_t)b * a.P + p] = 0;

    // -- flags
    for (int off = 32; off > 0; off >>= 1) flags |= __shfl_xor(flags, off);
    if (lane == 0) flag_bits[wave] = flags;
    __syncthreads();
    if (tid == 0) {
        for (int w = 0; w < DQ_WAVES; ++w) item_flags |= flag_bits[w];
        if (rounding == MG_DUR_CARRY && carry_e != ((carry_c + 32768) >> 16)) item_flags |= MG_DUR_FLAG_PUSHED;
        n_frames[b] = carry_e;
        flags_out[b] = item_flags;
    }
}

extern "C" {

int mg_quantise_durations_f32(const float* pred, int B, int P, int S, int64_t stride_b, int64_t stride_p, int64_t stride_s,
                              const int64_t* n_phones, const float* p0, const float* p1, const int32_t* item_row, int n_rows, int log_input,
                              double scale, int64_t lo, int64_t hi, int rounding, const int64_t* total, int64_t* dur, int64_t* phone_dur,
                              int64_t* n_frames, int32_t* flags, void* stream) {
    MG_CHECK_ARG(rounding == MG_DUR_CARRY || rounding == MG_DUR_NEAREST, "mg_quantise_durations_f32: unknown rounding %d", rounding);
    MG_CHECK_ARG(B >= 0 && P > 0 && S > 0, "mg_quantise_durations_f32: bad shape (B=%d P=%d S=%d)", B, P, S);
    MG_CHECK_ARG(B <= DQ_MAX_ITEMS, "mg_quantise_durations_f32: B=%d exceeds %d items", B, DQ_MAX_ITEMS);
    MG_CHECK_ARG((int64_t)P * S < DQ_MAX_SEGMENTS, "mg_quantise_durations_f32: P=%d x S=%d must stay below %d segments per item", P, S,
                 DQ_MAX_SEGMENTS);
    MG_CHECK_ARG(stride_b >= 0 && stride_p >= 0 && stride_s >= 0, "mg_quantise_durations_f32: negative strides (%lld, %lld, %lld)",
                 (long long)stride_b, (long long)stride_p, (long long)stride_s);
    MG_CHECK_ARG(lo >= 0 && lo <= hi && hi <= DQ_MAX_FRAMES, "mg_quantise_durations_f32: need 0 <= lo=%lld <= hi=%lld <= %d", (long long)lo,
                 (long long)hi, DQ_MAX_FRAMES);
    MG_CHECK_ARG(scale > 0.0 && scale <= 1.7976931348623157e308, "mg_quantise_durations_f32: scale=%g must be positive and finite", scale);
    MG_CHECK_ARG((p0 != NULL) == (p1 != NULL), "mg_quantise_durations_f32: p0 and p1 go together");
    MG_CHECK_ARG(!item_row || p0, "mg_quantise_durations_f32: item_row without parameter tables");
    MG_CHECK_PARAM_ROWS("mg_quantise_durations_f32", "n_rows", item_row, n_rows);
    if (B == 0) return MG_OK;
    MG_CHECK_ARG(pred && dur && phone_dur && n_frames && flags, "mg_quantise_durations_f32: pred and the four outputs must not be NULL");
    MG_CHECK_ARG((((uintptr_t)pred | (uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)item_row | (uintptr_t)flags) & 3u) == 0 &&
                     (((uintptr_t)n_phones | (uintptr_t)total | (uintptr_t)dur | (uintptr_t)phone_dur | (uintptr_t)n_frames) & 7u) == 0,
                 "mg_quantise_durations_f32: pred, the parameters, item_row and flags must be 4-byte, n_phones, total, dur, phone_dur and "
                 "n_frames 8-byte aligned");
    DqParams a;
    a.pred = pred, a.sb = stride_b, a.sp = stride_p, a.ss = stride_s, a.P = P, a.S = S;
    a.p0 = p0, a.p1 = p1, a.log_input = log_input != 0, a.scale = scale, a.lo = lo, a.hi = hi;
    hipLaunchKernelGGL(quantise_durations_kernel, dim3((unsigned)B), dim3(DQ_THREADS), 0, (hipStream_t)stream, a, B, n_phones, item_row, n_rows,
                       rounding, total, dur, phone_dur, n_frames, flags);
    MG_CHECK_LAUNCH("mg_quantise_durations_f32");
    return MG_OK;
}

}  // extern "C"
