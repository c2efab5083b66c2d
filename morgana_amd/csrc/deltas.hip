// K23 - delta features: the FORWARD of the window operator whose inverse is MLPG (csrc/mlpg.hip).  Output column w D + d at frame t is
//     sum_k coeff[w][k] x[t - l_w + k, d],
// row t of the window matrix W_w of morgana/viz/synthesis.py:8-36 (_build_win_mats).  The reference never applies it: its delta
// streams ({name}_deltas files) come from the un-vendored tts_data_tools.  Here the loader's pad-and-normalise pass applies it to the
// statics that are on the device anyway (mg_pad_normalise_f32 with a stencil in front), and the statistics pass reads its packed form.
//
// Numerics.  Every output element: the products coeff * x in float64, taps in ascending k, the first product starting the sum and
// every later one added with one rounding each (no contraction into an fma: the NumPy restatement of data.compute_deltas has none),
// the sum rounded once to float32.  The normalised twin is mg_normalise_f32's float arithmetic (csrc/item_norm.h) on that rounded value.  A tap outside
// [0, len) reads the item's first / last frame (MG_DELTAS_EDGE_REPLICATE) or is left out (MG_DELTAS_EDGE_ZERO: exactly W_w).
//
// Memory.  One streaming pass: every input frame is read from memory once (its neighbours t +- 1, t +- 2 come from L1 / L2: nothing
// is staged in LDS), every output element written once, no atomics, no workspace.  The DESTINATION rows are cut into flat chunks of
// mg_deltas_chunk_rows(D) rows (DELTAS_CHUNK_ELEMS input elements, DELTAS_CHUNK_ELEMS_NARROW when D % 4 != 0); a chunk finds its first item by a binary search in the items'
// first destination rows (packed output; padded output: a division) - mg_item_at of csrc/item_norm.h, as csrc/unpad.hip - and walks the item pieces inside it.
// Inside a piece the item - its length, its source rows, its parameter row - is uniform for the workgroup.  16-byte loads and
// stores when D % 4 == 0 and every base is 16-byte aligned, one element per access otherwise.  64-bit element indices throughout.
// A padded input whose output is packed has no offsets to search: every workgroup scans the clamped lengths once in LDS
// (B <= MG_DELTAS_MAX_SCAN_ITEMS), the only use of LDS here.
#include "common.h"
#include "item_norm.h"
#include "packed_rows.h"

#define DELTAS_THREADS 256
#define DELTAS_CHUNK_ELEMS 2048      // input elements (rows x D) of one chunk when D % 4 == 0: two 16-byte trips per thread
#define DELTAS_CHUNK_ELEMS_NARROW 256      // ... otherwise one trip of one element: lf0 (D = 1) at 64 x 1000 frames still fills 250 workgroups
#define DELTAS_MAX_BLOCKS 2048
#define DELTAS_MAX_WINDOWS MG_MLPG_MAX_WINDOWS      // the limits of mg_mlpg_f32 (csrc/mlpg.hip)
#define DELTAS_MAX_COEFF MG_MLPG_MAX_COEFF

#define DELTAS_TO_PADDED 0           // destination rows of item b start at b T_out
#define DELTAS_TO_PACKED 1           // ... at offsets[b] (packed input: the output has the input's rows)
#define DELTAS_TO_PACKED_SCAN 2      // ... at the scanned clamped lengths (padded input), held in LDS

struct deltas_windows {
    int n;
    int l[DELTAS_MAX_WINDOWS], u[DELTAS_MAX_WINDOWS];
    double c[DELTAS_MAX_WINDOWS][DELTAS_MAX_COEFF];
};

static inline int deltas_chunk_rows(int D) {
    const int elems = D % 4 == 0 ? DELTAS_CHUNK_ELEMS : DELTAS_CHUNK_ELEMS_NARROW;
    return D >= elems ? 1 : elems / D;
}

// mg_norm_forward (csrc/item_norm.h) written out: the same float operations in the same order.  Left here because with the shared
// function, in any form tried, hipcc allocates deltas_kernel<4, *> other registers than it had (45 / 44 / 44 or 60 / 59 / 57, not
// 46 / 45 / 45); tests/test_gpu_deltas.py holds the two to the same bits.
__device__ __forceinline__ float deltas_norm(float v, float a, float b, int kind) {
    if (kind == MG_NORM_MVN) return (v - a) / (b + 1e-8f);
    float scale = b - a;
    if (fabsf(scale) <= 1e-8f) scale = 1.f;
    return (v - a) / scale;
}

template <int MODE>
__device__ __forceinline__ int64_t deltas_first_row(int b, int64_t T_out, const int64_t* __restrict__ offsets, const int64_t* s_cum) {
    if (MODE == DELTAS_TO_PADDED) return (int64_t)b * T_out;
    if (MODE == DELTAS_TO_PACKED) return offsets[b];
    return s_cum[b];
}

template <int VEC, int MODE>
__global__ __launch_bounds__(DELTAS_THREADS) void deltas_kernel(const float* __restrict__ x, const int64_t* __restrict__ offsets,
                                                                const int64_t* __restrict__ seq_len, int64_t T_in, int B, int D,
                                                                deltas_windows win, int edge, const float* __restrict__ p0,
                                                                const float* __restrict__ p1, const int32_t* __restrict__ item_row, int S,
                                                                int kind, int64_t T_out, int64_t out_rows, int chunk_rows,
                                                                float* __restrict__ raw_out, float* __restrict__ norm_out) {
    extern __shared__ __attribute__((aligned(16))) int64_t s_deltas[];      // DELTAS_TO_PACKED_SCAN only: [B + 1] first rows, [256] partials
    const int tid = threadIdx.x;
    const int64_t* s_cum = s_deltas;
    if (MODE == DELTAS_TO_PACKED_SCAN) {
        mg_clamped_length_scan(seq_len, B, T_in, s_deltas, s_deltas + B + 1);
    }

    const int W = win.n;
    const int64_t WD = (int64_t)W * D;
    const int step = DELTAS_THREADS * VEC;
    const int dr = step / D, dd = step - dr * D;
    const int64_t n_chunks = (out_rows + chunk_rows - 1) / chunk_rows;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t c_lo = c * chunk_rows;
        const int64_t c_hi = c_lo + chunk_rows < out_rows ? c_lo + chunk_rows : out_rows;
        const auto first_of = [&](int b) { return deltas_first_row<MODE>(b, T_out, offsets, s_cum); };
        // the item that holds destination row c_lo, then the item pieces inside the chunk
        int b = MODE == DELTAS_TO_PADDED ? (int)(c_lo / T_out) : mg_item_at(B, c_lo, first_of);
        for (; b < B; ++b) {
            const int64_t i_lo = first_of(b), i_hi = first_of(b + 1);
            if (i_lo >= c_hi) break;
            const int64_t p_lo = i_lo > c_lo ? i_lo : c_lo, p_hi = i_hi < c_hi ? i_hi : c_hi;
            if (p_hi <= p_lo) continue;                        // an empty item
            // the item: uniform for the workgroup
            int64_t first, len;
            mg_item_rows(offsets, seq_len, T_in, b, first, len);
            if (MODE == DELTAS_TO_PADDED && len > T_out) len = T_out;      // cut to T_out frames, as mg_pad_normalise_f32 cuts it
            const float* src = x + first * D;
            const float *q0 = p0, *q1 = p1;
            const bool row_ok = !norm_out || mg_item_param_rows(item_row, b, S, WD, q0, q1);      // false: NaN in the valid frames
            const int64_t t0 = p_lo - i_lo;
            const int64_t n_el = (p_hi - p_lo) * D;
            int64_t e = (int64_t)tid * VEC;
            int64_t rr = e / D;
            int d = (int)(e - rr * D);
            for (; e < n_el; e += step) {
                const int64_t t = t0 + rr;
                const int64_t at = (p_lo + rr) * WD + d;       // (this row, window 0, column d) of the outputs
                for (int w = 0; w < W; ++w) {
                    float v[VEC], r[VEC];
#pragma unroll
                    for (int j = 0; j < VEC; ++j) v[j] = r[j] = 0.f;
                    if (t < len) {
                        double acc[VEC];
                        const int l = win.l[w], nk = l + win.u[w] + 1;
                        bool open = true;
                        for (int k = 0; k < nk; ++k) {
                            int64_t tt = t - l + k;
                            if (tt < 0 || tt >= len) {
                                if (edge == MG_DELTAS_EDGE_ZERO) continue;
                                tt = tt < 0 ? 0 : len - 1;
                            }
                            const double ck = win.c[w][k];
                            const float* at_x = src + tt * D + d;
                            float xv[VEC];
                            if (VEC == 4) {
                                const f32x4 q = *reinterpret_cast<const f32x4*>(at_x);
#pragma unroll
                                for (int j = 0; j < VEC; ++j) xv[j] = q[j];
                            } else {
                                xv[0] = at_x[0];
                            }
#pragma unroll
                            for (int j = 0; j < VEC; ++j) {
                                const double prod = __dmul_rn(ck, (double)xv[j]);
                                acc[j] = open ? prod : __dadd_rn(acc[j], prod);
                            }
                            open = false;
                        }
#pragma unroll
                        for (int j = 0; j < VEC; ++j) v[j] = open ? 0.f : (float)acc[j];
                        if (norm_out) {
                            const int col = w * D + d;
#pragma unroll
                            for (int j = 0; j < VEC; ++j) r[j] = __builtin_nanf("");
                            if (row_ok) {
                                float a[VEC], bb[VEC];
                                if (VEC == 4) {
                                    const f32x4 qa = *reinterpret_cast<const f32x4*>(q0 + col), qb = *reinterpret_cast<const f32x4*>(q1 + col);
#pragma unroll
                                    for (int j = 0; j < VEC; ++j) {
                                        a[j] = qa[j];
                                        bb[j] = qb[j];
                                    }
                                } else {
                                    a[0] = q0[col];
                                    bb[0] = q1[col];
                                }
#pragma unroll
                                for (int j = 0; j < VEC; ++j) r[j] = deltas_norm(v[j], a[j], bb[j], kind);
                            }
                        }
                    }
                    const int64_t o = at + (int64_t)w * D;
                    if (VEC == 4) {
                        if (raw_out) *reinterpret_cast<f32x4*>(raw_out + o) = f32x4{v[0], v[1], v[2], v[3]};
                        if (norm_out) *reinterpret_cast<f32x4*>(norm_out + o) = f32x4{r[0], r[1], r[2], r[3]};
                    } else {
                        if (raw_out) raw_out[o] = v[0];
                        if (norm_out) norm_out[o] = r[0];
                    }
                }
                d += dd;
                rr += dr;
                if (d >= D) {
                    d -= D;
                    ++rr;
                }
            }
        }
    }
}

template <int VEC, int MODE>
static void deltas_launch(unsigned blocks, size_t lds, hipStream_t st, const float* x, const int64_t* offsets, const int64_t* seq_len,
                          int64_t T_in, int B, int D, const deltas_windows& win, int edge, const float* p0, const float* p1,
                          const int32_t* item_row, int S, int kind, int64_t T_out, int64_t out_rows, float* raw_out, float* norm_out) {
    hipLaunchKernelGGL((deltas_kernel<VEC, MODE>), dim3(blocks), dim3(DELTAS_THREADS), lds, st, x, offsets, seq_len, T_in, B, D, win, edge, p0,
                       p1, item_row, S, kind, T_out, out_rows, deltas_chunk_rows(D), raw_out, norm_out);
}

extern "C" {

int mg_deltas_chunk_rows(int D) { return D > 0 ? deltas_chunk_rows(D) : 0; }

int mg_deltas_f32(const float* x, int D, int B, const int64_t* offsets, const int64_t* seq_len, int T_in, int n_windows, const int* win_l,
                  const int* win_u, const double* win_coeff, int edge, const float* p0, const float* p1, const int32_t* item_row, int S,
                  int kind, int out_form, int64_t out_rows, float* raw_out, float* norm_out, void* stream) {
    MG_CHECK_ONE_LAYOUT("mg_deltas_f32", offsets, seq_len, "(B, T_in, D)");
    MG_CHECK_ARG(D > 0, "mg_deltas_f32: D=%d must be positive", D);
    MG_CHECK_ARG(B >= 0, "mg_deltas_f32: B=%d must not be negative", B);
    MG_CHECK_ARG(n_windows > 0 && n_windows <= DELTAS_MAX_WINDOWS, "mg_deltas_f32: 1..%d windows supported, got %d", DELTAS_MAX_WINDOWS,
                 n_windows);
    MG_CHECK_ARG(win_l && win_u && win_coeff, "mg_deltas_f32: win_l, win_u and win_coeff must not be NULL");
    deltas_windows win;
    win.n = n_windows;
    for (int w = 0; w < DELTAS_MAX_WINDOWS; ++w) {
        win.l[w] = win.u[w] = 0;
        for (int k = 0; k < DELTAS_MAX_COEFF; ++k) win.c[w][k] = 0.0;
    }
    for (int w = 0; w < n_windows; ++w) {
        MG_CHECK_ARG(win_l[w] >= 0 && win_u[w] >= 0 && win_l[w] <= DELTAS_MAX_COEFF && win_u[w] <= DELTAS_MAX_COEFF &&
                         win_l[w] + win_u[w] + 1 <= DELTAS_MAX_COEFF,
                     "mg_deltas_f32: window %d (l=%d, u=%d) is wider than %d coefficients", w, win_l[w], win_u[w], DELTAS_MAX_COEFF);
        win.l[w] = win_l[w];
        win.u[w] = win_u[w];
        for (int k = 0; k <= win_l[w] + win_u[w]; ++k) win.c[w][k] = win_coeff[w * MG_MLPG_MAX_COEFF + k];
    }
    MG_CHECK_ARG((int64_t)n_windows * D <= INT32_MAX, "mg_deltas_f32: %d windows x D=%d columns overflow 32 bits", n_windows, D);
    MG_CHECK_ARG(edge == MG_DELTAS_EDGE_REPLICATE || edge == MG_DELTAS_EDGE_ZERO, "mg_deltas_f32: unknown edge mode %d", edge);
    MG_CHECK_ARG(out_form == MG_DELTAS_OUT_PADDED || out_form == MG_DELTAS_OUT_PACKED, "mg_deltas_f32: unknown output form %d", out_form);
    MG_CHECK_ARG(out_rows >= 0 && (out_form == MG_DELTAS_OUT_PACKED || out_rows <= INT32_MAX),
                 "mg_deltas_f32: out_rows=%lld (padded: frames per item, packed: rows) out of range", (long long)out_rows);
    MG_CHECK_ARG(offsets || T_in >= 0, "mg_deltas_f32: T_in=%d must not be negative", T_in);
    MG_CHECK_ARG(raw_out || norm_out, "mg_deltas_f32: no output requested");
    MG_CHECK_NORM_TWIN("mg_deltas_f32", norm_out, p0, p1, kind);
    MG_CHECK_PARAM_ROWS("mg_deltas_f32", "S", item_row, S);
    const int64_t WD = (int64_t)n_windows * D;
    int64_t total = out_rows;                                 // destination rows of the launch
    if (out_form == MG_DELTAS_OUT_PADDED) {
        MG_CHECK_ARG(B == 0 || out_rows == 0 || out_rows <= INT64_MAX / 4 / WD / B,
                     "mg_deltas_f32: B=%d x T=%lld x %lld columns overflow 64 bits", B, (long long)out_rows, (long long)WD);
        total = out_rows * B;
    } else {
        MG_CHECK_ARG(out_rows <= INT64_MAX / 4 / WD, "mg_deltas_f32: %lld rows x %lld columns overflow 64 bits", (long long)out_rows,
                     (long long)WD);
    }
    MG_CHECK_ARG(offsets || B == 0 || T_in == 0 || (int64_t)T_in <= INT64_MAX / 4 / D / B,
                 "mg_deltas_f32: B=%d x T_in=%d x D=%d overflow 64 bits", B, T_in, D);
    const bool scan = seq_len && out_form == MG_DELTAS_OUT_PACKED;
    MG_CHECK_ARG(!scan || B <= MG_DELTAS_MAX_SCAN_ITEMS, "mg_deltas_f32: a padded input with a packed output takes at most %d items, got B=%d",
                 MG_DELTAS_MAX_SCAN_ITEMS, B);
    if (B == 0 || total == 0) return MG_OK;
    MG_CHECK_ARG(x, "mg_deltas_f32: x must not be NULL");
    MG_CHECK_ARG((((uintptr_t)x | (uintptr_t)raw_out | (uintptr_t)norm_out | (uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)item_row) & 3u) == 0 &&
                     (((uintptr_t)offsets | (uintptr_t)seq_len) & 7u) == 0,
                 "mg_deltas_f32: x, the outputs, the parameters and item_row must be 4-byte, offsets and seq_len 8-byte aligned");
    uintptr_t bits = (uintptr_t)x | (uintptr_t)raw_out | (uintptr_t)norm_out;
    if (norm_out) bits |= (uintptr_t)p0 | (uintptr_t)p1;
    const bool vec = D % 4 == 0 && bits % 16 == 0;
    const int64_t chunks = mg_ceil_div(total, deltas_chunk_rows(D));
    const unsigned blocks = (unsigned)(chunks < DELTAS_MAX_BLOCKS ? chunks : DELTAS_MAX_BLOCKS);
    const size_t lds = scan ? mg_packed_scan_bytes(NULL, B, DELTAS_THREADS) : 0;
    hipStream_t st = (hipStream_t)stream;
#define DELTAS_GO(VEC, MODE) \
    deltas_launch<VEC, MODE>(blocks, lds, st, x, offsets, seq_len, T_in, B, D, win, edge, p0, p1, item_row, S, kind, out_rows, total, raw_out, norm_out)
    if (out_form == MG_DELTAS_OUT_PADDED) {
        if (vec) DELTAS_GO(4, DELTAS_TO_PADDED); else DELTAS_GO(1, DELTAS_TO_PADDED);
    } else if (!scan) {
        if (vec) DELTAS_GO(4, DELTAS_TO_PACKED); else DELTAS_GO(1, DELTAS_TO_PACKED);
    } else {
        if (vec) DELTAS_GO(4, DELTAS_TO_PACKED_SCAN); else DELTAS_GO(1, DELTAS_TO_PACKED_SCAN);
    }
#undef DELTAS_GO
    MG_CHECK_LAUNCH("mg_deltas_f32");
    return MG_OK;
}

}  // extern "C"
