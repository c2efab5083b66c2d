// Per-item normalisers: the speaker-dependent side of K5 (reference: morgana/data.py:388-530, the `_SpeakerDependentNormaliser`
// family - there a (B, D) parameter array is gathered on the host per batch and broadcast by torch over (B, T, D)).
//
// Here the parameters of ALL speakers live on the device once, as two (S, D) tables, and every batch item b names its row with
// item_row[b].  One kernel family (items_kernel) serves
//   mg_normalise_items_f32       x (B, R, D) -> out, the four kinds of mg_normalise_f32;  grad_mode: d out / d x applied to a gradient
//   mg_pad_normalise_items_f32   the device loader's pass (mg_pad_normalise_f32) with a row per utterance
// with the per-element arithmetic of normalise_kernel / pad_normalise_kernel (csrc/loss_norm.hip): both files take the factor and the
// element map from csrc/item_norm.h, so an item on speaker s gets bit for bit what mg_normalise_f32 gives with row s.
// mg_item_rows_f32 gathers the rows themselves ((B, D): what the per-item mode of mg_mlpg_f32 reads as variances' square roots).
//
// Memory bound: one read and one write of x.  grid (chunks, B): a workgroup works on ONE item, so the item's two parameter rows
// are staged once per workgroup in LDS as (offset, factor) - factor = the divisor or multiplier the kind derives from the row
// (std_dev + 1e-8, std_dev, the guarded min-max range) - and the element loop is a load, one LDS read, sub + div or fma, a store;
// 16-byte global and LDS accesses when D is a multiple of 4 and the pointers are 16-byte aligned.
//
// An item_row entry outside [0, S) never indexes the tables: the workgroup stages NaN instead, so that item's output is NaN (the
// host cannot look at a device index without a synchronisation).
#include "common.h"
#include "item_norm.h"      // no fp pragma in front of it, on purpose: the inverse kinds stay one fma, as in loss_norm.hip

#define ITEMS_MAX_D 8192          // 2 x D floats of dynamic LDS (64 KB)
#define ITEMS_CHUNK 4096          // elements of one item per workgroup and grid-stride step: 256 threads x 16

// (offset, factor) of column d for `kind`, from the item's parameter rows; grad_mode drops the offset (d out / d x is the factor alone)
__device__ __forceinline__ void items_stage(const float* __restrict__ p0, const float* __restrict__ p1, int row_ok, int D, int kind,
                                            int grad_mode, float* __restrict__ s_off, float* __restrict__ s_fac) {
    for (int d = threadIdx.x; d < D; d += 256) {
        float off = __builtin_nanf(""), fac = __builtin_nanf("");
        if (row_ok) {
            off = grad_mode ? 0.f : p0[d];
            fac = mg_norm_factor(p0[d], p1[d], kind);
        }
        s_off[d] = off;
        s_fac[d] = fac;
    }
}

// PAD: x is the packed feature and offsets (B + 1) its utterances' first rows; frames past an utterance's length are zero in both
// outputs.  !PAD: x is (B, R, D), every frame is valid, raw_out is unused.
template <bool VEC4, bool PAD>
__global__ __launch_bounds__(256) void items_kernel(const float* __restrict__ x, const int64_t* __restrict__ offsets, int64_t R, int D,
                                                    const float* __restrict__ p0, const float* __restrict__ p1,
                                                    const int32_t* __restrict__ item_row, int S, int kind, int grad_mode,
                                                    float* __restrict__ raw_out, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float s_par[];      // [0, D): offsets, [D, 2 D): factors
    float* s_off = s_par;
    float* s_fac = s_par + D;
    const int b = blockIdx.y;
    const float *q0 = p0, *q1 = p1;
    const bool row_ok = mg_item_param_rows(item_row, b, S, D, q0, q1);
    items_stage(q0, q1, row_ok, D, kind, grad_mode, s_off, s_fac);
    __syncthreads();
    const bool inverse = mg_norm_inverse(kind);
    const int64_t row_elems = R * D;
    int64_t valid = row_elems;
    const float* src = x + (size_t)b * row_elems;
    if (PAD) {
        int64_t lo, len;
        mg_item_rows(offsets, nullptr, 0, b, lo, len);
        if (len > R) len = R;
        valid = len * D;
        src = x + lo * D;
    }
    const size_t base = (size_t)b * row_elems;
    const int64_t stride = (int64_t)gridDim.x * ITEMS_CHUNK;
    for (int64_t lo = (int64_t)blockIdx.x * ITEMS_CHUNK; lo < row_elems; lo += stride) {
        const int64_t hi = min(lo + (int64_t)ITEMS_CHUNK, row_elems);
        if (VEC4) {
            int64_t e = lo + (int64_t)threadIdx.x * 4;
            int d = (int)(e % D);
            const int step = 1024 % D;
            for (; e < hi; e += 1024) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f}, r = {0.f, 0.f, 0.f, 0.f};
                if (e < valid) {                                     // D % 4 == 0: a group of four never straddles `valid` or a frame
                    v = *reinterpret_cast<const f32x4*>(src + e);
                    const f32x4 off = *reinterpret_cast<const f32x4*>(s_off + d);
                    const f32x4 fac = *reinterpret_cast<const f32x4*>(s_fac + d);
#pragma unroll
                    for (int j = 0; j < 4; ++j) r[j] = mg_norm_elem(v[j], off[j], fac[j], inverse);
                }
                if (PAD && raw_out) *reinterpret_cast<f32x4*>(raw_out + base + e) = v;
                *reinterpret_cast<f32x4*>(out + base + e) = r;
                d += step;
                if (d >= D) d -= D;
            }
        } else {
            int64_t e = lo + threadIdx.x;
            int d = (int)(e % D);
            const int step = 256 % D;
            for (; e < hi; e += 256) {
                float v = 0.f, r = 0.f;
                if (e < valid) {
                    v = src[e];
                    r = mg_norm_elem(v, s_off[d], s_fac[d], inverse);
                }
                if (PAD && raw_out) raw_out[base + e] = v;
                out[base + e] = r;
                d += step;
                if (d >= D) d -= D;
            }
        }
    }
}

__global__ __launch_bounds__(256) void item_rows_kernel(const float* __restrict__ table, int S, int D, const int32_t* __restrict__ item_row,
                                                        float* __restrict__ out) {
    const int b = blockIdx.x;
    const int row = mg_item_row(item_row, b, S);
    for (int d = threadIdx.x; d < D; d += 256) out[(size_t)b * D + d] = row >= 0 ? table[(size_t)row * D + d] : __builtin_nanf("");
}

template <bool PAD>
static void items_launch(const float* x, const int64_t* offsets, int B, int64_t R, int D, const float* p0, const float* p1,
                         const int32_t* item_row, int S, int kind, int grad_mode, float* raw_out, float* out, hipStream_t st) {
    int64_t chunks = mg_ceil_div(R * D, ITEMS_CHUNK);
    if (chunks > 1024) chunks = 1024;
    const uintptr_t ptrs = (uintptr_t)x | (uintptr_t)out | (uintptr_t)(raw_out ? raw_out : out);
    const bool vec = D % 4 == 0 && ptrs % 16 == 0;
    const size_t lds = (size_t)2 * D * sizeof(float);
    const dim3 grid((unsigned)chunks, (unsigned)B);
    if (vec)
        hipLaunchKernelGGL((items_kernel<true, PAD>), grid, dim3(256), lds, st, x, offsets, R, D, p0, p1, item_row, S, kind, grad_mode,
                           raw_out, out);
    else
        hipLaunchKernelGGL((items_kernel<false, PAD>), grid, dim3(256), lds, st, x, offsets, R, D, p0, p1, item_row, S, kind, grad_mode,
                           raw_out, out);
}

extern "C" {

int mg_normalise_items_f32(const float* x, float* out, const float* p0, const float* p1, const int32_t* item_row, int B, int64_t rows_per_item,
                           int D, int S, int kind, int grad_mode, void* stream) {
    MG_CHECK_ARG(x && out && p0 && p1 && item_row, "mg_normalise_items_f32: null argument");
    MG_CHECK_ARG(B > 0 && B <= 65535 && rows_per_item >= 0, "mg_normalise_items_f32: bad shape (B=%d rows_per_item=%lld)", B,
                 (long long)rows_per_item);
    MG_CHECK_PARAM_ROWS("mg_normalise_items_f32", "S", item_row, S);
    MG_CHECK_ARG(D > 0 && D <= ITEMS_MAX_D, "mg_normalise_items_f32: D=%d not in 1..%d", D, ITEMS_MAX_D);
    MG_CHECK_ARG(kind >= MG_NORM_MVN && kind <= MG_DENORM_MINMAX, "mg_normalise_items_f32: unknown kind %d", kind);
    if (rows_per_item == 0) return MG_OK;
    items_launch<false>(x, nullptr, B, rows_per_item, D, p0, p1, item_row, S, kind, grad_mode != 0, nullptr, out, (hipStream_t)stream);
    MG_CHECK_LAUNCH("mg_normalise_items_f32");
    return MG_OK;
}

int mg_pad_normalise_items_f32(const float* packed, const int64_t* offsets, int B, int T, int D, const float* p0, const float* p1,
                               const int32_t* item_row, int S, int kind, float* raw_out, float* norm_out, void* stream) {
    MG_CHECK_ARG(packed && offsets && p0 && p1 && item_row && norm_out, "mg_pad_normalise_items_f32: null argument");
    MG_CHECK_ARG(B > 0 && B <= 65535 && T >= 0, "mg_pad_normalise_items_f32: bad shape (B=%d T=%d)", B, T);
    MG_CHECK_PARAM_ROWS("mg_pad_normalise_items_f32", "S", item_row, S);
    MG_CHECK_ARG(D > 0 && D <= ITEMS_MAX_D, "mg_pad_normalise_items_f32: D=%d not in 1..%d", D, ITEMS_MAX_D);
    MG_CHECK_ARG(kind == MG_NORM_MVN || kind == MG_NORM_MINMAX, "mg_pad_normalise_items_f32: kind %d is not MG_NORM_MVN or MG_NORM_MINMAX",
                 kind);
    if (T == 0) return MG_OK;
    items_launch<true>(packed, offsets, B, T, D, p0, p1, item_row, S, kind, 0, raw_out, norm_out, (hipStream_t)stream);
    MG_CHECK_LAUNCH("mg_pad_normalise_items_f32");
    return MG_OK;
}

int mg_item_rows_f32(const float* table, int S, int D, const int32_t* item_row, int B, float* out, void* stream) {
    MG_CHECK_ARG(table && item_row && out, "mg_item_rows_f32: null argument");
    MG_CHECK_ARG(B > 0 && S > 0 && D > 0, "mg_item_rows_f32: bad shape (B=%d S=%d D=%d)", B, S, D);
    hipLaunchKernelGGL(item_rows_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, table, S, D, item_row, out);
    MG_CHECK_LAUNCH("mg_item_rows_f32");
    return MG_OK;
}

}  // extern "C"
