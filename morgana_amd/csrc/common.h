// Shared host/device helpers for libmorgana_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/morgana_hip.h"

#define MG_WAVE 64

void mg_set_error(const char* fmt, ...);

#define MG_CHECK_ARG(cond, ...)          \
    do {                                 \
        if (!(cond)) {                   \
            mg_set_error(__VA_ARGS__);   \
            return MG_EINVAL;            \
        }                                \
    } while (0)

// The checks the data-path entry points share (`name`, `label` and `padded` are string literals: the message names its entry point).
// A ragged input comes in exactly one layout: packed rows with offsets, or a padded batch `padded` with seq_len.
#define MG_CHECK_ONE_LAYOUT(name, offsets, seq_len, padded)          \
    MG_CHECK_ARG(((offsets) != NULL) != ((seq_len) != NULL),         \
                 name ": exactly one of offsets (packed rows) and seq_len (padded " padded ") must be given")
// The checks of an entry point that maps a ragged input `x` (`width` elements per row, 8-byte with in_f64, else 4-byte) to packed
// rows of `cols` elements in `out` (8-byte with out_f64): one layout, the sizes, the output, the alignment.  It reads the entry
// point's B, offsets, seq_len, T_in, packed_rows, out and out_f64 by name, and returns MG_OK itself where there is nothing to do.
#define MG_CHECK_PACKED_IO(name, padded, x, in_f64, width, cols)                                                                        \
    MG_CHECK_ONE_LAYOUT(name, offsets, seq_len, padded);                                                                                \
    MG_CHECK_ARG(B >= 0, name ": B=%d must not be negative", B);                                                                        \
    MG_CHECK_ARG(offsets || T_in >= 0, name ": T_in=%d must not be negative", T_in);                                                    \
    MG_CHECK_ARG(offsets || B <= MG_VOC_MAX_ITEMS, name ": a padded input takes at most %d items, got B=%d", MG_VOC_MAX_ITEMS, B);      \
    MG_CHECK_ARG(out, name ": out must not be NULL");                                                                                   \
    MG_CHECK_ARG(packed_rows >= 0 && packed_rows <= INT64_MAX / 8 / ((width) > (cols) ? (width) : (cols)),                              \
                 name ": packed_rows=%lld out of range", (long long)packed_rows);                                                       \
    MG_CHECK_ARG(offsets || B == 0 || T_in == 0 || (int64_t)T_in <= INT64_MAX / 8 / (width) / B,                                        \
                 name ": B=%d x T_in=%d x %d overflow 64 bits", B, T_in, (int)(width));                                                 \
    if (B == 0 || packed_rows == 0) return MG_OK;                                                                                       \
    MG_CHECK_ARG(x, name ": the input must not be NULL");                                                                               \
    MG_CHECK_ARG(((uintptr_t)(x) & ((in_f64) ? 7u : 3u)) == 0 && ((uintptr_t)out & (out_f64 ? 7u : 3u)) == 0 &&                         \
                     (((uintptr_t)offsets | (uintptr_t)seq_len) & 7u) == 0,                                                             \
                 name ": the input must be 4-byte (8-byte with in_f64), out 4-byte (8-byte with out_f64), offsets and seq_len 8-byte "   \
                      "aligned")
// One launch statement per element type: T names double where `f64` is set and float where it is not, in STMT.
#define MG_SWITCH_F64(f64, T, STMT)     \
    do {                                \
        if (f64) {                      \
            using T = double;           \
            STMT;                       \
        } else {                        \
            using T = float;            \
            STMT;                       \
        }                               \
    } while (0)
// A normalised twin needs both parameter operands and a forward kind.
#define MG_CHECK_NORM_TWIN(name, norm_out, p0, p1, kind)                                                          \
    MG_CHECK_ARG(!(norm_out) || ((p0) && (p1) && ((kind) == MG_NORM_MVN || (kind) == MG_NORM_MINMAX)),            \
                 name ": a normalised output needs parameters and kind MG_NORM_MVN or MG_NORM_MINMAX (kind=%d)", kind)
// item_row indexes tables of `rows` rows (the argument the entry point calls `label`).
#define MG_CHECK_PARAM_ROWS(name, label, item_row, rows) MG_CHECK_ARG(!(item_row) || (rows) > 0, name ": " label "=%d parameter rows", rows)

// Call right after a kernel launch: turns a launch-time error into MG_ELAUNCH.
#define MG_CHECK_LAUNCH(name)                                                          \
    do {                                                                               \
        hipError_t e_ = hipGetLastError();                                             \
        if (e_ != hipSuccess) {                                                        \
            mg_set_error("%s: launch failed: %s", name, hipGetErrorString(e_));        \
            return MG_ELAUNCH;                                                         \
        }                                                                              \
    } while (0)

static inline int64_t mg_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
extern int g_mg_tuning[];
// Lab builds (make lab / diag, -DMG_EXPERIMENTS) only: key 1 != 0 makes the weight-gradient entry points skip their slab-reduce launch
// (results then invalid) so that a script can time the producing kernel alone.  The product library refuses the key.
#define MG_TUNE_SKIP_REDUCE 1

static inline size_t mg_align_up(size_t a, size_t b) { return (a + b - 1) / b * b; }

// Write-through (sc1) stores for the bulk outputs of the phone-rate step's launches (the device helpers are below): a launch that
// is one tile / split / row block per workgroup ends with everything it wrote dirty in the eight L2s, and the kernel boundary
// behind it writes that back before the next launch starts; written through, the bytes leave during the epilogue's own work.
// Same bytes either way.  One bit per launch; MG_WT_DEFAULT holds the launches where the same-box A/B showed a gain (DESIGN.md
// section 4.1 has the table).  MG_TUNE_AB 85 (A/B): plain write-back stores everywhere; lab builds: 300 + mask (1, 4 or 5) picks the launches.
#define MG_WT_FWD 1      // layer-1 forward in the phone-rate step's first launch (phone_front_gemm_kernel): H1
#define MG_WT_PAIR 4     // wgrad_dgrad_pair_kernel: dZ1 and the layer-2 slabs
// Measured one launch at a time (same box, three interleaved rounds, C2 step against 0.1057 ms with plain stores): FWD -1.5 us,
// PAIR -2.3 us; the layer-1 weight gradient -0.2 us (inside the noise: its 4-byte lanes write partial lines through), the update
// kernel +0.4 us, the layers 2-4 pass +24 us (4-byte slab values) - those three keep plain stores and carry no switch.
#define MG_WT_DEFAULT (MG_WT_FWD | MG_WT_PAIR)
static inline int mg_wt_mask(void) {
    const int ab = g_mg_tuning[MG_TUNE_AB];
    if (ab == 85) return 0;
#ifdef MG_EXPERIMENTS
    if (ab >= 300 && ab <= 300 + (MG_WT_FWD | MG_WT_PAIR)) return (ab - 300) & (MG_WT_FWD | MG_WT_PAIR);
#endif
    return MG_WT_DEFAULT;
}

#ifdef __HIPCC__
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short bf16x4 __attribute__((ext_vector_type(4)));

// float -> bf16 bits, round to nearest even; the plain cast lowers to v_cvt_pk_bf16_f32 on gfx950 and keeps NaNs.
__device__ __forceinline__ uint16_t mg_f2bf(float x) {
    __bf16 b = (__bf16)x;
    return __builtin_bit_cast(uint16_t, b);
}
__device__ __forceinline__ float mg_bf2f(uint16_t v) { return __uint_as_float(((uint32_t)v) << 16); }

__device__ __forceinline__ float mg_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
// bf16-mode sigmoid: one v_exp_f32 and one v_rcp_f32 (1 ulp each, far below the bf16 rounding of the result).  1/(1+e) through
// `/` or __frcp_rn is the IEEE division sequence (div_scale, rcp, 6 fma, div_fmas, div_fixup) and exp2f adds denormal
// handling: ~20 VALU instructions per value, which made the layer-1 forward epilogue a third of its kernel.
__device__ __forceinline__ float mg_sigmoid_fast(float x) {
    return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * -1.4426950408889634f));
}

// Epilogues of the Linear GEMM kernels (their EPI template parameter): bias (+ activation) forward, or the dgrad form
// dX = (dY W) * f'(H) with f' written in the activation's OUTPUT H: H (1 - H), 1 - H^2, H > 0.
#define EPI_BIAS 0
#define EPI_BIAS_SIGMOID 1
#define EPI_SIGMOID_GRAD 2
#define EPI_BIAS_TANH 3
#define EPI_BIAS_RELU 4
#define EPI_TANH_GRAD 5
#define EPI_RELU_GRAD 6
#define EPI_IS_GRAD(e) ((e) == EPI_SIGMOID_GRAD || (e) == EPI_TANH_GRAD || (e) == EPI_RELU_GRAD)

// One launch statement per forward / dgrad epilogue: CALL is a one-argument macro that launches its EPI instantiation.
#define MG_SWITCH_FWD_EPI(epi, CALL)                                 \
    do {                                                             \
        switch (epi) {                                               \
            case EPI_BIAS_SIGMOID: CALL(EPI_BIAS_SIGMOID); break;    \
            case EPI_BIAS_TANH: CALL(EPI_BIAS_TANH); break;          \
            case EPI_BIAS_RELU: CALL(EPI_BIAS_RELU); break;          \
            default: CALL(EPI_BIAS); break;                          \
        }                                                            \
    } while (0)
#define MG_SWITCH_GRAD_EPI(epi, CALL)                                \
    do {                                                             \
        switch (epi) {                                               \
            case EPI_TANH_GRAD: CALL(EPI_TANH_GRAD); break;          \
            case EPI_RELU_GRAD: CALL(EPI_RELU_GRAD); break;          \
            default: CALL(EPI_SIGMOID_GRAD); break;                  \
        }                                                            \
    } while (0)

static inline bool mg_act_known(int act) { return act >= MG_ACT_NONE && act <= MG_ACT_RELU; }
static inline int mg_epi_fwd(int act) {
    return act == MG_ACT_SIGMOID ? EPI_BIAS_SIGMOID : act == MG_ACT_TANH ? EPI_BIAS_TANH : act == MG_ACT_RELU ? EPI_BIAS_RELU : EPI_BIAS;
}
// the dgrad epilogue for an input that is the OUTPUT of `act` (MG_ACT_NONE: plain dX = dY W, the EPI_BIAS form without a bias)
static inline int mg_epi_grad(int act) {
    return act == MG_ACT_SIGMOID ? EPI_SIGMOID_GRAD : act == MG_ACT_TANH ? EPI_TANH_GRAD : act == MG_ACT_RELU ? EPI_RELU_GRAD : EPI_BIAS;
}

// relu as torch.relu has it (clamp_min(0)): NaN stays NaN and -0.0 stays -0.0
__device__ __forceinline__ float mg_relu(float x) { return x < 0.f ? 0.f : x; }

// z = the pre-activation (bias added).  FAST selects the hardware-exp sigmoid of the bf16 kernels.  Tanh is tanhf in every mode:
// the hardware-exp form the GRU candidate gate uses (gru_cell.h: 2 sigmoid_fast(2x) - 1) cancels near 0 - its absolute error stays
// near 2^-23 while a bf16 output rounds to |x| 2^-9, so it is above the output rounding for every |x| < 2^-14 (flushing them to
// 0) - and the bf16x3 mode runs these kernels with fp32 outputs held to 1e-4.
template <int EPI, bool FAST>
__device__ __forceinline__ float mg_epi_act(float z) {
    if (EPI == EPI_BIAS_SIGMOID) return FAST ? mg_sigmoid_fast(z) : mg_sigmoid(z);
    if (EPI == EPI_BIAS_TANH) return tanhf(z);
    if (EPI == EPI_BIAS_RELU) return mg_relu(z);
    return z;
}
// v f'(h), h the activation's output; ReLU as torch's threshold_backward (h <= 0 ? 0 : v, so a NaN h passes v on)
template <int EPI>
__device__ __forceinline__ float mg_epi_dact(float v, float h) {
    if (EPI == EPI_TANH_GRAD) return v * (1.f - h * h);
    if (EPI == EPI_RELU_GRAD) return h <= 0.f ? 0.f : v;
    return v * h * (1.f - h);
}

// The 32x32x16 bf16 MFMA of the large GEMM kernels behind one name, so that a PROBE build (make probe16 -> libmorgana_hip_probe16.so,
// -DMG_PROBE16, results garbage, never loaded by the package) can issue two v_mfma_f32_16x16x32_bf16 in its place on the same
// registers: same matrix cycles, same operand traffic, a different clock under load (MI355X_MICROARCH.md, DVFS give-back item 7).
typedef __bf16 mg_bfv8 __attribute__((ext_vector_type(8)));
#ifdef MG_PROBE16
#define MG_MFMA_PER_TILE 2
__device__ __forceinline__ f32x16 mg_mfma_32x32x16(mg_bfv8 a, mg_bfv8 b, f32x16 c) {
    f32x4 lo = {c[0], c[1], c[2], c[3]}, hi = {c[8], c[9], c[10], c[11]};
    lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, lo, 0, 0, 0);
    hi = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, a, hi, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        c[r] = lo[r];
        c[8 + r] = hi[r];
    }
    asm volatile("" : "+v"(c));                        // the other registers stay opaque: the epilogues keep all their work
    return c;
}
#else
#define MG_MFMA_PER_TILE 1
__device__ __forceinline__ f32x16 mg_mfma_32x32x16(mg_bfv8 a, mg_bfv8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
#endif

// LDS-DMA of 64 x 16 bytes: lane l's 16 bytes (from its own address `src`) land at LDS byte (wave-uniform address + 16 l); no VGPR
// staging, no ds_write, completion counted by vmcnt.  The one statement of this form in the library.  Inline asm on purpose: hipcc
// keeps no record of the pending LDS write, so it drains vmcnt neither in front of the fragment reads (it does for
// ds_read_b64_tr_b16 behind the builtin form: one s_waitcnt vmcnt(0) per step, measured) nor in front of __syncthreads; its own waits
// stay conservative - a wait for a tracked load also covers every older DMA.  What the caller owes: it drains vmcnt, with a counted
// wait of its own, before the barrier in front of the first read.  M0 is saved and restored inside the statement
// (cdna_hip_programming.md section 5.7).
//   mg_glds16_at takes the LDS address as an integer: casting a generic pointer back to the LDS address space inside a step loop
//   made hipcc emit a null check that does not assemble.  mg_glds16 takes the pointer, where that cast is harmless.
__device__ __forceinline__ void mg_glds16_at(const void* src, unsigned lds_addr) {
    const unsigned lds_uni = __builtin_amdgcn_readfirstlane(lds_addr);
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(src), "s"(lds_uni)
                 : "memory");
}
__device__ __forceinline__ void mg_glds16(const void* src, unsigned char* lds_wave_base) {
    mg_glds16_at(src, (unsigned)(unsigned long long)((__attribute__((address_space(3))) unsigned char*)lds_wave_base));
}

// Write-through stores (mg_wt_mask above): the value goes to memory with the sc1 bit, the line does not stay dirty in L2.
// 4 bytes per lane: a relaxed agent-scope atomic store (global_store_dword ... sc1), which hipcc counts in its vmcnt bookkeeping like
// any store.  16 bytes per lane: inline asm on a flat 64-bit address (the raw-buffer builtin of the recurrent kernels needs a
// wave-uniform base and 32-bit offsets: the outputs here may be larger than 4 GB), which hipcc does NOT count - the hardware's vmcnt
// counts it like a plain store (a kernel that counts vmcnt by hand keeps its numbers), a compiler wait for an older load only becomes
// conservative, and nothing reads the data back inside the launch.  s_nop 1: the next instruction must not overwrite the data
// registers early.
typedef unsigned int mg_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void mg_store_wt(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mg_store_wt16(void* p, mg_u32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
// the form chosen by a wave-uniform flag (a kernel argument)
template <typename T>
__device__ __forceinline__ void mg_store_sel(bool wt, T* p, T v) {
    if (wt) mg_store_wt(p, v); else *p = v;
}
__device__ __forceinline__ void mg_store16_sel(bool wt, void* p, mg_u32x4 v) {
    if (wt) mg_store_wt16(p, v); else *reinterpret_cast<mg_u32x4*>(p) = v;
}

// Sum over each row of 16 lanes, in every lane of the row, on the DPP path (row_ror 8, 4, 2, 1: four VALU instructions, where four
// __shfl_xor go through the LDS crossbar one after the other).  Bit for bit the xor butterfly 8, 4, 2, 1: at every level a lane's
// partner belongs to the same class of lanes either way, and a + b == b + a.
template <int CTRL>
__device__ __forceinline__ float mg_dpp_f32(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float mg_row16_sum(float v) {
    v += mg_dpp_f32<0x128>(v);
    v += mg_dpp_f32<0x124>(v);
    v += mg_dpp_f32<0x122>(v);
    v += mg_dpp_f32<0x121>(v);
    return v;
}

__device__ __forceinline__ float mg_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
#endif


// ---------------------------------------------------------------------------------------------------------------------
// In-kernel stamps (cdna_hip_programming.md section 7).  Compiled only into the DIAGNOSTIC library
// (make diag -> ../libmorgana_hip_diag.so, -DMG_STAMPS); the product library contains none of this.
// Each stamping kernel owns a file-local buffer: [block][wave 0 or 4][MG_STAMP_SLOTS] shader-clock values.
// ---------------------------------------------------------------------------------------------------------------------
#define MG_STAMP_SLOTS 16
#define MG_STAMP_BLOCKS 4096
#ifdef MG_STAMPS
#define MG_STAMP_DECL(name) __device__ unsigned long long name[MG_STAMP_BLOCKS * 2 * MG_STAMP_SLOTS]
#define MG_STAMP(var)                                                                         \
    do {                                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                    \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory");           \
        __builtin_amdgcn_sched_barrier(0);                                                    \
    } while (0)
#define MG_STAMP_REAL(var)                                                                    \
    do {                                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                    \
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory");       \
        __builtin_amdgcn_sched_barrier(0);                                                    \
    } while (0)
#define MG_STAMP_ADD(sum, t1, t0) ((sum) += (t1) - (t0))
#define MG_STAMP_STORE(buf, block, wave, lane, slot, value)                                   \
    do {                                                                                      \
        if ((block) < MG_STAMP_BLOCKS && ((wave) & 3) == 0 && (lane) == 0)                    \
            buf[((size_t)(block) * 2 + ((wave) >> 2)) * MG_STAMP_SLOTS + (slot)] = (value);   \
    } while (0)
#else
#define MG_STAMP_DECL(name)
#define MG_STAMP(var) do { } while (0)
#define MG_STAMP_REAL(var) do { } while (0)
#define MG_STAMP_ADD(sum, t1, t0) do { } while (0)
#define MG_STAMP_STORE(buf, block, wave, lane, slot, value) do { } while (0)
#endif
