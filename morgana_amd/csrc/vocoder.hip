// K32 - vocoder features: what the reference's flagship model hands to WORLD for every validation utterance (models/RNN_SPSS.py:141-161),
// up to the call of the synthesiser itself.  Three entry points, one launch each, packed outputs (float32, or the float32 value
// widened to float64 with out_f64: the arrays a WORLD-style vocoder takes need no host conversion pass):
//
//   mg_mcep_spectrum_f32     sp[r, k] = exp(2 L[r, k]),  L[r, k] = sum_{m < M} c[r, m] basis[m, k]        (log_out: 2 L itself)
//   mg_bap_aperiodicity_f32  ap[r, k] = exp(dB[r, k] ln10 / 20), dB linear between the band anchors at f_k = k fs / F
//   mg_smooth_f0_f32         f0[r]    = vuv > threshold ? (float)savgol_1(exp(lf0))[r] : 0              (float64 inside)
//
// The full rules are in include/morgana_hip.h (K32).  No cosine, no atomics, no workspace, no host read: every output element is a
// function of its item alone, computed in one fixed order - the same bits on every call, capturable.
//
// Spectrum mapping.  The output is the traffic (K = F/2 + 1 floats per frame against M cepstra), so LANES RUN ALONG BINS: a workgroup
// owns VOC_TILE_BINS = 256 consecutive bins, one per thread, and a wave's store instruction writes 64 consecutive floats (256
// contiguous bytes; 512 with out_f64).  K is odd: rows are 4-byte aligned only, so every store is one dword (qword) per lane and the
// last bin tile is a tail of K mod 256 live lanes (a wave without a live lane skips the arithmetic).  A thread keeps ITS COLUMN OF THE
// BASIS IN REGISTERS (32 MC floats, MC = ceil(M / 32) a template parameter, zero above M), loaded once per workgroup; the workgroup
// then walks row tiles of VOC_TILE_FRAMES packed rows (grid-stride over blockIdx.y).  A frame's cepstra are wave-uniform: they are
// read through a uniform pointer (scalar loads of VOC_GROUP = 8) and enter the fma as scalar operands, so a frame costs a wave about
// M fma, one expf and one store.  Scalar loads return out of order, so a wave can only wait for all of them: the groups of
// VOC_FRAMES = 2 frames share one wait (2 x 8 scalar registers is what the kernel holds without spilling: 2 x 16 and 4 x 8 spill
// scalar registers), and other waves of the SIMD cover the wait.  The group that M cuts reads the LAST 8 cepstra of the frame,
// c[r, M - 8 .. M), and takes the ones it has not counted yet (the others enter as exact zeros against zero basis registers);
// M < 8 reads element by element.  Nothing at or past c[r, M] is read.  Accumulation: fmaf in ascending m from 0, one rounding per
// term.
//
// Rows.  A row tile of a packed input reads its own rows, [offsets[0], offsets[B]).  A padded input's tile finds the source frame of
// each of its packed rows by a binary search in the items' first packed rows (mg_packed_source_row of csrc/packed_rows.h): the scanned
// clamped lengths, held in LDS, B <= MG_VOC_MAX_ITEMS.  A packed row that belongs to no item, and every row from packed_rows on, is not
// written; a frame past its item's length is never read.
//
// Smoothing mapping.  One workgroup per item (grid-stride), as csrc/f0.hip; per column the item is taken in chunks of VOC_F0_CHUNK
// frames whose y = exp((double)lf0) are staged in LDS with a halo of h = (window - 1) / 2 frames on either side, cut to the item - the
// window cannot reach a neighbouring item.  The first and last h frames of an item take the least-squares line of the item's first /
// last `window` frames, recomputed from memory by the few threads that own them (the same function of the same input).
#include "common.h"
#include "item_norm.h"
#include "packed_rows.h"

#define VOC_THREADS 256
#define VOC_TILE_BINS VOC_THREADS
#define VOC_TILE_FRAMES 32
#define VOC_GROUP 8                    // cepstra of one frame per scalar load
#define VOC_FRAMES 2                   // frames whose loads share one wait
#define VOC_TARGET_BLOCKS 1280         // five workgroups on each of 256 CUs: what the M = 60 kernel's registers admit at once
#define VOC_F0_CHUNK 256
#define VOC_MAX_HALF ((MG_VOC_MAX_WINDOW - 1) / 2)
#define VOC_F0_MAX_BLOCKS 65536

__device__ __forceinline__ int64_t voc_uniform(int64_t v) {      // a value every lane holds, moved to scalar registers
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Orders two accumulation chains: `next` starts after `done` has finished.  No instruction is emitted.  Without it the compiler
// pairs the independent chains of two frames into packed fma, whose operands must be vector registers: the frames' cepstra, scalar
// operands of a plain fma, would each be copied into one first.
__device__ __forceinline__ void voc_chain_fence(float& done, float& next) { asm volatile("" : "+v"(done), "+v"(next)); }

template <int MC, typename OutT>
__global__ __launch_bounds__(VOC_THREADS) void mcep_spectrum_kernel(const float* __restrict__ c, const float* __restrict__ basis, int64_t ldb,
                                                                    const int64_t* __restrict__ offsets, const int64_t* __restrict__ seq_len,
                                                                    int64_t T_in, int B, int M, int K, int log_out, int64_t packed_rows,
                                                                    OutT* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) int64_t s_voc[];      // a padded input only: [B + 1] first rows, [256] partials
    __shared__ int64_t s_src[VOC_TILE_FRAMES];
    const int tid = threadIdx.x;
    const int64_t rows_end = mg_packed_rows_end(offsets, seq_len, T_in, B, packed_rows, s_voc);
    const int64_t n_tiles = (rows_end + VOC_TILE_FRAMES - 1) / VOC_TILE_FRAMES;

    const int bin = blockIdx.x * VOC_TILE_BINS + tid;
    const bool live = bin < K;
    const bool wave_live = blockIdx.x * VOC_TILE_BINS + (tid & ~(MG_WAVE - 1)) < K;      // uniform for the wave
    // register m of group m0 = m - m % VOC_GROUP holds basis row m; in the group that M cuts it holds the LAST VOC_GROUP rows,
    // M - VOC_GROUP + j, with zeros where those lie below m0 (M < VOC_GROUP: row m, zeros from M on); zeros in every later group
    float bz[MC * 32];
#pragma unroll
    for (int m = 0; m < MC * 32; ++m) {
        const int m0 = m - m % VOC_GROUP;
        int row = m;
        bool ok = m < M;
        if (m0 + VOC_GROUP > M && m0 < M && M >= VOC_GROUP) {
            row = M - VOC_GROUP + m % VOC_GROUP;
            ok = row >= m0;
        }
        bz[m] = live && ok ? basis[(int64_t)row * ldb + bin] : 0.f;
    }

    for (int64_t tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
        const int64_t r_lo = tile * VOC_TILE_FRAMES;
        __syncthreads();                                       // the previous tile's readers of s_src are done
        if (tid < VOC_TILE_FRAMES) s_src[tid] = mg_packed_source_row(r_lo + tid, rows_end, B, offsets, seq_len, T_in, s_voc);
        __syncthreads();
        if (!wave_live) continue;
        for (int r = 0; r < VOC_TILE_FRAMES; r += VOC_FRAMES) {
            // VOC_FRAMES frames share each wait; a frame without a source repeats the arithmetic of one that has and stores nothing
            int64_t src[VOC_FRAMES], have = -1;
#pragma unroll
            for (int f = 0; f < VOC_FRAMES; ++f) {
                src[f] = voc_uniform(s_src[r + f]);
                if (have < 0) have = src[f];
            }
            if (have < 0) continue;
            const float* __restrict__ cr[VOC_FRAMES];
#pragma unroll
            for (int f = 0; f < VOC_FRAMES; ++f) cr[f] = c + (src[f] >= 0 ? src[f] : have) * M;
            // M as this trip's own scalar: the comparisons below stay one scalar compare each, made where they are used (hoisted
            // out of the frame loop, the 32 MC of them were kept as lane masks and spilled)
            int Mf = M;
            asm volatile("" : "+s"(Mf));
            float acc[VOC_FRAMES];
#pragma unroll
            for (int f = 0; f < VOC_FRAMES; ++f) acc[f] = 0.f;
#pragma unroll
            for (int g = 0; g < MC * 32 / VOC_GROUP; ++g) {
                const int m0 = g * VOC_GROUP;
                if (m0 + VOC_GROUP <= Mf) {
                    float cv[VOC_FRAMES][VOC_GROUP];
#pragma unroll
                    for (int f = 0; f < VOC_FRAMES; ++f) {
#pragma unroll
                        for (int j = 0; j < VOC_GROUP; ++j) cv[f][j] = cr[f][m0 + j];
                    }
#pragma unroll
                    for (int f = 0; f < VOC_FRAMES; ++f) {
#pragma unroll
                        for (int j = 0; j < VOC_GROUP; ++j) acc[f] = fmaf(cv[f][j], bz[m0 + j], acc[f]);
                        voc_chain_fence(acc[f], acc[(f + 1) % VOC_FRAMES]);
                    }
                } else if (m0 < Mf) {
                    if (Mf >= VOC_GROUP) {                     // the last VOC_GROUP cepstra; those below m0 are counted already
                        const int counted = m0 - (Mf - VOC_GROUP);
                        float cv[VOC_FRAMES][VOC_GROUP];
#pragma unroll
                        for (int f = 0; f < VOC_FRAMES; ++f) {
#pragma unroll
                            for (int j = 0; j < VOC_GROUP; ++j) cv[f][j] = cr[f][Mf - VOC_GROUP + j];
                        }
#pragma unroll
                        for (int f = 0; f < VOC_FRAMES; ++f) {
#pragma unroll
                            for (int j = 0; j < VOC_GROUP; ++j) acc[f] = fmaf(j >= counted ? cv[f][j] : 0.f, bz[m0 + j], acc[f]);
                            voc_chain_fence(acc[f], acc[(f + 1) % VOC_FRAMES]);
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < VOC_GROUP; ++j) {
                            if (m0 + j < Mf) {                 // M < VOC_GROUP: m0 is 0
#pragma unroll
                                for (int f = 0; f < VOC_FRAMES; ++f) acc[f] = fmaf(cr[f][m0 + j], bz[m0 + j], acc[f]);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int f = 0; f < VOC_FRAMES; ++f) {
                float v = 2.f * acc[f];
                if (!log_out) v = expf(v);
                if (live && src[f] >= 0) out[(r_lo + r + f) * K + bin] = (OutT)v;
            }
        }
    }
}

__device__ __forceinline__ float voc_clamp_db(float v) { return v < -60.f ? -60.f : v > 0.f ? 0.f : v; }      // a NaN stays a NaN

template <typename OutT>
__global__ __launch_bounds__(VOC_THREADS) void bap_aperiodicity_kernel(const float* __restrict__ bap, const int64_t* __restrict__ offsets,
                                                                       const int64_t* __restrict__ seq_len, int64_t T_in, int B, int Nb, int fs,
                                                                       int F, int K, int64_t packed_rows, OutT* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) int64_t s_voc[];
    __shared__ int64_t s_src[VOC_TILE_FRAMES];
    const int tid = threadIdx.x;
    const int64_t rows_end = mg_packed_rows_end(offsets, seq_len, T_in, B, packed_rows, s_voc);
    const int64_t n_tiles = (rows_end + VOC_TILE_FRAMES - 1) / VOC_TILE_FRAMES;

    const int bin = blockIdx.x * VOC_TILE_BINS + tid;
    const bool live = bin < K;
    // the bin's place between two anchors: once per thread, in float64
    const double f = (double)bin * (double)fs / (double)F;
    int seg = (int)(f / 3000.0);
    if (seg > Nb) seg = Nb;
    const double f_lo = 3000.0 * seg, f_hi = seg < Nb ? 3000.0 * (seg + 1) : 0.5 * (double)fs;
    const float w = (float)((f - f_lo) / (f_hi - f_lo));
    const float db_to_ln = 0.11512925464970228f;               // ln(10) / 20

    for (int64_t tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
        const int64_t r_lo = tile * VOC_TILE_FRAMES;
        __syncthreads();
        if (tid < VOC_TILE_FRAMES) s_src[tid] = mg_packed_source_row(r_lo + tid, rows_end, B, offsets, seq_len, T_in, s_voc);
        __syncthreads();
        if (!live) continue;
#pragma unroll 4
        for (int r = 0; r < VOC_TILE_FRAMES; ++r) {
            const int64_t src = s_src[r];
            if (src >= 0) {
                const float* __restrict__ row = bap + src * Nb;
                const float a = seg == 0 ? -60.f : voc_clamp_db(row[seg - 1]);
                const float b = seg == Nb ? 0.f : voc_clamp_db(row[seg]);
                const float db = fmaf(b - a, w, a);
                out[(r_lo + r) * K + bin] = (OutT)expf(db * db_to_ln);
            }
        }
    }
}

template <typename OutT>
__global__ __launch_bounds__(VOC_THREADS) void smooth_f0_kernel(const float* __restrict__ lf0, const float* __restrict__ vuv,
                                                                const int64_t* __restrict__ offsets, const int64_t* __restrict__ seq_len,
                                                                int64_t T_in, int B, int D, int window, float threshold, int64_t packed_rows,
                                                                OutT* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) int64_t s_voc[];
    __shared__ double s_y[VOC_F0_CHUNK + 2 * VOC_MAX_HALF];
    const int tid = threadIdx.x;
    if (!offsets) mg_clamped_length_scan(seq_len, B, T_in, s_voc, s_voc + B + 1);
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        // the item: uniform for the workgroup
        int64_t first, len;
        mg_item_rows(offsets, seq_len, T_in, b, first, len);
        const int64_t pfirst = mg_packed_first_row(b, offsets, s_voc);
        const bool smooth = window > 1 && len >= window;
        const int h = smooth ? (window - 1) / 2 : 0;
        const double den = (double)h * (double)(h + 1) * (double)(2 * h + 1) / 3.0;      // sum_j (j - h)^2, an integer
        const float* lsrc = lf0 + first * D;
        const float* vsrc = vuv + first * D;
        for (int d = 0; d < D; ++d) {
            for (int64_t t0 = 0; t0 < len; t0 += VOC_F0_CHUNK) {
                __syncthreads();                               // the previous chunk's readers of s_y are done
                for (int i = tid; i < VOC_F0_CHUNK + 2 * h; i += VOC_THREADS) {
                    const int64_t t = t0 - h + i;
                    if (t >= 0 && t < len) s_y[i] = exp((double)lsrc[t * D + d]);
                }
                __syncthreads();
                const int64_t t = t0 + tid;
                if (t >= len) continue;
                double s;
                if (!smooth) {
                    s = s_y[tid];
                } else if (t >= h && t < len - h) {
                    s = s_y[tid];
                    for (int j = 1; j <= 2 * h; ++j) s += s_y[tid + j];
                    s = s / (double)window;
                } else {
                    const int64_t base = t < h ? 0 : len - window;
                    double sum = 0.0, num = 0.0;
                    for (int j = 0; j < window; ++j) {
                        const double y = exp((double)lsrc[(base + j) * D + d]);
                        sum += y;
                        num += (double)(j - h) * y;
                    }
                    s = sum / (double)window + (double)(t - base - h) * (num / den);
                }
                const float v = vsrc[t * D + d] > threshold ? (float)s : 0.f;
                if (pfirst + t < packed_rows) out[(pfirst + t) * D + d] = (OutT)v;
            }
        }
    }
}

static dim3 voc_tile_grid(int K, int64_t packed_rows) {
    const unsigned nbt = (unsigned)((K + VOC_TILE_BINS - 1) / VOC_TILE_BINS);
    const int64_t n_tiles = (packed_rows + VOC_TILE_FRAMES - 1) / VOC_TILE_FRAMES;
    int64_t gy = VOC_TARGET_BLOCKS / nbt;
    if (gy < 1) gy = 1;
    if (gy > n_tiles) gy = n_tiles;
    return dim3(nbt, (unsigned)gy);
}

template <int MC>
static void voc_launch_spectrum(dim3 grid, size_t lds, hipStream_t stream, const float* mcep, const float* basis, int64_t ldb,
                                const int64_t* offsets, const int64_t* seq_len, int T_in, int B, int M, int K, int log_out, int out_f64,
                                int64_t packed_rows, void* out) {
    MG_SWITCH_F64(out_f64, OutT,
                  hipLaunchKernelGGL((mcep_spectrum_kernel<MC, OutT>), grid, dim3(VOC_THREADS), lds, stream, mcep, basis, ldb, offsets, seq_len,
                                     (int64_t)T_in, B, M, K, log_out ? 1 : 0, packed_rows, (OutT*)out));
}

extern "C" {

int mg_vocoder_tile_frames(void) { return VOC_TILE_FRAMES; }
int mg_vocoder_tile_bins(void) { return VOC_TILE_BINS; }
int mg_smooth_f0_chunk_rows(void) { return VOC_F0_CHUNK; }

int mg_mcep_spectrum_f32(const float* mcep, int M, int B, const int64_t* offsets, const int64_t* seq_len, int T_in, const float* basis,
                         int64_t ldb, int F, int log_out, int out_f64, int64_t packed_rows, void* out, void* stream) {
    MG_CHECK_ARG(F >= 8 && F <= 8192 && (F & (F - 1)) == 0, "mg_mcep_spectrum_f32: F=%d must be a power of two in [8, 8192]", F);
    MG_CHECK_ARG(M >= 1 && M <= MG_VOC_MAX_ORDER, "mg_mcep_spectrum_f32: M=%d cepstra outside [1, %d]", M, MG_VOC_MAX_ORDER);
    const int K = F / 2 + 1;
    MG_CHECK_ARG(ldb >= K, "mg_mcep_spectrum_f32: ldb=%lld is below the F / 2 + 1 = %d bins of a basis row", (long long)ldb, K);
    MG_CHECK_PACKED_IO("mg_mcep_spectrum_f32", "(B, T_in, D)", mcep, 0, M, K);
    MG_CHECK_ARG(basis && ((uintptr_t)basis & 3u) == 0, "mg_mcep_spectrum_f32: basis must not be NULL and 4-byte aligned");
    const dim3 grid = voc_tile_grid(K, packed_rows);
    const size_t lds = mg_packed_scan_bytes(offsets, B, VOC_THREADS);
    switch ((M + 31) / 32) {
        case 1: voc_launch_spectrum<1>(grid, lds, (hipStream_t)stream, mcep, basis, ldb, offsets, seq_len, T_in, B, M, K, log_out, out_f64, packed_rows, out); break;
        case 2: voc_launch_spectrum<2>(grid, lds, (hipStream_t)stream, mcep, basis, ldb, offsets, seq_len, T_in, B, M, K, log_out, out_f64, packed_rows, out); break;
        case 3: voc_launch_spectrum<3>(grid, lds, (hipStream_t)stream, mcep, basis, ldb, offsets, seq_len, T_in, B, M, K, log_out, out_f64, packed_rows, out); break;
        default: voc_launch_spectrum<4>(grid, lds, (hipStream_t)stream, mcep, basis, ldb, offsets, seq_len, T_in, B, M, K, log_out, out_f64, packed_rows, out); break;
    }
    MG_CHECK_LAUNCH("mg_mcep_spectrum_f32");
    return MG_OK;
}

int mg_bap_aperiodicity_f32(const float* bap, int Nb, int B, const int64_t* offsets, const int64_t* seq_len, int T_in, int fs, int F,
                            int out_f64, int64_t packed_rows, void* out, void* stream) {
    MG_CHECK_ARG(F >= 8 && F <= 8192 && (F & (F - 1)) == 0, "mg_bap_aperiodicity_f32: F=%d must be a power of two in [8, 8192]", F);
    MG_CHECK_ARG(fs > 0, "mg_bap_aperiodicity_f32: fs=%d must be positive", fs);
    MG_CHECK_ARG(Nb >= 1 && (int64_t)6000 * Nb < (int64_t)fs,
                 "mg_bap_aperiodicity_f32: Nb=%d bands of 3000 Hz must end below fs / 2 = %g Hz (and Nb >= 1)", Nb, 0.5 * fs);
    const int K = F / 2 + 1;
    MG_CHECK_PACKED_IO("mg_bap_aperiodicity_f32", "(B, T_in, D)", bap, 0, Nb, K);
    const dim3 grid = voc_tile_grid(K, packed_rows);
    const size_t lds = mg_packed_scan_bytes(offsets, B, VOC_THREADS);
    MG_SWITCH_F64(out_f64, OutT,
                  hipLaunchKernelGGL(bap_aperiodicity_kernel<OutT>, grid, dim3(VOC_THREADS), lds, (hipStream_t)stream, bap, offsets, seq_len,
                                     (int64_t)T_in, B, Nb, fs, F, K, packed_rows, (OutT*)out));
    MG_CHECK_LAUNCH("mg_bap_aperiodicity_f32");
    return MG_OK;
}

int mg_smooth_f0_f32(const float* lf0, const float* vuv, int D, int B, const int64_t* offsets, const int64_t* seq_len, int T_in, int window,
                     float threshold, int out_f64, int64_t packed_rows, void* out, void* stream) {
    MG_CHECK_ARG(D > 0, "mg_smooth_f0_f32: D=%d must be positive", D);
    MG_CHECK_ARG(window >= 1 && window <= MG_VOC_MAX_WINDOW && (window & 1), "mg_smooth_f0_f32: window=%d must be odd and in [1, %d]", window,
                 MG_VOC_MAX_WINDOW);
    MG_CHECK_ARG(threshold == threshold, "mg_smooth_f0_f32: threshold is NaN: no frame would be voiced");
    MG_CHECK_PACKED_IO("mg_smooth_f0_f32", "(B, T_in, D)", lf0, 0, D, D);
    MG_CHECK_ARG(vuv && ((uintptr_t)vuv & 3u) == 0, "mg_smooth_f0_f32: vuv must not be NULL and 4-byte aligned");
    const unsigned blocks = (unsigned)(B < VOC_F0_MAX_BLOCKS ? B : VOC_F0_MAX_BLOCKS);
    const size_t lds = mg_packed_scan_bytes(offsets, B, VOC_THREADS);
    MG_SWITCH_F64(out_f64, OutT,
                  hipLaunchKernelGGL(smooth_f0_kernel<OutT>, dim3(blocks), dim3(VOC_THREADS), lds, (hipStream_t)stream, lf0, vuv, offsets,
                                     seq_len, (int64_t)T_in, B, D, window, threshold, packed_rows, (OutT*)out));
    MG_CHECK_LAUNCH("mg_smooth_f0_f32");
    return MG_OK;
}

}  // extern "C"
