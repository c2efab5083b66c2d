// K33 - vocoder analysis: the opposite direction of K32 (csrc/vocoder.hip).  What an analyser such as WORLD gives for an utterance - a
// power spectrum and a full-band aperiodicity, F / 2 + 1 bins per frame, usually float64 - coded into the mel-cepstrum and the band
// aperiodicity the acoustic models are trained on.  Two entry points, one launch each, packed outputs:
//
//   mg_spectrum_mcep      c[r, m]   = sum_{k < K} table[m, k] * 0.5 log(sp[r, k])      float64 throughout, stored as float or double
//   mg_aperiodicity_bap   bap[r, b] = dB(k0) + (dB(k0 + 1) - dB(k0)) w,  dB = clamp(20 log10(ap), -60, 0) at the bins around 3000 (b + 1) Hz
//
// The full rules are in include/morgana_hip.h (K33).  No cosine, no recursion, no atomics, no workspace, no host read: every output
// element is a function of its own frame, computed in one fixed order - the same bits on every call, capturable.
//
// Mel-cepstrum mapping.  The input is the traffic (K float64 per frame against M <= 128 results) and every bin costs one float64
// logarithm, so the logarithm is taken ONCE PER BIN and the contraction runs on the float64 matrix unit.  A workgroup of four waves
// owns ANA_TILE_FRAMES = 64 packed rows (grid-stride over row tiles), a wave 16 of them and all MT = ceil(M / 16) column tiles:
// MT x 4 float64 accumulators per lane.  The contraction walks K in chunks of ANA_KC = 16 bins.  Per chunk the workgroup stages
//   s_l[64][16]       l = 0.5 log(x) of its rows: thread (tid >> 4) + 16 j, bin tid & 15 - 16 consecutive bins of a row per 16 lanes,
//   s_t[16 MT][16]    the table's chunk (it does not fit LDS whole: 60 x 1025 x 8 B = 492 KB; it stays in L2),
// and every wave then issues 4 k-steps x MT v_mfma_f64_16x16x4_f64: A[frame i][k] = s_l, B[k][m] = s_t, one float64 per lane each,
// lane = 16 k + i.  Both LDS rows are ANA_LD = 18 doubles apart: 36 dwords, so the 16 rows of a half-wave read start in 16 different
// groups of four banks.  The next chunk's global loads are issued before the matrix instructions of this one and written to LDS after
// them (registers are the second buffer).
//   K is odd: rows are aligned to one element only, so every load is one element per lane, and the last chunk has ANA_KC - 1 dead
//   bins.  A dead bin (k >= K), a dead frame (a packed row of no item) and a dead table row (m >= M) are NOT LOADED and enter as
//   exact zeros on BOTH operands: a zero table entry times a NaN of the next row would be NaN.
// Accumulator layout of the f64 instruction: lane holds rows (lane >> 4) + 4 reg, column lane & 15 - a store instruction writes 16
// consecutive coefficients of four frames.
//
// Rows.  As K32: a packed input's tile reads its own rows, [offsets[0], offsets[B]); a padded input's tile finds the source frame of
// each packed row by a binary search in the scanned clamped lengths, held in LDS (B <= MG_VOC_MAX_ITEMS): the helpers of
// csrc/packed_rows.h.
//
// Aperiodicity mapping.  One thread per (packed row, band), grid-stride: two strided loads, two log10, one store.
#include "common.h"
#include "packed_rows.h"

#define ANA_THREADS 256
#define ANA_TILE_FRAMES 64             // packed rows of a workgroup's tile: 16 per wave
#define ANA_KC 16                      // bins per staged chunk: four k-steps of the 16x16x4 instruction
#define ANA_LD 18                      // doubles between LDS rows
#define ANA_ROWS_PER_THREAD (ANA_TILE_FRAMES * ANA_KC / ANA_THREADS)
#define ANA_MAX_BLOCKS 2048            // eight workgroups a CU: what the LDS of the M <= 64 kernel admits at once
#define ANA_BAP_MAX_BLOCKS 4096

typedef double ana_double4 __attribute__((ext_vector_type(4)));

template <int MT, typename InT, typename OutT>
__global__ __launch_bounds__(ANA_THREADS) void spectrum_mcep_kernel(const InT* __restrict__ sp, const double* __restrict__ table, int64_t ldt,
                                                                    const int64_t* __restrict__ offsets, const int64_t* __restrict__ seq_len,
                                                                    int64_t T_in, int B, int M, int K, int log_in, int64_t packed_rows,
                                                                    OutT* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) int64_t s_ana[];      // a padded input only: [B + 1] first rows, [256] partials
    __shared__ double s_l[ANA_TILE_FRAMES * ANA_LD];
    __shared__ double s_t[MT * 16 * ANA_LD];
    __shared__ int64_t s_src[ANA_TILE_FRAMES];
    const int tid = threadIdx.x;
    const int lane = tid & (MG_WAVE - 1), wave = tid / MG_WAVE;
    const int64_t rows_end = mg_packed_rows_end(offsets, seq_len, T_in, B, packed_rows, s_ana);
    const int64_t n_tiles = (rows_end + ANA_TILE_FRAMES - 1) / ANA_TILE_FRAMES;
    const int n_chunks = (K + ANA_KC - 1) / ANA_KC;

    // staging: this thread's bin of a chunk, its rows of the frame tile and of the table
    const int kk = tid & (ANA_KC - 1), row0 = tid / ANA_KC;   // rows row0 + 16 j
    // the matrix instruction: lane = 16 k + i holds A[i][k] and B[k][i]
    const int mi = lane & 15, mk = lane >> 4;

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r_lo = tile * ANA_TILE_FRAMES;
        __syncthreads();                                       // the previous tile's readers of s_src, s_l and s_t are done
        if (tid < ANA_TILE_FRAMES) s_src[tid] = mg_packed_source_row(r_lo + tid, rows_end, B, offsets, seq_len, T_in, s_ana);
        __syncthreads();
        const InT* __restrict__ xrow[ANA_ROWS_PER_THREAD];
#pragma unroll
        for (int j = 0; j < ANA_ROWS_PER_THREAD; ++j) {
            const int64_t src = s_src[row0 + 16 * j];
            xrow[j] = src >= 0 ? sp + src * K : nullptr;
        }

        ana_double4 acc[MT];
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = ana_double4{0.0, 0.0, 0.0, 0.0};

        InT xn[ANA_ROWS_PER_THREAD];
        double tn[MT];
        bool k_live = kk < K;
        // a dead slot is not loaded: its operand is an exact zero.  1 is the value whose logarithm is that zero.
#pragma unroll
        for (int j = 0; j < ANA_ROWS_PER_THREAD; ++j) xn[j] = k_live && xrow[j] ? xrow[j][kk] : (InT)(log_in ? 0 : 1);
#pragma unroll
        for (int t = 0; t < MT; ++t) tn[t] = k_live && row0 + 16 * t < M ? table[(int64_t)(row0 + 16 * t) * ldt + kk] : 0.0;

        for (int ch = 0; ch < n_chunks; ++ch) {
            if (ch) __syncthreads();                           // the previous chunk's readers are done
#pragma unroll
            for (int j = 0; j < ANA_ROWS_PER_THREAD; ++j) {
                double l = 0.0;
                if (k_live && xrow[j]) l = 0.5 * (log_in ? (double)xn[j] : log((double)xn[j]));
                s_l[(row0 + 16 * j) * ANA_LD + kk] = l;
            }
#pragma unroll
            for (int t = 0; t < MT; ++t) s_t[(row0 + 16 * t) * ANA_LD + kk] = tn[t];
            __syncthreads();
            if (ch + 1 < n_chunks) {
                const int k = (ch + 1) * ANA_KC + kk;
                k_live = k < K;
#pragma unroll
                for (int j = 0; j < ANA_ROWS_PER_THREAD; ++j) xn[j] = k_live && xrow[j] ? xrow[j][k] : (InT)(log_in ? 0 : 1);
#pragma unroll
                for (int t = 0; t < MT; ++t) tn[t] = k_live && row0 + 16 * t < M ? table[(int64_t)(row0 + 16 * t) * ldt + k] : 0.0;
            }
#pragma unroll
            for (int s = 0; s < ANA_KC / 4; ++s) {
                const double a = s_l[(wave * 16 + mi) * ANA_LD + 4 * s + mk];
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    const double b = s_t[(t * 16 + mi) * ANA_LD + 4 * s + mk];
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
                }
            }
        }

        // lane holds frames (lane >> 4) + 4 reg of its wave's sixteen, coefficient 16 t + (lane & 15)
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int m = t * 16 + mi;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int f = wave * 16 + mk + 4 * reg;
                if (m < M && s_src[f] >= 0) out[(r_lo + f) * M + m] = (OutT)acc[t][reg];
            }
        }
    }
}

__device__ __forceinline__ double ana_db(double ap) {         // a NaN stays a NaN; 0 gives -60
    const double v = 20.0 * log10(ap);
    return v < -60.0 ? -60.0 : v > 0.0 ? 0.0 : v;
}

template <typename InT, typename OutT>
__global__ __launch_bounds__(ANA_THREADS) void aperiodicity_bap_kernel(const InT* __restrict__ ap, const int64_t* __restrict__ offsets,
                                                                       const int64_t* __restrict__ seq_len, int64_t T_in, int B, int Nb, int fs,
                                                                       int F, int K, int64_t packed_rows, OutT* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) int64_t s_ana[];
    const int64_t rows_end = mg_packed_rows_end(offsets, seq_len, T_in, B, packed_rows, s_ana);
    const int64_t n = rows_end * Nb;
    for (int64_t e = (int64_t)blockIdx.x * ANA_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * ANA_THREADS) {
        const int64_t r = e / Nb;
        const int b = (int)(e - r * Nb);
        const int64_t src = mg_packed_source_row(r, rows_end, B, offsets, seq_len, T_in, s_ana);
        if (src < 0) continue;
        const int64_t pos = (int64_t)3000 * (b + 1) * F;       // the anchor's bin position times fs: below 2^30 * 2^13
        const int64_t k0 = pos / fs;                          // k0 + 1 <= F / 2: the anchor lies below fs / 2
        const double w = (double)(pos - k0 * fs) / (double)fs;
        const InT* __restrict__ row = ap + src * K;
        const double lo = ana_db((double)row[k0]), hi = ana_db((double)row[k0 + 1]);
        out[e] = (OutT)fma(hi - lo, w, lo);
    }
}

template <int MT>
static void ana_launch_mcep(int in_f64, dim3 grid, size_t lds, hipStream_t stream, const void* sp, const double* table, int64_t ldt,
                            const int64_t* offsets, const int64_t* seq_len, int T_in, int B, int M, int K, int log_in, int out_f64,
                            int64_t packed_rows, void* out) {
#define ANA_GO hipLaunchKernelGGL((spectrum_mcep_kernel<MT, InT, OutT>), grid, dim3(ANA_THREADS), lds, stream, (const InT*)sp, table, ldt, \
                                  offsets, seq_len, (int64_t)T_in, B, M, K, log_in ? 1 : 0, packed_rows, (OutT*)out)
    MG_SWITCH_F64(in_f64, InT, MG_SWITCH_F64(out_f64, OutT, ANA_GO));
#undef ANA_GO
}

extern "C" {

int mg_analysis_tile_frames(void) { return ANA_TILE_FRAMES; }

int mg_spectrum_mcep(const void* sp, int in_f64, int log_in, int F, int B, const int64_t* offsets, const int64_t* seq_len, int T_in,
                     const double* table, int64_t ldt, int M, int out_f64, int64_t packed_rows, void* out, void* stream) {
    MG_CHECK_ARG(F >= 8 && F <= 8192 && (F & (F - 1)) == 0, "mg_spectrum_mcep: F=%d must be a power of two in [8, 8192]", F);
    MG_CHECK_ARG(M >= 1 && M <= MG_VOC_MAX_ORDER, "mg_spectrum_mcep: M=%d coefficients outside [1, %d]", M, MG_VOC_MAX_ORDER);
    const int K = F / 2 + 1;
    MG_CHECK_ARG(ldt >= K, "mg_spectrum_mcep: ldt=%lld is below the F / 2 + 1 = %d bins of a table row", (long long)ldt, K);
    MG_CHECK_PACKED_IO("mg_spectrum_mcep", "(B, T_in, K)", sp, in_f64, K, M);
    MG_CHECK_ARG(table && ((uintptr_t)table & 7u) == 0, "mg_spectrum_mcep: table must not be NULL and 8-byte aligned");
    const int64_t n_tiles = (packed_rows + ANA_TILE_FRAMES - 1) / ANA_TILE_FRAMES;
    const dim3 grid((unsigned)(n_tiles < ANA_MAX_BLOCKS ? n_tiles : ANA_MAX_BLOCKS));
    const size_t lds = mg_packed_scan_bytes(offsets, B, ANA_THREADS);
    const hipStream_t s = (hipStream_t)stream;
    const int mt = (M + 15) / 16;
    if (mt <= 1) ana_launch_mcep<1>(in_f64, grid, lds, s, sp, table, ldt, offsets, seq_len, T_in, B, M, K, log_in, out_f64, packed_rows, out);
    else if (mt <= 2) ana_launch_mcep<2>(in_f64, grid, lds, s, sp, table, ldt, offsets, seq_len, T_in, B, M, K, log_in, out_f64, packed_rows, out);
    else if (mt <= 4) ana_launch_mcep<4>(in_f64, grid, lds, s, sp, table, ldt, offsets, seq_len, T_in, B, M, K, log_in, out_f64, packed_rows, out);
    else ana_launch_mcep<8>(in_f64, grid, lds, s, sp, table, ldt, offsets, seq_len, T_in, B, M, K, log_in, out_f64, packed_rows, out);
    MG_CHECK_LAUNCH("mg_spectrum_mcep");
    return MG_OK;
}

int mg_aperiodicity_bap(const void* ap, int in_f64, int F, int fs, int Nb, int B, const int64_t* offsets, const int64_t* seq_len,
                        int T_in, int out_f64, int64_t packed_rows, void* out, void* stream) {
    MG_CHECK_ARG(F >= 8 && F <= 8192 && (F & (F - 1)) == 0, "mg_aperiodicity_bap: F=%d must be a power of two in [8, 8192]", F);
    MG_CHECK_ARG(fs > 0, "mg_aperiodicity_bap: fs=%d must be positive", fs);
    MG_CHECK_ARG(Nb >= 1 && (int64_t)6000 * Nb < (int64_t)fs,
                 "mg_aperiodicity_bap: Nb=%d bands of 3000 Hz must end below fs / 2 = %g Hz (and Nb >= 1)", Nb, 0.5 * fs);
    const int K = F / 2 + 1;
    MG_CHECK_PACKED_IO("mg_aperiodicity_bap", "(B, T_in, K)", ap, in_f64, K, Nb);
    const int64_t n_blocks = (packed_rows * Nb + ANA_THREADS - 1) / ANA_THREADS;
    const dim3 grid((unsigned)(n_blocks < ANA_BAP_MAX_BLOCKS ? n_blocks : ANA_BAP_MAX_BLOCKS));
    const size_t lds = mg_packed_scan_bytes(offsets, B, ANA_THREADS);
#define ANA_GO hipLaunchKernelGGL((aperiodicity_bap_kernel<InT, OutT>), grid, dim3(ANA_THREADS), lds, (hipStream_t)stream, (const InT*)ap, \
                                  offsets, seq_len, (int64_t)T_in, B, Nb, fs, F, K, packed_rows, (OutT*)out)
    MG_SWITCH_F64(in_f64, InT, MG_SWITCH_F64(out_f64, OutT, ANA_GO));
#undef ANA_GO
    MG_CHECK_LAUNCH("mg_aperiodicity_bap");
    return MG_OK;
}

}  // extern "C"
