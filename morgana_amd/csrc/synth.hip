// K34 - WORLD-style waveform synthesis: the step behind K32 (csrc/vocoder.hip).  An utterance's f0 (n,), power spectrum sp (n, K) and
// aperiodicity ap (n, K), K = F / 2 + 1, become N = floor((n - 1) S) + 1 samples, S = fs * frame_period / 1000 samples per frame.
// The definition is in include/morgana_hip.h (K34) and, as NumPy float64, in tests/synth_ref64.py.  Four entry points:
//
//   mg_synth_noise        z[i] = N(0, 1) of (seed, site, counter, i) for the packed sample range (philox_noise.h)
//   mg_synth_pulses       per utterance: the pulse positions i_m from an int64 phase scan of the sample-rate F0, the fractional
//                         position delta_m, the interval T_m and the voiced flag; the per-utterance count
//   mg_synth_responses    per pulse of a pulse range: x_m (F float64) = sqrt(T_m) * (periodic response, DC removed) + shaped noise
//   mg_synth_overlap_add  per sample: y[i] += the covering x_m of the range in ascending m; the cast on the last range
//
// Contraction is off (the NumPy restatement has none): the integer decisions - voicing, the phase increments, the frame pair and the
// weight of a pulse - come out the same on host and device, and the interpolated envelope is the reference's bit for bit.
//
// Pulses.  One workgroup per utterance walks the samples in chunks of SY_THREADS, thread = sample: inc(i) = llrint(f(i) 2^32 / fs), an
// inclusive int64 sum scan on the carried phase (the pattern of durations.hip), a pulse where the high word moves on.  A wave's pulses
// are counted by ballot, placed by the prefix count of the lanes below, the waves before and the chunks before: ascending order
// without a sort.  T_m is written by a second walk over the stored indices.  All integer: the same pulses on every call.
//
// Responses.  One workgroup per pulse.  Every real transform of size F is half of a complex transform of size F in LDS - two real
// sequences ride in the real and the imaginary part - so a pulse costs four complex transforms:
//   B <- fft(e)                         the noise segment z[i_m .. i_m + T_m), zero up to F
//   A <- ifft(Lp + i La)                the two half log spectra, Hermitian-extended: real cepstra cp (real part) and ca (imaginary)
//   A <- fft(fold(cp) + i fold(ca))     split by symmetry into the two complex cepstral spectra Cp, Ca
//   A <- ifft(W),  W = H + i (E G)      H = exp(Cp) e^{2 pi i k delta / F}, G = exp(Ca), both Hermitian-extended: h (real), noise (imaginary)
// The transform is radix 2, decimation in time, in place behind a bit-reversal pass; the twiddles (cos, sin)(2 pi k / F), k < F / 2,
// and the normalised DC-removal window d come from the caller's float64 table (ops.synth_table): the kernel calls sincos only for
// exp of a complex cepstrum and for the delta phase.  LDS per workgroup: two complex float64 arrays, 32 F bytes (SY_LDS_BYTES) -
// 32 KiB at F = 1024 (four workgroups a CU of 160 KiB), 64 KiB at 2048 (two), 128 KiB at 4096 (one).
//
// Overlap-add.  One thread per packed sample: its utterance by a binary search in the sample offsets, the first covering pulse of the
// range by a binary search in the utterance's pulse indices, then acc = y[i]; acc += x_m[...] in ascending m; y[i] = acc.  The
// additions happen one at a time in m order whatever the ranges are, so the bits do not depend on the workspace budget.  No atomics.
#include "common.h"
#include "philox_noise.h"

#pragma clang fp contract(off)

#define SY_THREADS 256
#define SY_WAVES (SY_THREADS / 64)
#define SY_NOISE_MAX_BLOCKS 4096
#define SY_LDS_BYTES(F) ((size_t)32 * (size_t)(F))

// Inclusive int64 sum scan of one value per thread over the workgroup (dq_block_scan of durations.hip); `all`: the workgroup's sum.
__device__ __forceinline__ int64_t sy_block_scan(int64_t v, int64_t* wave_tot, int64_t& all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t o = __shfl_up((long long)v, off);
        if (lane >= off) v += o;
    }
    __syncthreads();                                      // the previous readers of wave_tot are done
    if (lane == 63) wave_tot[wave] = v;
    __syncthreads();
    int64_t before = 0;
    all = 0;
    for (int w = 0; w < SY_WAVES; ++w) {
        const int64_t t = wave_tot[w];
        if (w < wave) before += t;
        all += t;
    }
    return before + v;
}

// The frame pair and the weight of position u (in frames) of an utterance of n >= 1 frames: j = min(floor(u), n - 1), j1, w = u - j.
__device__ __forceinline__ void sy_frame_pair(double u, int64_t n, int64_t& j, int64_t& j1, double& w) {
    j = (int64_t)floor(u);
    if (j > n - 1) j = n - 1;
    j1 = j + 1 < n - 1 ? j + 1 : n - 1;
    w = u - (double)j;
}

// b with offsets[b] <= x < offsets[b + 1] (offsets ascending, x < offsets[B]): empty items are stepped over
__device__ __forceinline__ int sy_item_of(const int64_t* __restrict__ offsets, int B, int64_t x) {
    int lo = 0, hi = B;                                   // the answer lies in [lo, hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(SY_THREADS) void synth_noise_kernel(double* __restrict__ z, int64_t n, unsigned seed_lo, unsigned seed_hi,
                                                                 unsigned site, const unsigned long long* __restrict__ counter) {
    const unsigned long long ctr = counter[0];
    for (int64_t i = (int64_t)blockIdx.x * SY_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SY_THREADS)
        z[i] = (double)smp_normal(i, ctr, site, seed_lo, seed_hi);
}

__global__ __launch_bounds__(SY_THREADS) void synth_pulses_kernel(const double* __restrict__ f0, const int64_t* __restrict__ frame_start,
                                                                  const int64_t* __restrict__ n_frames,
                                                                  const int64_t* __restrict__ sample_offsets,
                                                                  const int64_t* __restrict__ region_offsets, double S, double f_lo,
                                                                  double f_hi, double inc_scale, int32_t* __restrict__ pulse_idx,
                                                                  double* __restrict__ pulse_delta, int32_t* __restrict__ pulse_T,
                                                                  int32_t* __restrict__ pulse_voiced, int64_t* __restrict__ counts) {
    __shared__ int64_t wave_tot[SY_WAVES];
    __shared__ int wave_cnt[SY_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int64_t n = n_frames[b];
    if (n < 2) return;                                    // uniform: nothing is written, the caller's count stays 0
    const int64_t N = sample_offsets[b + 1] - sample_offsets[b];
    const int64_t cap = region_offsets[b + 1] - region_offsets[b];
    const double* __restrict__ f = f0 + frame_start[b];
    int32_t* __restrict__ idx = pulse_idx + region_offsets[b];
    double* __restrict__ dlt = pulse_delta + region_offsets[b];
    int32_t* __restrict__ vcd = pulse_voiced + region_offsets[b];
    int64_t carry_phi = 0, carry_cnt = 0;                 // the same in every thread
    for (int64_t c0 = 0; c0 < N; c0 += SY_THREADS) {
        const int64_t i = c0 + tid;
        const bool live = i < N;
        int64_t inc = 0;
        bool voiced = false;
        if (live) {
            int64_t j, j1;
            double w;
            sy_frame_pair((double)i / S, n, j, j1, w);
            const double a0 = f[j], a1 = f[j1];
            const bool v0 = a0 > 0.0, v1 = a1 > 0.0;
            voiced = w < 0.5 ? v0 : (w > 0.5 ? v1 : (v0 && v1));
            double x = 500.0;
            if (voiced) {
                const double g0 = v0 ? a0 : 500.0, g1 = v1 ? a1 : 500.0;
                x = g0 + (g1 - g0) * w;
                if (!(x >= f_lo)) x = f_lo;               // also what a non-finite f0 is given
                if (x > f_hi) x = f_hi;
            }
            inc = (int64_t)llrint(x * inc_scale);         // ties to even; in [2^32 / F, 2^31]
        }
        int64_t chunk_phi;
        const int64_t phi = carry_phi + sy_block_scan(inc, wave_tot, chunk_phi);
        const bool pulse = live && (phi >> 32) > ((phi - inc) >> 32);
        const unsigned long long mask = __ballot(pulse);
        const int below = __popcll(mask & ((1ull << lane) - 1ull));
        __syncthreads();                                  // the previous readers of wave_cnt are done
        if (lane == 0) wave_cnt[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < SY_WAVES; ++w) {
            if (w < wave) before += wave_cnt[w];
            all += wave_cnt[w];
        }
        if (pulse) {
            const int64_t m = carry_cnt + before + below;
            if (m < cap) {                                // always: at most one pulse per two samples, cap = N / 2 + 1
                idx[m] = (int32_t)i;
                dlt[m] = (double)(phi & 0xFFFFFFFFll) / (double)inc;
                vcd[m] = voiced ? 1 : 0;
            }
        }
        carry_cnt += all;
        carry_phi += chunk_phi;
    }
    const int64_t count = carry_cnt < cap ? carry_cnt : cap;
    __syncthreads();                                      // the indices of every chunk are written
    int32_t* __restrict__ len = pulse_T + region_offsets[b];
    for (int64_t m = tid; m < count; m += SY_THREADS) len[m] = (int32_t)((m + 1 < count ? (int64_t)idx[m + 1] : N) - (int64_t)idx[m]);
    if (tid == 0) counts[b] = count;
}

// In-place complex transform of size F = 2^logF in LDS, all SY_THREADS threads: bit reversal, then logF radix-2 stages.  Forward:
// X[k] = sum_t x[t] e^{-2 pi i k t / F}; inverse: the conjugate twiddles, NOT scaled (the caller multiplies by the exact 1 / F).
// tw[2 q], tw[2 q + 1] = cos, sin of 2 pi q / F, q < F / 2.  Ends with a barrier.
__device__ __forceinline__ void sy_fft(double* __restrict__ re, double* __restrict__ im, int F, int logF, const double* __restrict__ tw,
                                       bool inverse) {
    const int tid = threadIdx.x;
    __syncthreads();                                      // the array is complete
    for (int i = tid; i < F; i += SY_THREADS) {
        const int j = (int)(__brev((unsigned)i) >> (32 - logF));
        if (i < j) {
            const double r = re[i], q = im[i];
            re[i] = re[j], im[i] = im[j];
            re[j] = r, im[j] = q;
        }
    }
    __syncthreads();
    for (int s = 0; s < logF; ++s) {
        const int h = 1 << s, step = F >> (s + 1);
        for (int t = tid; t < (F >> 1); t += SY_THREADS) {
            const int q = t & (h - 1);
            const int lo = ((t >> s) << (s + 1)) + q, hi = lo + h;
            const double wr = tw[2 * q * step], ws = tw[2 * q * step + 1];
            const double wi = inverse ? ws : -ws;
            const double br = re[hi], bi = im[hi];
            const double tr = br * wr - bi * wi, ti = br * wi + bi * wr;
            const double ar = re[lo], ai = im[lo];
            re[lo] = ar + tr, im[lo] = ai + ti;
            re[hi] = ar - tr, im[hi] = ai - ti;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ double sy_load(const void* __restrict__ p, int f64, int64_t i) {
    return f64 ? ((const double*)p)[i] : (double)((const float*)p)[i];
}

__global__ __launch_bounds__(SY_THREADS) void synth_responses_kernel(
    const void* __restrict__ sp, int sp_f64, const void* __restrict__ ap, int ap_f64, int B, const int64_t* __restrict__ frame_start,
    const int64_t* __restrict__ n_frames, const int64_t* __restrict__ sample_offsets, const int64_t* __restrict__ region_offsets,
    const int64_t* __restrict__ pulse_offsets, const int32_t* __restrict__ pulse_idx, const double* __restrict__ pulse_delta,
    const int32_t* __restrict__ pulse_T, const int32_t* __restrict__ pulse_voiced, const double* __restrict__ z,
    const double* __restrict__ table, double S, int F, int logF, int64_t g_lo, double* __restrict__ workspace) {
    extern __shared__ __attribute__((aligned(16))) double sy_lds[];
    __shared__ double s_part[SY_WAVES];
    double* __restrict__ a_re = sy_lds;
    double* __restrict__ a_im = sy_lds + F;
    double* __restrict__ b_re = sy_lds + 2 * F;
    double* __restrict__ b_im = sy_lds + 3 * F;
    const double* __restrict__ tw = table;                // (cos, sin) pairs, F / 2 of them
    const double* __restrict__ dc = table + F;            // d[p], F of them
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = F >> 1, K = half + 1;
    const double inv_F = 1.0 / (double)F;                 // exact

    const int64_t g = g_lo + blockIdx.x;                  // < pulse_offsets[B]: the grid is the range
    const int b = sy_item_of(pulse_offsets, B, g);
    const int64_t slot = region_offsets[b] + (g - pulse_offsets[b]);
    const int64_t i_m = pulse_idx[slot];
    const double delta = pulse_delta[slot];
    int T = pulse_T[slot];
    if (T > F) T = F;                                     // never: f >= fs / F
    const bool voiced = pulse_voiced[slot] != 0;
    const int64_t n = n_frames[b];
    double u = ((double)i_m - delta) / S;
    if (u < 0.0) u = 0.0;
    if (u > (double)(n - 1)) u = (double)(n - 1);
    int64_t j, j1;
    double w;
    sy_frame_pair(u, n, j, j1, w);
    const int64_t row0 = (frame_start[b] + j) * K, row1 = (frame_start[b] + j1) * K;

    // B <- fft(e)
    const double* __restrict__ zi = z + sample_offsets[b] + i_m;
    for (int t = tid; t < F; t += SY_THREADS) {
        b_re[t] = t < T ? zi[t] : 0.0;
        b_im[t] = 0.0;
    }
    sy_fft(b_re, b_im, F, logF, tw, false);

    // A <- the half log spectra (periodic in the real part, aperiodic in the imaginary part), Hermitian-extended
    for (int k = tid; k < K; k += SY_THREADS) {
        const double s0 = sy_load(sp, sp_f64, row0 + k), s1 = sy_load(sp, sp_f64, row1 + k);
        const double a0 = sy_load(ap, ap_f64, row0 + k), a1 = sy_load(ap, ap_f64, row1 + k);
        double s = s0 + (s1 - s0) * w;
        if (s < 0.0) s = 0.0;                             // a NaN stays a NaN
        const double a = a0 + (a1 - a0) * w;
        double r = a * a;
        if (r < 0.0) r = 0.0;
        if (r > 1.0) r = 1.0;
        double lp = 0.0, la;
        if (voiced) {
            lp = 0.5 * log(s * (1.0 - r) + 1e-12);
            la = 0.5 * log(s * r + 1e-12);
        } else {
            la = 0.5 * log(s + 1e-12 + 0.0 * r);          // 0 r: the bits of s + 1e-12, and a NaN aperiodicity reaches the response
        }
        a_re[k] = lp, a_im[k] = la;
        if (k > 0 && k < half) a_re[F - k] = lp, a_im[F - k] = la;
    }
    sy_fft(a_re, a_im, F, logF, tw, true);
    // fold: the cepstra times 1 / F, doubled inside (0, F / 2), zero above F / 2
    for (int q = tid; q < F; q += SY_THREADS) {
        const double f = (q == 0 || q == half) ? inv_F : (q < half ? 2.0 * inv_F : 0.0);
        a_re[q] = q > half ? 0.0 : a_re[q] * f;
        a_im[q] = q > half ? 0.0 : a_im[q] * f;
    }
    sy_fft(a_re, a_im, F, logF, tw, false);

    // the two spectra apart, exp, the delta phase, the noise spectrum times G; W = H + i (E G) in place, pair (k, F - k) per thread
    const double phase = 6.283185307179586 * delta * inv_F;
    for (int k = tid; k < K; k += SY_THREADS) {
        const int kc = (F - k) & (F - 1);
        const double zr = a_re[k], zq = a_im[k], yr = a_re[kc], yq = -a_im[kc];      // Z[k], conj(Z[F - k])
        const double cpr = 0.5 * (zr + yr), cpi = 0.5 * (zq + yq);                   // Cp = (Z[k] + conj(Z[F - k])) / 2
        const double car = 0.5 * (zq - yq), cai = -0.5 * (zr - yr);                  // Ca = (Z[k] - conj(Z[F - k])) / 2i
        double hr = 0.0, hi = 0.0;
        if (voiced) {
            double sn, cs, ps, pc;
            sincos(cpi, &sn, &cs);
            sincos(phase * (double)k, &ps, &pc);
            const double mag = exp(cpr);
            const double r0 = mag * cs, q0 = mag * sn;
            hr = r0 * pc - q0 * ps;
            hi = r0 * ps + q0 * pc;
        }
        double sn, cs;
        sincos(cai, &sn, &cs);
        const double mag = exp(car);
        const double gr = mag * cs, gi = mag * sn;
        const double er = b_re[k], ei = b_im[k];
        double xr = er * gr - ei * gi, xi = er * gi + ei * gr;
        if (k == 0 || k == half) hi = 0.0, xi = 0.0;      // irfft drops the imaginary part of bins 0 and F / 2
        a_re[k] = hr - xi, a_im[k] = hi + xr;
        if (kc != k) a_re[kc] = hr + xi, a_im[kc] = xr - hi;
    }
    sy_fft(a_re, a_im, F, logF, tw, true);

    // the sum of the periodic response, in one fixed order
    double part = 0.0;
    for (int t = tid; t < F; t += SY_THREADS) part += a_re[t] * inv_F;
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    if (lane == 0) s_part[wave] = part;
    __syncthreads();
    double total = 0.0;
    for (int v = 0; v < SY_WAVES; ++v) total += s_part[v];

    const double scale = sqrt((double)T);
    double* __restrict__ out = workspace + (int64_t)blockIdx.x * F;
    for (int p = tid; p < F; p += SY_THREADS) {
        const int t = (p - half + 1) & (F - 1);
        double x = a_im[t] * inv_F;
        if (voiced) x = (a_re[t] * inv_F - dc[p] * total) * scale + x;
        out[p] = x;
    }
}

template <typename OutT>
__global__ __launch_bounds__(SY_THREADS) void synth_overlap_add_kernel(const double* __restrict__ workspace, int B,
                                                                       const int64_t* __restrict__ sample_offsets,
                                                                       const int64_t* __restrict__ region_offsets,
                                                                       const int64_t* __restrict__ pulse_offsets,
                                                                       const int32_t* __restrict__ pulse_idx, int F, int64_t g_lo,
                                                                       int64_t g_hi, int64_t total_samples, double* __restrict__ y, int last,
                                                                       OutT* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * SY_THREADS + threadIdx.x;
    if (s >= total_samples) return;
    const int b = sy_item_of(sample_offsets, B, s);
    const int64_t i = s - sample_offsets[b];
    const int64_t p0 = pulse_offsets[b], p1 = pulse_offsets[b + 1];
    int64_t m_lo = (g_lo > p0 ? g_lo : p0) - p0, m_hi = (g_hi < p1 ? g_hi : p1) - p0;      // the utterance's pulses of this range
    double acc = y[s];
    if (m_lo < m_hi) {
        const int32_t* __restrict__ idx = pulse_idx + region_offsets[b];
        const int half = F >> 1;
        const int64_t first = i - half, past = i + half;   // covering pulses: first <= i_m < past
        int64_t lo = m_lo, hi = m_hi;                      // the first m in [m_lo, m_hi) with idx[m] >= first
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)idx[mid] < first) lo = mid + 1; else hi = mid;
        }
        for (int64_t m = lo; m < m_hi && (int64_t)idx[m] < past; ++m)
            acc += workspace[(p0 + m - g_lo) * F + (i - (int64_t)idx[m] + half - 1)];
        y[s] = acc;
    }
    if (last && (const void*)out != (const void*)y) out[s] = (OutT)acc;
}

static int sy_log2(int F) {
    int l = 0;
    while ((1 << l) < F) ++l;
    return l;
}

#define SY_CHECK_FFT(name) \
    MG_CHECK_ARG(F >= MG_SYNTH_MIN_FFT && F <= MG_SYNTH_MAX_FFT && (F & (F - 1)) == 0, name ": F=%d must be a power of two in [%d, %d]", F, \
                 MG_SYNTH_MIN_FFT, MG_SYNTH_MAX_FFT)

extern "C" {

size_t mg_synth_lds_bytes(int F) { return F > 0 ? SY_LDS_BYTES(F) : 0; }

int mg_synth_noise(double* z, int64_t n, uint64_t seed, uint32_t site, const int64_t* used, void* stream) {
    MG_CHECK_ARG(n >= 0, "mg_synth_noise: n=%lld must not be negative", (long long)n);
    if (n == 0) return MG_OK;
    MG_CHECK_ARG(z && used && (((uintptr_t)z | (uintptr_t)used) & 7u) == 0, "mg_synth_noise: z and used must not be NULL and 8-byte aligned");
    const int64_t blocks = mg_ceil_div(n, SY_THREADS);
    hipLaunchKernelGGL(synth_noise_kernel, dim3((unsigned)(blocks < SY_NOISE_MAX_BLOCKS ? blocks : SY_NOISE_MAX_BLOCKS)), dim3(SY_THREADS), 0,
                       (hipStream_t)stream, z, n, (unsigned)seed, (unsigned)(seed >> 32), site, (const unsigned long long*)used);
    MG_CHECK_LAUNCH("mg_synth_noise");
    return MG_OK;
}

int mg_synth_pulses(const double* f0, int B, const int64_t* frame_start, const int64_t* n_frames, const int64_t* sample_offsets,
                    const int64_t* region_offsets, double S, double fs, double inc_scale, int F, int32_t* pulse_idx, double* pulse_delta,
                    int32_t* pulse_T, int32_t* pulse_voiced, int64_t* counts, void* stream) {
    SY_CHECK_FFT("mg_synth_pulses");
    MG_CHECK_ARG(B >= 0 && B <= MG_SYNTH_MAX_ITEMS, "mg_synth_pulses: B=%d outside [0, %d]", B, MG_SYNTH_MAX_ITEMS);
    MG_CHECK_ARG(S >= 1.0 && S <= 1048576.0, "mg_synth_pulses: S=%g samples per frame outside [1, 2^20]", S);
    MG_CHECK_ARG(fs > 0.0 && fs <= 1048576.0 && inc_scale > 0.0 && fs * inc_scale > 4294967295.0 && fs * inc_scale < 4294967297.0,
                 "mg_synth_pulses: fs=%g must lie in (0, 2^20] Hz and inc_scale=%g must be 2^32 / fs", fs, inc_scale);
    MG_CHECK_ARG(fs <= 500.0 * F, "mg_synth_pulses: fs=%g above 500 F = %g Hz: the 500 Hz unvoiced pulses would be more than F=%d samples apart", fs,
                 500.0 * F, F);
    if (B == 0) return MG_OK;                             // a grid of 0 is an error
    MG_CHECK_ARG(f0 && frame_start && n_frames && sample_offsets && region_offsets && pulse_idx && pulse_delta && pulse_T && pulse_voiced &&
                     counts,
                 "mg_synth_pulses: no pointer may be NULL");
    MG_CHECK_ARG((((uintptr_t)f0 | (uintptr_t)frame_start | (uintptr_t)n_frames | (uintptr_t)sample_offsets | (uintptr_t)region_offsets |
                   (uintptr_t)pulse_delta | (uintptr_t)counts) & 7u) == 0 &&
                     (((uintptr_t)pulse_idx | (uintptr_t)pulse_T | (uintptr_t)pulse_voiced) & 3u) == 0,
                 "mg_synth_pulses: f0, the offsets, pulse_delta and counts must be 8-byte, pulse_idx, pulse_T and pulse_voiced 4-byte aligned");
    hipLaunchKernelGGL(synth_pulses_kernel, dim3((unsigned)B), dim3(SY_THREADS), 0, (hipStream_t)stream, f0, frame_start, n_frames,
                       sample_offsets, region_offsets, S, fs / (double)F, 0.5 * fs, inc_scale, pulse_idx, pulse_delta, pulse_T, pulse_voiced,
                       counts);
    MG_CHECK_LAUNCH("mg_synth_pulses");
    return MG_OK;
}

int mg_synth_responses(const void* sp, int sp_f64, const void* ap, int ap_f64, int B, const int64_t* frame_start, const int64_t* n_frames,
                       const int64_t* sample_offsets, const int64_t* region_offsets, const int64_t* pulse_offsets, const int32_t* pulse_idx,
                       const double* pulse_delta, const int32_t* pulse_T, const int32_t* pulse_voiced, const double* z, const double* table,
                       double S, int F, int64_t g_lo, int64_t g_hi, double* workspace, void* stream) {
    SY_CHECK_FFT("mg_synth_responses");
    MG_CHECK_ARG(B >= 0 && B <= MG_SYNTH_MAX_ITEMS, "mg_synth_responses: B=%d outside [0, %d]", B, MG_SYNTH_MAX_ITEMS);
    MG_CHECK_ARG(S >= 1.0 && S <= 1048576.0, "mg_synth_responses: S=%g samples per frame outside [1, 2^20]", S);
    MG_CHECK_ARG(g_lo >= 0 && g_lo <= g_hi && g_hi - g_lo <= 0x7FFFFFFFll, "mg_synth_responses: bad pulse range [%lld, %lld)", (long long)g_lo,
                 (long long)g_hi);
    if (B == 0 || g_lo == g_hi) return MG_OK;
    MG_CHECK_ARG(sp && ap && frame_start && n_frames && sample_offsets && region_offsets && pulse_offsets && pulse_idx && pulse_delta &&
                     pulse_T && pulse_voiced && z && table && workspace,
                 "mg_synth_responses: no pointer may be NULL");
    MG_CHECK_ARG(((uintptr_t)sp & (sp_f64 ? 7u : 3u)) == 0 && ((uintptr_t)ap & (ap_f64 ? 7u : 3u)) == 0 &&
                     (((uintptr_t)frame_start | (uintptr_t)n_frames | (uintptr_t)sample_offsets | (uintptr_t)region_offsets |
                       (uintptr_t)pulse_offsets | (uintptr_t)pulse_delta | (uintptr_t)z | (uintptr_t)table | (uintptr_t)workspace) & 7u) == 0 &&
                     (((uintptr_t)pulse_idx | (uintptr_t)pulse_T | (uintptr_t)pulse_voiced) & 3u) == 0,
                 "mg_synth_responses: sp and ap must be aligned to their element, the float64 and int64 operands 8-byte, the int32 ones 4-byte");
    const size_t lds = SY_LDS_BYTES(F);
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)synth_responses_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            mg_set_error("mg_synth_responses: %zu bytes of LDS refused: %s", lds, hipGetErrorString(e));
            return MG_ELAUNCH;
        }
    }
    hipLaunchKernelGGL(synth_responses_kernel, dim3((unsigned)(g_hi - g_lo)), dim3(SY_THREADS), lds, (hipStream_t)stream, sp, sp_f64 ? 1 : 0, ap,
                       ap_f64 ? 1 : 0, B, frame_start, n_frames, sample_offsets, region_offsets, pulse_offsets, pulse_idx, pulse_delta, pulse_T,
                       pulse_voiced, z, table, S, F, sy_log2(F), g_lo, workspace);
    MG_CHECK_LAUNCH("mg_synth_responses");
    return MG_OK;
}

int mg_synth_overlap_add(const double* workspace, int B, const int64_t* sample_offsets, const int64_t* region_offsets,
                         const int64_t* pulse_offsets, const int32_t* pulse_idx, int F, int64_t g_lo, int64_t g_hi, int64_t total_samples,
                         double* y, int last, int out_f64, void* out, void* stream) {
    SY_CHECK_FFT("mg_synth_overlap_add");
    MG_CHECK_ARG(B >= 0 && B <= MG_SYNTH_MAX_ITEMS, "mg_synth_overlap_add: B=%d outside [0, %d]", B, MG_SYNTH_MAX_ITEMS);
    MG_CHECK_ARG(g_lo >= 0 && g_lo <= g_hi, "mg_synth_overlap_add: bad pulse range [%lld, %lld)", (long long)g_lo, (long long)g_hi);
    MG_CHECK_ARG(total_samples >= 0 && total_samples <= (int64_t)0x7FFFFFFFll * SY_THREADS, "mg_synth_overlap_add: total_samples=%lld out of range",
                 (long long)total_samples);
    if (B == 0 || total_samples == 0) return MG_OK;
    MG_CHECK_ARG(sample_offsets && region_offsets && pulse_offsets && pulse_idx && y && (g_lo == g_hi || workspace) && (!last || out),
                 "mg_synth_overlap_add: no pointer may be NULL (workspace only for an empty range, out only without last)");
    MG_CHECK_ARG((((uintptr_t)workspace | (uintptr_t)sample_offsets | (uintptr_t)region_offsets | (uintptr_t)pulse_offsets | (uintptr_t)y) & 7u) == 0 &&
                     ((uintptr_t)pulse_idx & 3u) == 0 && ((uintptr_t)out & (out_f64 ? 7u : 3u)) == 0,
                 "mg_synth_overlap_add: the float64 and int64 operands must be 8-byte, pulse_idx and a float out 4-byte aligned");
    const dim3 grid((unsigned)mg_ceil_div(total_samples, SY_THREADS));
#define SY_GO hipLaunchKernelGGL((synth_overlap_add_kernel<OutT>), grid, dim3(SY_THREADS), 0, (hipStream_t)stream, workspace, B, sample_offsets, \
                                 region_offsets, pulse_offsets, pulse_idx, F, g_lo, g_hi, total_samples, y, last ? 1 : 0, (OutT*)out)
    MG_SWITCH_F64(out_f64, OutT, SY_GO);
#undef SY_GO
    MG_CHECK_LAUNCH("mg_synth_overlap_add");
    return MG_OK;
}

}  // extern "C"
