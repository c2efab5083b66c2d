// K8 - maximum-likelihood parameter generation on the device (reference: morgana/viz/synthesis.py:79-178 `MLPG`, called from
// predict() of the shipped models - models/f0_test_model.py:86-89, models/RNN_SPSS.py:107-118 - i.e. once per training step,
// where the reference copies the predicted delta streams to the host, solves B x D banded systems with `bandmat` in float64 and
// copies the trajectories back to feed the LF0 / MCD metrics of loss()).
//
// Per (utterance b, feature dimension d) one symmetric positive-definite banded system of N = len_b + 2 padding unknowns:
//     P = sum_w W_w^T diag(tau_w) W_w,   rhs = sum_w W_w^T (mu_w tau_w),   x = P^-1 rhs           (synthesis.py:39-77, :164-168)
// with W_w the N x N Toeplitz matrix of window w cut off at the edges (W[s, t] = c_w[l_w + t - s]), mu / tau the padded
// (first / last frame repeated `padding` times, :113-120) means and precisions of stream column w D + d.  As in the reference
// mu / var and 1 / var are formed in float32 (numpy arithmetic on the float32 arrays the model produced, :161-165) and
// everything after that is float64 (:64-65).
//
// Two kernels:
//   mlpg_band_kernel   one thread per (frame, system): the band row P[t, t-m], m = 0..HB, and rhs[t], straight into the
//                      workspace planes [plane][frame][system] (fully parallel, coalesced over systems; HBM bound).
//   mlpg_solve_kernel  one thread per system: banded LDL^T row by row (the rows of a system form a dependent chain of
//                      HB + 1 fused multiply-adds and one reciprocal each), forward substitution in the same sweep, L and
//                      z = D^-1 L^-1 rhs written over the band planes; then the backward sweep and the float32 store of
//                      frames [padding, N - padding).  The chain is latency bound (one fp64 reciprocal + ~12 FMA per row, 2 N
//                      steps per system): rows are fetched 8 at a time, a block ahead of the arithmetic, and the reciprocal is
//                      v_rcp_f64 + two Newton steps instead of the IEEE division sequence.
// The variances are global (W D,), per frame (B, T, W D) or per item (B, W D) - MG_MLPG_VAR_ITEM: speaker-dependent delta variances,
// one row per utterance; only the address the band kernel reads them from differs, the systems and the solve are the same.
// Summation order differs from bandmat's (which adds the windows band by band), so results agree to float64 rounding, not bit
// for bit: tests hold the float32 trajectories to 1e-6 relative against the float64 CPU restatement.
//
// The gradient with respect to the means (mg_mlpg_grad_f32; trajectory / minimum-generation-error training).  x is linear in mu:
// x = P^-1 sum_w W_w^T (tau_w o mu_w), so for an upstream gradient g on the output rows [padding, N - padding)
//     P lambda = g~ (g on the output rows, zero on the padding rows),    v_w = tau_w o (W_w lambda),
//     dL/dmu[b, f, w D + d] = sum over the padded rows s that read frame f of v_w[s]
// (one row for an inner frame, padding + 1 rows for the first and the last frame, all N rows when len = 1).  P is symmetric: the band,
// the factorisation and both sweeps are the forward's, instantiated with GRAD / KEEP:
//   mlpg_band_kernel<HB, true>          the same band rows; the right-hand-side plane holds g~ (frames >= len are never read)
//   mlpg_solve_kernel<HB, double, true> the same sweeps; x_i = lambda_i goes over z_i in plane HB + 1 for ALL N rows (by then z_i is
//                                       in registers, and the prefetch reads lower rows only) instead of to the output
//   mlpg_scatter_kernel                 one thread per (inner frame, system): tau (W_w lambda) at the frame's one padded row, float64,
//                                       one rounding at the store.  No atomics: a frame has one owner.
//   mlpg_scatter_edge_kernel            one thread per (first / last frame, system): the same over its padding + 1 rows in increasing s
// The variances get no gradient there (normaliser constants at those call sites).
//
// Both gradients (mg_mlpg_grad_mv_f32; per-frame variances a model predicts - a 'gaussian' stream under a trajectory or global-variance
// loss).  x~ = P^-1 rhs on ALL n rows is needed next to lambda:
//     dL/dvar[b, f, w D + d] = sum over the padded rows s that read frame f of -tau_w[s]^2 (W_w lambda)[s] (mu_w[s] - (W_w x~)[s])
// so the forward's system and the adjoint one are built and solved SIDE BY SIDE, grid.y = 2 picking a set of planes:
//   mlpg_band_pair_kernel<HB>     y = 0: the forward's band rows and rhs; y = 1: the GRAD rows (the same band, g~)
//   mlpg_solve_pair_kernel<HB>    the KEEP solve of either set: two independent chains on waves of their own, so the chain latency
//                                 of one solve, not of two; x~ and lambda stay in plane HB + 1 of their sets
//   mlpg_fold_mv_kernel / mlpg_fold_mv_edge_kernel   the scatter kernels with a second tap pass / register window over x~; grad_means
//                                 bit for bit what mg_mlpg_grad_f32 writes
#include "common.h"

#define MLPG_MAX_WINDOWS 4
#define MLPG_MAX_COEFF 5

struct MlpgWindows {
    int n;
    int l[MLPG_MAX_WINDOWS], u[MLPG_MAX_WINDOWS];
    double c[MLPG_MAX_WINDOWS][MLPG_MAX_COEFF];
};

// GRAD: `means` is the upstream gradient [B, T, D] and the right-hand side is g~ (see the header comment); the band is the same
template <int HB, bool GRAD = false>
__global__ __launch_bounds__(256) void mlpg_band_kernel(const float* __restrict__ means, const float* __restrict__ variances,
                                                        int var_per_frame, const int64_t* __restrict__ seq_len, int B, int T, int D,
                                                        MlpgWindows win, int padding, double* __restrict__ planes) {
#include "mlpg_band_body.inc"
}

// The two systems of mg_mlpg_grad_mv_f32 side by side, blockIdx.y picks one: 0 = the forward's (right-hand side mu tau, per-frame
// variances) into the first set of planes, 1 = the adjoint's (right-hand side g~) into the second, `set_stride` doubles further on
template <int HB>
__global__ __launch_bounds__(256) void mlpg_band_pair_kernel(const float* __restrict__ fwd_means, const float* __restrict__ grad_out,
                                                             const float* __restrict__ variances, const int64_t* __restrict__ seq_len,
                                                             int B, int T, int D, MlpgWindows win, int padding,
                                                             double* __restrict__ both, size_t set_stride) {
    constexpr int var_per_frame = 1;
    if (blockIdx.y == 0) {
        constexpr bool GRAD = false;
        const float* __restrict__ means = fwd_means;
        double* __restrict__ planes = both;
#include "mlpg_band_body.inc"
    } else {
        constexpr bool GRAD = true;
        const float* __restrict__ means = grad_out;
        double* __restrict__ planes = both + set_stride;
#include "mlpg_band_body.inc"
    }
}

#define MLPG_ROWS 8      // rows fetched ahead per block: their loads fly while the previous block's chain is worked off

// 1 / d for d > 0 (pivots of an SPD band): v_rcp_f64 + two Newton steps, ~1 ulp - a third of the IEEE division sequence, and
// it sits on the row-to-row dependency chain
__device__ __forceinline__ double mlpg_rcp(double d) {
    double y = __builtin_amdgcn_rcp(d);
    double e = __builtin_fma(-d, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-d, y, 1.0);
    return __builtin_fma(y, e, y);
}

// KEEP: the solution of all n rows stays in the workspace, float64, over z in plane HB + 1; `out` is not used
template <int HB, typename OutT, bool KEEP = false>
__global__ __launch_bounds__(64) void mlpg_solve_kernel(const int64_t* __restrict__ seq_len, int B, int T, int D, int padding,
                                                       double* __restrict__ planes, OutT* __restrict__ out) {
#include "mlpg_solve_body.inc"
}

// Both sets of planes of mlpg_band_pair_kernel in one launch, blockIdx.y picks one: two independent chains on waves of their own,
// each the KEEP solve (x~ resp. lambda of all n rows over z in its plane HB + 1)
template <int HB>
__global__ __launch_bounds__(64) void mlpg_solve_pair_kernel(const int64_t* __restrict__ seq_len, int B, int T, int D, int padding,
                                                            double* __restrict__ both, size_t set_stride) {
    using OutT = double;
    constexpr bool KEEP = true;
    double* __restrict__ planes = both + blockIdx.y * set_stride;
    OutT* __restrict__ out = nullptr;
#include "mlpg_solve_body.inc"
}

#define MLPG_SPAN (MLPG_MAX_COEFF - 1)      // a window reaches at most this many rows to either side of its own

// grad_means[b, f, w D + d] of the INNER frames 0 < f < len - 1, one (frame, system) per thread, gid / S = f as in the band kernel: one
// padded row each, its taps read directly; lambda loads coalesce over the systems and the W stores of neighbouring threads are
// contiguous over d.  Rows past len stay as the memset left them; the first and the last frame are the edge kernel's.
template <typename OutT>
__global__ __launch_bounds__(256) void mlpg_scatter_kernel(const float* __restrict__ variances, int var_per_frame,
                                                           const int64_t* __restrict__ seq_len, int B, int T, int D, MlpgWindows win,
                                                           int padding, const double* __restrict__ lambda, OutT* __restrict__ grad_means) {
    const int S = B * D;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)T * S) return;
    const int f = (int)(gid / S), sys = (int)(gid - (int64_t)f * S);
    const int b = sys / D, d = sys - b * D;
    const int len = (int)(seq_len ? (seq_len[b] < T ? seq_len[b] : (int64_t)T) : (int64_t)T);
    if (f <= 0 || f >= len - 1) return;
    const int n = len + 2 * padding, width = win.n * D, s = f + padding;
    const double* lam = lambda + sys;
    for (int w = 0; w < win.n; ++w) {
        const int l = win.l[w], u = win.u[w];
        const size_t at = ((size_t)b * T + f) * width + (size_t)w * D + d;
        const float var = var_per_frame == MG_MLPG_VAR_ITEM ? variances[(size_t)b * width + w * D + d]
                          : var_per_frame ? variances[at] : variances[w * D + d];
        double dot = 0.0;
        for (int k = -l; k <= u; ++k)
            if (s + k >= 0 && s + k < n) dot += win.c[w][l + k] * lam[(size_t)(s + k) * S];
        grad_means[at] = (OutT)((double)(1.0f / var) * dot);
    }
}

// The first (e = 0) and the last (e = 1) frame of every system, one (e, system) per thread: padding + 1 padded rows each, or all n rows
// for the one frame of an utterance of length 1.  A chain of dependent additions but NOT of dependent loads: lambda slides through a
// register window of 2 SPAN + 1 rows, one new row per step, fetched MLPG_ROWS at a time with unconditional (clamped) loads that fly
// together - a load per tap and row, waited for one by one, cost 0.1 ms for 101 rows.  Taps outside a window's [-l, u] carry a zero
// coefficient and rows outside [0, n) a zero lambda, so every sum keeps its order: rows in increasing s, taps in increasing k.
template <typename OutT>
__global__ __launch_bounds__(64) void mlpg_scatter_edge_kernel(const float* __restrict__ variances, int var_per_frame,
                                                              const int64_t* __restrict__ seq_len, int B, int T, int D, MlpgWindows win,
                                                              int padding, const double* __restrict__ lambda,
                                                              OutT* __restrict__ grad_means) {
    const int S = B * D;
    const int gid = blockIdx.x * 64 + threadIdx.x;
    if (gid >= 2 * S) return;
    const int e = gid / S, sys = gid - e * S;
    const int b = sys / D, d = sys - b * D;
    const int len = (int)(seq_len ? (seq_len[b] < T ? seq_len[b] : (int64_t)T) : (int64_t)T);
    if (len <= 0 || (e && len == 1)) return;
    const int f = e ? len - 1 : 0;
    const int n = len + 2 * padding, width = win.n * D;
    const int s_lo = f == 0 ? 0 : f + padding, s_hi = f == len - 1 ? n - 1 : f + padding;      // the padded rows that read frame f
    const double* lam = lambda + sys;
    const size_t at0 = ((size_t)b * T + f) * width + d;
    double coeff[MLPG_MAX_WINDOWS][2 * MLPG_SPAN + 1], tau[MLPG_MAX_WINDOWS], acc[MLPG_MAX_WINDOWS];
#pragma unroll
    for (int w = 0; w < MLPG_MAX_WINDOWS; ++w) {
        tau[w] = 0.0; acc[w] = 0.0;
        const int l = w < win.n ? win.l[w] : 0, u = w < win.n ? win.u[w] : -1;
#pragma unroll
        for (int k = -MLPG_SPAN; k <= MLPG_SPAN; ++k) {
            const double c = win.c[w < win.n ? w : 0][min(max(l + k, 0), MLPG_MAX_COEFF - 1)];
            coeff[w][k + MLPG_SPAN] = (k >= -l && k <= u) ? c : 0.0;
        }
        if (w < win.n) {
            const size_t at = at0 + (size_t)w * D;
            const float var = var_per_frame == MG_MLPG_VAR_ITEM ? variances[(size_t)b * width + w * D + d]
                              : var_per_frame ? variances[at] : variances[w * D + d];
            tau[w] = (double)(1.0f / var);
        }
    }
    auto fetch = [&](int r) __attribute__((always_inline)) {       // lambda[r], zero outside [0, n); the address is clamped into it
        const double v = lam[(size_t)min(max(r, 0), n - 1) * S];
        return r >= 0 && r < n ? v : 0.0;
    };
    double rows[2 * MLPG_SPAN + 1];              // before row s: rows[j + 1] = lambda[s - SPAN + j], j = 0 .. 2 SPAN - 1
    rows[0] = 0.0;
#pragma unroll
    for (int j = 0; j < 2 * MLPG_SPAN; ++j) rows[j + 1] = fetch(s_lo - MLPG_SPAN + j);
    for (int s0 = s_lo; s0 <= s_hi; s0 += MLPG_ROWS) {
        double nxt[MLPG_ROWS];
#pragma unroll
        for (int j = 0; j < MLPG_ROWS; ++j) nxt[j] = fetch(s0 + j + MLPG_SPAN);
#pragma unroll
        for (int j = 0; j < MLPG_ROWS; ++j) {
            if (s0 + j > s_hi) break;
#pragma unroll
            for (int i = 0; i < 2 * MLPG_SPAN; ++i) rows[i] = rows[i + 1];
            rows[2 * MLPG_SPAN] = nxt[j];
#pragma unroll
            for (int w = 0; w < MLPG_MAX_WINDOWS; ++w) {
                double dot = 0.0;
#pragma unroll
                for (int i = 0; i <= 2 * MLPG_SPAN; ++i) dot += coeff[w][i] * rows[i];
                acc[w] += tau[w] * dot;
            }
        }
    }
#pragma unroll
    for (int w = 0; w < MLPG_MAX_WINDOWS; ++w)
        if (w < win.n) grad_means[at0 + (size_t)w * D] = (OutT)acc[w];
}

// mg_mlpg_grad_mv_f32: both gradients of the INNER frames 0 < f < len - 1, one (frame, system) per thread as mlpg_scatter_kernel.  With
// lambda and x~ (the forward's solution on ALL n rows) side by side: dL/dmu = tau (W_w lambda)[s] - the same expression, in the same
// order, as mlpg_scatter_kernel, so the same bits - and dL/dvar = -tau^2 (W_w lambda)[s] (mu - (W_w x~)[s]), one rounding each.
template <typename OutT>
__global__ __launch_bounds__(256) void mlpg_fold_mv_kernel(const float* __restrict__ means, const float* __restrict__ variances,
                                                           const int64_t* __restrict__ seq_len, int B, int T, int D, MlpgWindows win,
                                                           int padding, const double* __restrict__ lambda, const double* __restrict__ xs,
                                                           OutT* __restrict__ grad_means, OutT* __restrict__ grad_variances) {
    const int S = B * D;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)T * S) return;
    const int f = (int)(gid / S), sys = (int)(gid - (int64_t)f * S);
    const int b = sys / D, d = sys - b * D;
    const int len = (int)(seq_len ? (seq_len[b] < T ? seq_len[b] : (int64_t)T) : (int64_t)T);
    if (f <= 0 || f >= len - 1) return;
    const int n = len + 2 * padding, width = win.n * D, s = f + padding;
    const double* lam = lambda + sys;
    const double* xt = xs + sys;
    for (int w = 0; w < win.n; ++w) {
        const int l = win.l[w], u = win.u[w];
        const size_t at = ((size_t)b * T + f) * width + (size_t)w * D + d;
        const float var = variances[at];
        const double tau = (double)(1.0f / var), mu = (double)means[at];
        double dot = 0.0, wx = 0.0;
        for (int k = -l; k <= u; ++k)
            if (s + k >= 0 && s + k < n) {
                dot += win.c[w][l + k] * lam[(size_t)(s + k) * S];
                wx += win.c[w][l + k] * xt[(size_t)(s + k) * S];
            }
        grad_means[at] = (OutT)(tau * dot);
        grad_variances[at] = (OutT)(-(tau * tau) * dot * (mu - wx));
    }
}

// The first and the last frame, as mlpg_scatter_edge_kernel with a second register window for x~: per padded row s and window w
// dot = (W_w lambda)[s], wx = (W_w x~)[s]; acc += tau dot (the means, bit for bit the edge kernel's) and accv += -tau^2 dot (mu - wx)
// (mu and tau are the frame's, the same on every one of its rows).  Rows in increasing s, taps in increasing k.
template <typename OutT>
__global__ __launch_bounds__(64) void mlpg_fold_mv_edge_kernel(const float* __restrict__ means, const float* __restrict__ variances,
                                                              const int64_t* __restrict__ seq_len, int B, int T, int D, MlpgWindows win,
                                                              int padding, const double* __restrict__ lambda,
                                                              const double* __restrict__ xs, OutT* __restrict__ grad_means,
                                                              OutT* __restrict__ grad_variances) {
    const int S = B * D;
    const int gid = blockIdx.x * 64 + threadIdx.x;
    if (gid >= 2 * S) return;
    const int e = gid / S, sys = gid - e * S;
    const int b = sys / D, d = sys - b * D;
    const int len = (int)(seq_len ? (seq_len[b] < T ? seq_len[b] : (int64_t)T) : (int64_t)T);
    if (len <= 0 || (e && len == 1)) return;
    const int f = e ? len - 1 : 0;
    const int n = len + 2 * padding, width = win.n * D;
    const int s_lo = f == 0 ? 0 : f + padding, s_hi = f == len - 1 ? n - 1 : f + padding;      // the padded rows that read frame f
    const double* lam = lambda + sys;
    const double* xt = xs + sys;
    const size_t at0 = ((size_t)b * T + f) * width + d;
    double coeff[MLPG_MAX_WINDOWS][2 * MLPG_SPAN + 1], tau[MLPG_MAX_WINDOWS], ntau2[MLPG_MAX_WINDOWS], mu[MLPG_MAX_WINDOWS];
    double acc[MLPG_MAX_WINDOWS], accv[MLPG_MAX_WINDOWS];
#pragma unroll
    for (int w = 0; w < MLPG_MAX_WINDOWS; ++w) {
        tau[w] = 0.0; ntau2[w] = 0.0; mu[w] = 0.0; acc[w] = 0.0; accv[w] = 0.0;
        const int l = w < win.n ? win.l[w] : 0, u = w < win.n ? win.u[w] : -1;
#pragma unroll
        for (int k = -MLPG_SPAN; k <= MLPG_SPAN; ++k) {
            const double c = win.c[w < win.n ? w : 0][min(max(l + k, 0), MLPG_MAX_COEFF - 1)];
            coeff[w][k + MLPG_SPAN] = (k >= -l && k <= u) ? c : 0.0;
        }
        if (w < win.n) {
            const size_t at = at0 + (size_t)w * D;
            tau[w] = (double)(1.0f / variances[at]);
            ntau2[w] = -(tau[w] * tau[w]);
            mu[w] = (double)means[at];
        }
    }
    auto fetch = [&](const double* __restrict__ from, int r) __attribute__((always_inline)) {      // zero outside [0, n); address clamped
        const double v = from[(size_t)min(max(r, 0), n - 1) * S];
        return r >= 0 && r < n ? v : 0.0;
    };
    double rows[2 * MLPG_SPAN + 1], xrows[2 * MLPG_SPAN + 1];      // before row s: rows[j + 1] = lambda[s - SPAN + j], xrows likewise of x~
    rows[0] = 0.0; xrows[0] = 0.0;
#pragma unroll
    for (int j = 0; j < 2 * MLPG_SPAN; ++j) {
        rows[j + 1] = fetch(lam, s_lo - MLPG_SPAN + j);
        xrows[j + 1] = fetch(xt, s_lo - MLPG_SPAN + j);
    }
    for (int s0 = s_lo; s0 <= s_hi; s0 += MLPG_ROWS) {
        double nxt[MLPG_ROWS], xnxt[MLPG_ROWS];
#pragma unroll
        for (int j = 0; j < MLPG_ROWS; ++j) {
            nxt[j] = fetch(lam, s0 + j + MLPG_SPAN);
            xnxt[j] = fetch(xt, s0 + j + MLPG_SPAN);
        }
#pragma unroll
        for (int j = 0; j < MLPG_ROWS; ++j) {
            if (s0 + j > s_hi) break;
#pragma unroll
            for (int i = 0; i < 2 * MLPG_SPAN; ++i) {
                rows[i] = rows[i + 1];
                xrows[i] = xrows[i + 1];
            }
            rows[2 * MLPG_SPAN] = nxt[j];
            xrows[2 * MLPG_SPAN] = xnxt[j];
#pragma unroll
            for (int w = 0; w < MLPG_MAX_WINDOWS; ++w) {
                double dot = 0.0, wx = 0.0;
#pragma unroll
                for (int i = 0; i <= 2 * MLPG_SPAN; ++i) dot += coeff[w][i] * rows[i];
#pragma unroll
                for (int i = 0; i <= 2 * MLPG_SPAN; ++i) wx += coeff[w][i] * xrows[i];
                acc[w] += tau[w] * dot;
                accv[w] += ntau2[w] * dot * (mu[w] - wx);
            }
        }
    }
#pragma unroll
    for (int w = 0; w < MLPG_MAX_WINDOWS; ++w)
        if (w < win.n) {
            grad_means[at0 + (size_t)w * D] = (OutT)acc[w];
            grad_variances[at0 + (size_t)w * D] = (OutT)accv[w];
        }
}

static int mlpg_half_bandwidth(int n_windows, const int* win_l, const int* win_u) {
    int hb = 0;
    for (int w = 0; w < n_windows; ++w) hb = win_l[w] + win_u[w] > hb ? win_l[w] + win_u[w] : hb;
    return hb <= 2 ? 2 : 4;
}

extern "C" {

// planes: (HB + 2) x (T + 2 padding) x (B D) doubles
size_t mg_mlpg_workspace_bytes(int B, int T, int D, int padding, int n_windows, const int* win_l, const int* win_u) {
    if (B <= 0 || T <= 0 || D <= 0 || padding < 0 || n_windows <= 0 || !win_l || !win_u) return 0;
    const int hb = mlpg_half_bandwidth(n_windows, win_l, win_u);
    return (size_t)(hb + 2) * (size_t)(T + 2 * padding) * (size_t)B * D * sizeof(double);
}

int mg_mlpg_f32(const float* means, const float* variances, int var_per_frame, const int64_t* seq_len, int B, int T, int D,
                int n_windows, const int* win_l, const int* win_u, const double* win_coeff, int padding, void* out, int out_f64,
                void* workspace, size_t workspace_bytes, void* stream) {
    MG_CHECK_ARG(means && variances && out && win_l && win_u && win_coeff, "mg_mlpg_f32: null argument");
    MG_CHECK_ARG(B > 0 && T > 0 && D > 0 && padding >= 0, "mg_mlpg_f32: bad shape (B=%d T=%d D=%d padding=%d)", B, T, D, padding);
    MG_CHECK_ARG(n_windows > 0 && n_windows <= MLPG_MAX_WINDOWS, "mg_mlpg_f32: 1..%d windows supported, got %d", MLPG_MAX_WINDOWS,
                 n_windows);
    MlpgWindows win = {};
    win.n = n_windows;
    for (int w = 0; w < n_windows; ++w) {
        MG_CHECK_ARG(win_l[w] >= 0 && win_u[w] >= 0 && win_l[w] + win_u[w] + 1 <= MLPG_MAX_COEFF,
                     "mg_mlpg_f32: window %d (l=%d, u=%d) is wider than %d coefficients", w, win_l[w], win_u[w], MLPG_MAX_COEFF);
        win.l[w] = win_l[w];
        win.u[w] = win_u[w];
        for (int k = 0; k <= win_l[w] + win_u[w]; ++k) win.c[w][k] = win_coeff[w * MLPG_MAX_COEFF + k];
    }
    const size_t need = mg_mlpg_workspace_bytes(B, T, D, padding, n_windows, win_l, win_u);
    MG_CHECK_ARG((size_t)(T + 2 * padding) * (size_t)B * D < ((size_t)1 << 31), "mg_mlpg_f32: too many unknowns for 32-bit frame x system ids");
    if (!workspace || workspace_bytes < need) {
        mg_set_error("mg_mlpg_f32: workspace of %zu bytes needed, got %zu", need, workspace_bytes);
        return MG_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t out_bytes = (size_t)B * T * D * (out_f64 ? sizeof(double) : sizeof(float));
    if (hipMemsetAsync(out, 0, out_bytes, st) != hipSuccess) {           // frames past seq_len stay zero (synthesis.py:152, :170)
        mg_set_error("mg_mlpg_f32: memset failed");
        return MG_ELAUNCH;
    }
    const int hb = mlpg_half_bandwidth(n_windows, win_l, win_u);
    const int64_t cells = (int64_t)(T + 2 * padding) * B * D;
    const unsigned grid_a = (unsigned)mg_ceil_div(cells, 256), grid_b = (unsigned)mg_ceil_div((int64_t)B * D, 64);
    double* planes = (double*)workspace;
#define MLPG_RUN(HB)                                                                                                                  \
    do {                                                                                                                              \
        hipLaunchKernelGGL((mlpg_band_kernel<HB>), dim3(grid_a), dim3(256), 0, st, means, variances, var_per_frame, seq_len, B, T, D,  \
                           win, padding, planes);                                                                                     \
        if (out_f64)                                                                                                                  \
            hipLaunchKernelGGL((mlpg_solve_kernel<HB, double>), dim3(grid_b), dim3(64), 0, st, seq_len, B, T, D, padding, planes,      \
                               (double*)out);                                                                                         \
        else                                                                                                                          \
            hipLaunchKernelGGL((mlpg_solve_kernel<HB, float>), dim3(grid_b), dim3(64), 0, st, seq_len, B, T, D, padding, planes,       \
                               (float*)out);                                                                                          \
    } while (0)
    if (hb == 2)
        MLPG_RUN(2);
    else
        MLPG_RUN(4);
    MG_CHECK_LAUNCH("mg_mlpg_f32");
    return MG_OK;
}

int mg_mlpg_grad_f32(const float* grad_out, const float* variances, int var_per_frame, const int64_t* seq_len, int B, int T, int D,
                     int n_windows, const int* win_l, const int* win_u, const double* win_coeff, int padding, void* grad_means,
                     int out_f64, void* workspace, size_t workspace_bytes, void* stream) {
    MG_CHECK_ARG(grad_out && variances && grad_means && win_l && win_u && win_coeff, "mg_mlpg_grad_f32: null argument");
    MG_CHECK_ARG(B > 0 && T > 0 && D > 0 && padding >= 0, "mg_mlpg_grad_f32: bad shape (B=%d T=%d D=%d padding=%d)", B, T, D, padding);
    MG_CHECK_ARG(n_windows > 0 && n_windows <= MLPG_MAX_WINDOWS, "mg_mlpg_grad_f32: 1..%d windows supported, got %d", MLPG_MAX_WINDOWS,
                 n_windows);
    MlpgWindows win = {};
    win.n = n_windows;
    for (int w = 0; w < n_windows; ++w) {
        MG_CHECK_ARG(win_l[w] >= 0 && win_u[w] >= 0 && win_l[w] + win_u[w] + 1 <= MLPG_MAX_COEFF,
                     "mg_mlpg_grad_f32: window %d (l=%d, u=%d) is wider than %d coefficients", w, win_l[w], win_u[w], MLPG_MAX_COEFF);
        win.l[w] = win_l[w];
        win.u[w] = win_u[w];
        for (int k = 0; k <= win_l[w] + win_u[w]; ++k) win.c[w][k] = win_coeff[w * MLPG_MAX_COEFF + k];
    }
    const size_t need = mg_mlpg_workspace_bytes(B, T, D, padding, n_windows, win_l, win_u);
    MG_CHECK_ARG((size_t)(T + 2 * padding) * (size_t)B * D < ((size_t)1 << 31), "mg_mlpg_grad_f32: too many unknowns for 32-bit frame x system ids");
    if (!workspace || workspace_bytes < need) {
        mg_set_error("mg_mlpg_grad_f32: workspace of %zu bytes needed, got %zu", need, workspace_bytes);
        return MG_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t out_bytes = (size_t)B * T * n_windows * D * (out_f64 ? sizeof(double) : sizeof(float));
    if (hipMemsetAsync(grad_means, 0, out_bytes, st) != hipSuccess) {    // frames past seq_len get no gradient
        mg_set_error("mg_mlpg_grad_f32: memset failed");
        return MG_ELAUNCH;
    }
    const int hb = mlpg_half_bandwidth(n_windows, win_l, win_u);
    const int n_max = T + 2 * padding;
    const unsigned grid_a = (unsigned)mg_ceil_div((int64_t)n_max * B * D, 256), grid_b = (unsigned)mg_ceil_div((int64_t)B * D, 64);
    const unsigned grid_c = (unsigned)mg_ceil_div((int64_t)T * B * D, 256), grid_d = (unsigned)mg_ceil_div((int64_t)2 * B * D, 64);
    double* planes = (double*)workspace;
    const double* lambda = planes + (size_t)(hb + 1) * n_max * B * D;
#define MLPG_GRAD_RUN(HB)                                                                                                             \
    do {                                                                                                                              \
        hipLaunchKernelGGL((mlpg_band_kernel<HB, true>), dim3(grid_a), dim3(256), 0, st, grad_out, variances, var_per_frame, seq_len,  \
                           B, T, D, win, padding, planes);                                                                            \
        hipLaunchKernelGGL((mlpg_solve_kernel<HB, double, true>), dim3(grid_b), dim3(64), 0, st, seq_len, B, T, D, padding, planes,    \
                           (double*)nullptr);                                                                                         \
    } while (0)
    if (hb == 2)
        MLPG_GRAD_RUN(2);
    else
        MLPG_GRAD_RUN(4);
#define MLPG_SCATTER(OutT)                                                                                                            \
    do {                                                                                                                              \
        hipLaunchKernelGGL((mlpg_scatter_kernel<OutT>), dim3(grid_c), dim3(256), 0, st, variances, var_per_frame, seq_len, B, T, D,    \
                           win, padding, lambda, (OutT*)grad_means);                                                                  \
        hipLaunchKernelGGL((mlpg_scatter_edge_kernel<OutT>), dim3(grid_d), dim3(64), 0, st, variances, var_per_frame, seq_len, B, T,   \
                           D, win, padding, lambda, (OutT*)grad_means);                                                               \
    } while (0)
    if (out_f64)
        MLPG_SCATTER(double);
    else
        MLPG_SCATTER(float);
    MG_CHECK_LAUNCH("mg_mlpg_grad_f32");
    return MG_OK;
}

// two sets of the forward's planes: the forward system (x~ of all rows in its plane HB + 1) and the adjoint one (lambda)
size_t mg_mlpg_grad_mv_workspace_bytes(int B, int T, int D, int padding, int n_windows, const int* win_l, const int* win_u) {
    return 2 * mg_mlpg_workspace_bytes(B, T, D, padding, n_windows, win_l, win_u);
}

int mg_mlpg_grad_mv_f32(const float* grad_out, const float* means, const float* variances, const int64_t* seq_len, int B, int T, int D,
                        int n_windows, const int* win_l, const int* win_u, const double* win_coeff, int padding, void* grad_means,
                        void* grad_variances, int out_f64, void* workspace, size_t workspace_bytes, void* stream) {
    MG_CHECK_ARG(grad_out && means && variances && grad_means && grad_variances && win_l && win_u && win_coeff,
                 "mg_mlpg_grad_mv_f32: null argument");
    MG_CHECK_ARG(B > 0 && T > 0 && D > 0 && padding >= 0, "mg_mlpg_grad_mv_f32: bad shape (B=%d T=%d D=%d padding=%d)", B, T, D, padding);
    MG_CHECK_ARG(n_windows > 0 && n_windows <= MLPG_MAX_WINDOWS, "mg_mlpg_grad_mv_f32: 1..%d windows supported, got %d", MLPG_MAX_WINDOWS,
                 n_windows);
    MlpgWindows win = {};
    win.n = n_windows;
    for (int w = 0; w < n_windows; ++w) {
        MG_CHECK_ARG(win_l[w] >= 0 && win_u[w] >= 0 && win_l[w] + win_u[w] + 1 <= MLPG_MAX_COEFF,
                     "mg_mlpg_grad_mv_f32: window %d (l=%d, u=%d) is wider than %d coefficients", w, win_l[w], win_u[w], MLPG_MAX_COEFF);
        win.l[w] = win_l[w];
        win.u[w] = win_u[w];
        for (int k = 0; k <= win_l[w] + win_u[w]; ++k) win.c[w][k] = win_coeff[w * MLPG_MAX_COEFF + k];
    }
    const size_t need = mg_mlpg_grad_mv_workspace_bytes(B, T, D, padding, n_windows, win_l, win_u);
    MG_CHECK_ARG((size_t)(T + 2 * padding) * (size_t)B * D < ((size_t)1 << 31), "mg_mlpg_grad_mv_f32: too many unknowns for 32-bit frame x system ids");
    if (!workspace || workspace_bytes < need) {
        mg_set_error("mg_mlpg_grad_mv_f32: workspace of %zu bytes needed, got %zu", need, workspace_bytes);
        return MG_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t out_bytes = (size_t)B * T * n_windows * D * (out_f64 ? sizeof(double) : sizeof(float));
    if (hipMemsetAsync(grad_means, 0, out_bytes, st) != hipSuccess || hipMemsetAsync(grad_variances, 0, out_bytes, st) != hipSuccess) {
        mg_set_error("mg_mlpg_grad_mv_f32: memset failed");                  // frames past seq_len get no gradient
        return MG_ELAUNCH;
    }
    const int hb = mlpg_half_bandwidth(n_windows, win_l, win_u);
    const int n_max = T + 2 * padding;
    const unsigned grid_a = (unsigned)mg_ceil_div((int64_t)n_max * B * D, 256), grid_b = (unsigned)mg_ceil_div((int64_t)B * D, 64);
    const unsigned grid_c = (unsigned)mg_ceil_div((int64_t)T * B * D, 256), grid_d = (unsigned)mg_ceil_div((int64_t)2 * B * D, 64);
    double* planes = (double*)workspace;
    const size_t set_stride = (size_t)(hb + 2) * n_max * B * D;             // doubles per set: mg_mlpg_workspace_bytes / 8
    const double* xs = planes + (size_t)(hb + 1) * n_max * B * D;
    const double* lambda = xs + set_stride;
#define MLPG_PAIR_RUN(HB)                                                                                                             \
    do {                                                                                                                              \
        hipLaunchKernelGGL((mlpg_band_pair_kernel<HB>), dim3(grid_a, 2), dim3(256), 0, st, means, grad_out, variances, seq_len, B, T,  \
                           D, win, padding, planes, set_stride);                                                                      \
        hipLaunchKernelGGL((mlpg_solve_pair_kernel<HB>), dim3(grid_b, 2), dim3(64), 0, st, seq_len, B, T, D, padding, planes,          \
                           set_stride);                                                                                               \
    } while (0)
    if (hb == 2)
        MLPG_PAIR_RUN(2);
    else
        MLPG_PAIR_RUN(4);
#define MLPG_FOLD_MV(OutT)                                                                                                            \
    do {                                                                                                                              \
        hipLaunchKernelGGL((mlpg_fold_mv_kernel<OutT>), dim3(grid_c), dim3(256), 0, st, means, variances, seq_len, B, T, D, win,       \
                           padding, lambda, xs, (OutT*)grad_means, (OutT*)grad_variances);                                            \
        hipLaunchKernelGGL((mlpg_fold_mv_edge_kernel<OutT>), dim3(grid_d), dim3(64), 0, st, means, variances, seq_len, B, T, D, win,   \
                           padding, lambda, xs, (OutT*)grad_means, (OutT*)grad_variances);                                            \
    } while (0)
    if (out_f64)
        MLPG_FOLD_MV(double);
    else
        MLPG_FOLD_MV(float);
    MG_CHECK_LAUNCH("mg_mlpg_grad_mv_f32");
    return MG_OK;
}

}  // extern "C"
