// K8b - parameter generation under a global-variance prior (Toda & Tokuda 2007: "A speech parameter generation algorithm considering
// global variance for HMM-based speech synthesis"; the generation step HTS and Merlin ship, which the reference does not have: its
// every generation path - morgana/viz/synthesis.py:79-178 - writes the plain, over-smoothed MLPG solution).
//
// Per (utterance b, static dimension d): P, rhs, N = len + 2 padding rows and the output rows O = [padding, N - padding) are exactly
// mg_mlpg_f32's (csrc/mlpg.hip; the band kernel's body is the same text).  With n = len, W windows, omega = 1 / (W n), v(x) the biased
// variance of x over O and (mu_v, sigma_v^2) the GV mean and variance of dimension d, minimised is
//     F(x) = omega (1/2 x^T P x - x^T rhs) + (w / 2) (v(x) - mu_v)^2 / sigma_v^2                          w = gv_weight
// NOT by the steepest descent of HTS (data-dependent step branches, thousands of sweeps, no test against "the optimum") but through
// the structure of its stationary points: grad F = 0 reads A(kappa) x = rhs with
//     A(kappa) = P + gamma E - (gamma / n) e e^T,   gamma = 2 kappa / (n omega) = 2 W kappa,   kappa = w (v(x) - mu_v) / sigma_v^2
// (e the indicator of O, E = diag(e)).  Where A is positive definite v(x(kappa)) does not increase with kappa, so
//     h(kappa) = w (v(x(kappa)) - mu_v) / sigma_v^2 - kappa
// falls strictly, h' <= -1, and has one root: a scalar root search, one banded solve per evaluation.
//
// One evaluation: B = P + gamma E is the band with a shifted diagonal on the output rows; unpivoted banded LDL^T with two right-hand
// sides gives y = B^-1 rhs and z = B^-1 e, and with c = -gamma / n (Sherman-Morrison) x = y - alpha z, alpha = c (e^T y) / (1 + c e^T z).
// B may be indefinite where A is not (short utterances at their root have one negative pivot), so feasibility is by inertia: A is
// positive definite iff (no pivot <= 0 and 1 + c e^T z > 0) or (exactly one pivot < 0, none zero, and 1 + c e^T z < 0).  v(x) comes
// from five sums over O taken in the backward sweep RELATIVE to the first output row met (the last one): sum dy, dz, dy^2, dy dz,
// dz^2 with dy = y - y_first - never sums of raw squares (csrc/gv.hip, csrc/colstats.hip).
//
// The search keeps a bracket [lo, hi], h(lo) > 0 >= h(hi) or lo infeasible:
//     v(x0) >= mu_v:  [0, w (v(x0) - mu_v) / sigma_v^2]               (x0 = MLPG's solution, the evaluation at kappa = 0)
//     otherwise:      [-omega n min_O P_tt / (2 (1 - 1/n)), 0]        (at the lower end a diagonal entry of A is zero: infeasible)
// The next point is the secant of the two ends with the Illinois halving of a retained end, or the midpoint where an end has no
// value, the secant leaves the bracket or two evaluations in a row failed to halve it.  No data leaves the thread, no atomics, the
// same branches on the same data: the same bits on every call.  It stops at h = 0, once [kappa, kappa + h] (which holds the root, by
// h' <= -1) is no wider than 2^-41 of kappa, once the bracket is no wider than 2^-40 of its larger end AND |h| meets the rule below,
// when no double is left between the ends, or when max_iter evaluations are used up; x is stored from the evaluation with the
// smallest |h| (repeated if it was not the last, which is why the search itself stops at max_iter - 1).
// Fallback, info flag 1, output = x0: n < 2, w = 0, sigma_v^2 not positive, or a search that ends with |h| > 1e-6 (1 + |kappa|) (not
// converged, or a trajectory with v = 0 whatever kappa).
//
// Two kernels and two sets of planes (workspace: 2 x mg_mlpg_workspace_bytes):
//   mlpg_gv_band_kernel    mlpg_band_kernel's text: band rows and rhs into the first set, which is KEPT
//   mlpg_gv_search_kernel  one thread per system (coalesced over systems like mlpg_solve_kernel, whose row recurrences, fetch-ahead
//                          of MLPG_ROWS rows and reciprocal these are): the whole search; each evaluation factors the shifted band
//                          into the second set (HB planes of L, two of D^-1 L^-1 [rhs e]), writes y and z of the output rows over
//                          the latter in the backward sweep, and a last pass stores x = y - alpha z.
// The rows of a system are a dependent chain: the cost is about (evaluations x one MLPG solve), accepted for a generation-time
// operator.
#include "common.h"

#define MLPG_MAX_WINDOWS MG_MLPG_MAX_WINDOWS
#define MLPG_MAX_COEFF MG_MLPG_MAX_COEFF

struct MlpgWindows {      // as csrc/mlpg.hip: mlpg_band_body.inc reads it
    int n;
    int l[MLPG_MAX_WINDOWS], u[MLPG_MAX_WINDOWS];
    double c[MLPG_MAX_WINDOWS][MLPG_MAX_COEFF];
};

template <int HB>
__global__ __launch_bounds__(256) void mlpg_gv_band_kernel(const float* __restrict__ means, const float* __restrict__ variances,
                                                           int var_per_frame, const int64_t* __restrict__ seq_len, int B, int T, int D,
                                                           MlpgWindows win, int padding, double* __restrict__ planes) {
    constexpr bool GRAD = false;
#include "mlpg_band_body.inc"
}

// rows fetched ahead per block (csrc/mlpg.hip: 8); with two right-hand sides HB = 4 holds 4 in registers, 8 spill to scratch
#define MLPG_ROWS (HB > 2 ? 4 : 8)

// 1 / d: v_rcp_f64 + two Newton steps, as csrc/mlpg.hip; d < 0 is as good as d > 0, d = 0 gives inf and the evaluation is infeasible
__device__ __forceinline__ double mlpg_gv_rcp(double d) {
    double y = __builtin_amdgcn_rcp(d);
    double e = __builtin_fma(-d, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-d, y, 1.0);
    return __builtin_fma(y, e, y);
}

#define MLPG_GV_WIDTH 0x1p-40       // the bracket is narrow enough at this fraction of its larger end
#define MLPG_GV_H_RULE 1e-6         // converged: |h| <= this (1 + |kappa|)

__global__ __launch_bounds__(256) void mlpg_gv_info_fallback_kernel(double* __restrict__ info, int S) {
    const int sys = blockIdx.x * 256 + threadIdx.x;
    if (sys >= S) return;
    info[(size_t)sys * 4 + 0] = 0.0;
    info[(size_t)sys * 4 + 1] = 0.0;
    info[(size_t)sys * 4 + 2] = 0.0;
    info[(size_t)sys * 4 + 3] = 1.0;
}

template <int HB, typename OutT>
__global__ __launch_bounds__(64) void mlpg_gv_search_kernel(const float* __restrict__ gv_mean, const float* __restrict__ gv_variance,
                                                           int gv_per_item, const int64_t* __restrict__ seq_len, int B, int T, int D,
                                                           int n_windows, int padding, double gv_weight, int max_iter,
                                                           const double* __restrict__ band, double* __restrict__ fac,
                                                           OutT* __restrict__ out, double* __restrict__ info) {
    const int S = B * D, n_max = T + 2 * padding;
    const int sys = blockIdx.x * 64 + threadIdx.x;
    if (sys >= S) return;
    const int b = sys / D, d = sys - b * D;
    const int len = (int)(seq_len ? (seq_len[b] < T ? seq_len[b] : (int64_t)T) : (int64_t)T);
    double* inf = info ? info + (size_t)sys * 4 : nullptr;
    if (len <= 0) {
        if (inf) { inf[0] = 0.0; inf[1] = 0.0; inf[2] = 0.0; inf[3] = 1.0; }
        return;
    }
    const int n = len + 2 * padding, o_lo = padding, o_hi = n - padding;      // rows, and the output rows [o_lo, o_hi)
    const size_t plane = (size_t)n_max * S;
    const double* a = band + sys;       // planes 0..HB: P[t, t-m]; plane HB + 1: rhs - read only
    double* p = fac + sys;              // planes 0..HB-1: L[i, i-1-k]; plane HB: D^-1 L^-1 rhs, then y; plane HB + 1: the same of e, then z
    const double dlen = (double)len, two_w = 2.0 * (double)n_windows;
    const double mu_v = (double)gv_mean[gv_per_item ? sys : d], sigma2 = (double)gv_variance[gv_per_item ? sys : d];
    const double w_over_s2 = gv_weight / sigma2;

    // the search's state
    int stage = 0;                      // 0: the evaluation at kappa = 0 (x0); 1: searching; 2: the evaluation whose x is stored
    int evals = 0, flag = 0, side = 0, slow = 0;
    double kappa = 0.0, lo = 0.0, hi = 0.0, flo = 0.0, fhi = 0.0, kbest = 0.0, hbest = 0.0, alpha = 0.0;
    const double INF = __builtin_huge_val();

    for (;;) {
        // ------------------------------------------------------------------------------------------ one evaluation at kappa
        const double gamma = two_w * kappa, c = -gamma / dlen;
        int nonpos = 0, neg = 0;
        double min_diag = INF;
        {
            // forward: row i of L (unit lower band), d_i and both right-hand sides, as mlpg_solve_kernel
            double lprev[HB][HB];        // lprev[r][k]: L[i-1-r, i-1-r-(k+1)]
            double yprev[HB], zprev[HB], dinv[HB];
#pragma unroll
            for (int r = 0; r < HB; ++r) {
                yprev[r] = 0.0; zprev[r] = 0.0; dinv[r] = 0.0;
#pragma unroll
                for (int k = 0; k < HB; ++k) lprev[r][k] = 0.0;
            }
            auto fwd_row = [&](const double (&r)[HB + 2], int i) __attribute__((always_inline)) {
                double lw[HB], ud[HB];       // lw[k] = L[i, i-1-k], ud[k] = lw[k] * d_{i-1-k}
#pragma unroll
                for (int m = HB - 1; m >= 0; --m) {
                    double v = r[m + 1];
#pragma unroll
                    for (int k = m + 1; k < HB; ++k) v -= ud[k] * lprev[m][k - m - 1];
                    ud[m] = v;
                    lw[m] = v * dinv[m];
                }
                const bool inside = i >= o_lo && i < o_hi;
                double di = r[0] + (inside ? gamma : 0.0), yi = r[HB + 1], zi = inside ? 1.0 : 0.0;
                min_diag = inside && r[0] < min_diag ? r[0] : min_diag;
#pragma unroll
                for (int k = 0; k < HB; ++k) {
                    di -= lw[k] * ud[k];
                    yi -= lw[k] * yprev[k];
                    zi -= lw[k] * zprev[k];
                }
                nonpos += !(di > 0.0);
                neg += di < 0.0;
                const double inv = mlpg_gv_rcp(di);
#pragma unroll
                for (int k = 0; k < HB; ++k) p[k * plane + (size_t)i * S] = lw[k];
                p[HB * plane + (size_t)i * S] = yi * inv;
                p[(HB + 1) * plane + (size_t)i * S] = zi * inv;
#pragma unroll
                for (int q = HB - 1; q > 0; --q) {
                    yprev[q] = yprev[q - 1]; zprev[q] = zprev[q - 1]; dinv[q] = dinv[q - 1];
#pragma unroll
                    for (int k = 0; k < HB; ++k) lprev[q][k] = lprev[q - 1][k];
                }
                yprev[0] = yi; zprev[0] = zi; dinv[0] = inv;
#pragma unroll
                for (int k = 0; k < HB; ++k) lprev[0][k] = lw[k];
            };
            // blocks of MLPG_ROWS rows, every load unconditional (row index clamped into [0, n)) so that the block ahead is in flight
            double cur[MLPG_ROWS][HB + 2], nxt[MLPG_ROWS][HB + 2];
#pragma unroll
            for (int r = 0; r < MLPG_ROWS; ++r)
#pragma unroll
                for (int m = 0; m < HB + 2; ++m) cur[r][m] = a[m * plane + (size_t)min(r, n - 1) * S];
            int i0 = 0;
            for (; i0 + MLPG_ROWS <= n; i0 += MLPG_ROWS) {
#pragma unroll
                for (int r = 0; r < MLPG_ROWS; ++r)
#pragma unroll
                    for (int m = 0; m < HB + 2; ++m) nxt[r][m] = a[m * plane + (size_t)min(i0 + MLPG_ROWS + r, n - 1) * S];
#pragma unroll
                for (int r = 0; r < MLPG_ROWS; ++r) fwd_row(cur[r], i0 + r);
#pragma unroll
                for (int r = 0; r < MLPG_ROWS; ++r)
#pragma unroll
                    for (int m = 0; m < HB + 2; ++m) cur[r][m] = nxt[r][m];
            }
#pragma unroll
            for (int r = 0; r < MLPG_ROWS - 1; ++r)
                if (i0 + r < n) fwd_row(cur[r], i0 + r);
        }
        double y_first = 0.0, z_first = 0.0, s_y = 0.0, s_z = 0.0, s_yy = 0.0, s_yz = 0.0, s_zz = 0.0;
        {
            // backward: both solutions; per row their D^-1 L^-1 entries (planes HB, HB + 1, row i) and L[i+1+k, i] (plane k, row i+1+k,
            // clamped past the last row where the x it multiplies is zero).  y and z of the output rows go over the entries just read
            // (the fetch-ahead reads lower rows only) for the last pass; the sums are relative to the first output row met.
            double yn[HB], zn[HB];
#pragma unroll
            for (int k = 0; k < HB; ++k) { yn[k] = 0.0; zn[k] = 0.0; }
            auto bwd_row = [&](const double (&r)[HB + 2], int i) __attribute__((always_inline)) {
                double yv = r[HB], zv = r[HB + 1];
#pragma unroll
                for (int k = 0; k < HB; ++k) {
                    yv -= r[k] * yn[k];
                    zv -= r[k] * zn[k];
                }
                if (i >= o_lo && i < o_hi) {
                    p[HB * plane + (size_t)i * S] = yv;
                    p[(HB + 1) * plane + (size_t)i * S] = zv;
                    if (i == o_hi - 1) { y_first = yv; z_first = zv; }
                    const double dy = yv - y_first, dz = zv - z_first;
                    s_y += dy; s_z += dz;
                    s_yy = __builtin_fma(dy, dy, s_yy);
                    s_yz = __builtin_fma(dy, dz, s_yz);
                    s_zz = __builtin_fma(dz, dz, s_zz);
                }
#pragma unroll
                for (int k = HB - 1; k > 0; --k) { yn[k] = yn[k - 1]; zn[k] = zn[k - 1]; }
                yn[0] = yv; zn[0] = zv;
            };
            auto bwd_load = [&](double (&r)[HB + 2], int i) __attribute__((always_inline)) {
                i = max(i, 0);
                r[HB] = p[HB * plane + (size_t)i * S];
                r[HB + 1] = p[(HB + 1) * plane + (size_t)i * S];
#pragma unroll
                for (int k = 0; k < HB; ++k) r[k] = p[k * plane + (size_t)min(i + 1 + k, n - 1) * S];
            };
            double bc[MLPG_ROWS][HB + 2], bn[MLPG_ROWS][HB + 2];
#pragma unroll
            for (int r = 0; r < MLPG_ROWS; ++r) bwd_load(bc[r], n - 1 - r);
            int i0 = n - 1;
            for (; i0 - MLPG_ROWS >= -1; i0 -= MLPG_ROWS) {
#pragma unroll
                for (int r = 0; r < MLPG_ROWS; ++r) bwd_load(bn[r], i0 - MLPG_ROWS - r);
#pragma unroll
                for (int r = 0; r < MLPG_ROWS; ++r) bwd_row(bc[r], i0 - r);
#pragma unroll
                for (int r = 0; r < MLPG_ROWS; ++r)
#pragma unroll
                    for (int k = 0; k < HB + 2; ++k) bc[r][k] = bn[r][k];
            }
#pragma unroll
            for (int r = 0; r < MLPG_ROWS - 1; ++r)
                if (i0 - r >= 0) bwd_row(bc[r], i0 - r);
        }
        // Sherman-Morrison, the inertia of A, v(x) and h
        const double e_y = __builtin_fma(dlen, y_first, s_y), e_z = __builtin_fma(dlen, z_first, s_z);
        const double sm = __builtin_fma(c, e_z, 1.0);
        alpha = c * e_y / sm;
        const double s_x = s_y - alpha * s_z, s_xx = s_yy - 2.0 * alpha * s_yz + alpha * alpha * s_zz;
        const double mean_dx = s_x / dlen, v = s_xx / dlen - mean_dx * mean_dx;
        const double h = w_over_s2 * (v - mu_v) - kappa;
        const bool feasible = ((nonpos == 0 && sm > 0.0) || (nonpos == 1 && neg == 1 && sm < 0.0)) && h == h && fabs(h) < INF;

        // ------------------------------------------------------------------------------------------ the search's step
        if (stage == 2) break;
        ++evals;
        if (stage == 0) {
            kbest = 0.0; hbest = 0.0;
            if (len < 2 || !(sigma2 > 0.0) || !(gv_weight > 0.0) || !feasible) { flag = 1; break; }       // alpha = 0: x = y = x0
            if (h == 0.0) break;
            hbest = fabs(h);
            if (h > 0.0) {
                lo = 0.0; flo = h; hi = h; fhi = -INF;
                kappa = hi;
            } else {
                hi = 0.0; fhi = h; flo = INF;
                lo = -min_diag / (two_w * (1.0 - 1.0 / dlen));
                kappa = 0.5 * (lo + hi);
            }
            stage = 1;
            continue;
        }
        const double width_before = hi - lo;
        bool stop = false, failed = false;
        if (!feasible) {
            if (kappa < 0.0) { lo = kappa; flo = INF; side = 0; }
            else { failed = true; stop = true; }             // A(kappa >= 0) is positive definite: arithmetic broke down
        } else {
            if (fabs(h) <= hbest) { kbest = kappa; hbest = fabs(h); }
            if (h > 0.0) {
                lo = kappa; flo = h;
                if (side == 1) fhi *= 0.5;
                side = 1;
            } else {
                hi = kappa; fhi = h;
                if (side == -1) flo *= 0.5;
                side = -1;
            }
            if (fabs(h) <= 0.5 * MLPG_GV_WIDTH * fabs(kappa)) stop = true;
        }
        const double width = hi - lo;
        // a narrow bracket ends the search only once |h| is converged as well: where h is steep (a tight prior far from v(x0)) 2^-40 of
        // kappa is still too coarse for it, and the search goes on for as long as there are evaluations and doubles between the ends
        if (width <= MLPG_GV_WIDTH * fmax(fabs(lo), fabs(hi)) && hbest <= MLPG_GV_H_RULE * (1.0 + fabs(kbest))) stop = true;
        if (!stop && evals < max_iter - 1) {
            slow = width > 0.5 * width_before ? slow + 1 : 0;
            double next = 0.5 * (lo + hi);
            if (fabs(flo) < INF && fabs(fhi) < INF && slow < 2) {
                const double secant = (lo * fhi - hi * flo) / (fhi - flo);
                if (secant > lo && secant < hi) next = secant;
            } else {
                slow = 0;
            }
            if (next > lo && next < hi) {
                kappa = next;
                continue;
            }
        }
        if (failed || !(hbest <= MLPG_GV_H_RULE * (1.0 + fabs(kbest)))) {
            flag = 1;
            kappa = 0.0;                 // x0 once more: the planes hold another kappa's y and z
            stage = 2;
            continue;
        }
        if (feasible && kappa == kbest) break;
        kappa = kbest;
        stage = 2;
        ++evals;
    }

    // x = y - alpha z on the output rows (alpha = 0 at kappa = 0: x0 itself, whatever z is)
    OutT* o = out + (size_t)b * T * D + d;
    const bool shift = alpha != 0.0 && flag == 0;
#pragma unroll 4
    for (int i = o_lo; i < o_hi; ++i) {
        const double yv = p[HB * plane + (size_t)i * S], zv = p[(HB + 1) * plane + (size_t)i * S];
        o[(size_t)(i - padding) * D] = (OutT)(shift ? __builtin_fma(-alpha, zv, yv) : yv);
    }
    if (inf) {
        inf[0] = kbest;
        inf[1] = hbest;
        inf[2] = (double)evals;
        inf[3] = (double)flag;
    }
}

static int mlpg_gv_half_bandwidth(int n_windows, const int* win_l, const int* win_u) {
    int hb = 0;
    for (int w = 0; w < n_windows; ++w) hb = win_l[w] + win_u[w] > hb ? win_l[w] + win_u[w] : hb;
    return hb <= 2 ? 2 : 4;
}

extern "C" {

// two sets of mg_mlpg_f32's planes: the band (kept) and the factor of the shifted band with both solutions
size_t mg_mlpg_gv_workspace_bytes(int B, int T, int D, int padding, int n_windows, const int* win_l, const int* win_u) {
    return 2 * mg_mlpg_workspace_bytes(B, T, D, padding, n_windows, win_l, win_u);
}

int mg_mlpg_gv_f32(const float* means, const float* variances, int var_per_frame, const float* gv_mean, const float* gv_variance,
                   int gv_per_item, const int64_t* seq_len, int B, int T, int D, int n_windows, const int* win_l, const int* win_u,
                   const double* win_coeff, int padding, double gv_weight, int max_iter, void* out, int out_f64, double* info,
                   void* workspace, size_t workspace_bytes, void* stream) {
    MG_CHECK_ARG(means && variances && gv_mean && gv_variance && out && win_l && win_u && win_coeff, "mg_mlpg_gv_f32: null argument");
    MG_CHECK_ARG(B > 0 && T > 0 && D > 0 && padding >= 0, "mg_mlpg_gv_f32: bad shape (B=%d T=%d D=%d padding=%d)", B, T, D, padding);
    MG_CHECK_ARG(n_windows > 0 && n_windows <= MLPG_MAX_WINDOWS, "mg_mlpg_gv_f32: 1..%d windows supported, got %d", MLPG_MAX_WINDOWS,
                 n_windows);
    MG_CHECK_ARG(gv_weight >= 0.0 && gv_weight < __builtin_huge_val(), "mg_mlpg_gv_f32: gv_weight must be finite and >= 0, got %g",
                 gv_weight);
    MG_CHECK_ARG(max_iter >= 3, "mg_mlpg_gv_f32: max_iter must be at least 3 (x0, one search point, the stored one), got %d", max_iter);
    MlpgWindows win = {};
    win.n = n_windows;
    for (int w = 0; w < n_windows; ++w) {
        MG_CHECK_ARG(win_l[w] >= 0 && win_u[w] >= 0 && win_l[w] + win_u[w] + 1 <= MLPG_MAX_COEFF,
                     "mg_mlpg_gv_f32: window %d (l=%d, u=%d) is wider than %d coefficients", w, win_l[w], win_u[w], MLPG_MAX_COEFF);
        win.l[w] = win_l[w];
        win.u[w] = win_u[w];
        for (int k = 0; k <= win_l[w] + win_u[w]; ++k) win.c[w][k] = win_coeff[w * MLPG_MAX_COEFF + k];
    }
    const size_t need = mg_mlpg_gv_workspace_bytes(B, T, D, padding, n_windows, win_l, win_u);
    MG_CHECK_ARG((size_t)(T + 2 * padding) * (size_t)B * D < ((size_t)1 << 31), "mg_mlpg_gv_f32: too many unknowns for 32-bit frame x system ids");
    if (!workspace || workspace_bytes < need) {
        mg_set_error("mg_mlpg_gv_f32: workspace of %zu bytes needed, got %zu", need, workspace_bytes);
        return MG_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    if (gv_weight == 0.0) {                  // no prior: MLPG itself, bit for bit, and every system reports the fallback
        const int rc = mg_mlpg_f32(means, variances, var_per_frame, seq_len, B, T, D, n_windows, win_l, win_u, win_coeff, padding, out,
                                   out_f64, workspace, workspace_bytes, stream);
        if (rc != MG_OK) return rc;
        if (info) {
            hipLaunchKernelGGL(mlpg_gv_info_fallback_kernel, dim3((unsigned)mg_ceil_div((int64_t)B * D, 256)), dim3(256), 0, st, info,
                               B * D);
            MG_CHECK_LAUNCH("mg_mlpg_gv_f32");
        }
        return MG_OK;
    }
    const size_t out_bytes = (size_t)B * T * D * (out_f64 ? sizeof(double) : sizeof(float));
    if (hipMemsetAsync(out, 0, out_bytes, st) != hipSuccess) {           // frames past seq_len stay zero
        mg_set_error("mg_mlpg_gv_f32: memset failed");
        return MG_ELAUNCH;
    }
    const int hb = mlpg_gv_half_bandwidth(n_windows, win_l, win_u);
    const int64_t cells = (int64_t)(T + 2 * padding) * B * D;
    const unsigned grid_a = (unsigned)mg_ceil_div(cells, 256), grid_b = (unsigned)mg_ceil_div((int64_t)B * D, 64);
    double* band = (double*)workspace;
    double* fac = band + (size_t)(hb + 2) * (size_t)(T + 2 * padding) * B * D;
#define MLPG_GV_RUN(HB)                                                                                                               \
    do {                                                                                                                              \
        hipLaunchKernelGGL((mlpg_gv_band_kernel<HB>), dim3(grid_a), dim3(256), 0, st, means, variances, var_per_frame, seq_len, B, T,  \
                           D, win, padding, band);                                                                                    \
        if (out_f64)                                                                                                                  \
            hipLaunchKernelGGL((mlpg_gv_search_kernel<HB, double>), dim3(grid_b), dim3(64), 0, st, gv_mean, gv_variance, gv_per_item,  \
                               seq_len, B, T, D, n_windows, padding, gv_weight, max_iter, band, fac, (double*)out, info);             \
        else                                                                                                                          \
            hipLaunchKernelGGL((mlpg_gv_search_kernel<HB, float>), dim3(grid_b), dim3(64), 0, st, gv_mean, gv_variance, gv_per_item,   \
                               seq_len, B, T, D, n_windows, padding, gv_weight, max_iter, band, fac, (float*)out, info);              \
    } while (0)
    if (hb == 2)
        MLPG_GV_RUN(2);
    else
        MLPG_GV_RUN(4);
    MG_CHECK_LAUNCH("mg_mlpg_gv_f32");
    return MG_OK;
}

}  // extern "C"
