// The body of mlpg_band_kernel and of either half of mlpg_band_pair_kernel (csrc/mlpg.hip), textually: HB, GRAD, means, variances,
// var_per_frame, seq_len, B, T, D, win, padding and planes are the including kernel's.  Text and not a device function, so that the
// single-system kernels compile to the very instructions they compiled to before the pair kernels existed.
    const int S = B * D, n_max = T + 2 * padding;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)n_max * S) return;
    const int t = (int)(gid / S), sys = (int)(gid - (int64_t)t * S);
    const int b = sys / D, d = sys - b * D;
    const int len = (int)(seq_len ? (seq_len[b] < T ? seq_len[b] : (int64_t)T) : (int64_t)T);
    if (len <= 0) return;
    const int n = len + 2 * padding;
    if (t >= n) return;
    const int width = win.n * D;
    double band[HB + 1], rhs = 0.0;
#pragma unroll
    for (int m = 0; m <= HB; ++m) band[m] = 0.0;
    for (int w = 0; w < win.n; ++w) {
        const int l = win.l[w], u = win.u[w];
        for (int k = -l; k <= u; ++k) {                       // row s = t - k of W_w has a coefficient in column t
            const int s = t - k;
            if (s < 0 || s >= n) continue;
            int f = s - padding;
            f = f < 0 ? 0 : (f >= len ? len - 1 : f);
            const size_t at = ((size_t)b * T + f) * width + (size_t)w * D + d;
            const float var = var_per_frame == MG_MLPG_VAR_ITEM ? variances[(size_t)b * width + w * D + d]
                              : var_per_frame ? variances[at] : variances[w * D + d];
            const float tau = 1.0f / var;                                     // float32, as numpy does on the model's arrays
            const double ck = win.c[w][l + k];
            if constexpr (!GRAD) {
                const float mu_tau = means[at] / var;
                rhs += ck * (double)mu_tau;
            }
#pragma unroll
            for (int m = 0; m <= HB; ++m) {
                const int k2 = l + k - m;
                if (t - m >= 0 && k2 >= 0 && k2 <= l + u) band[m] += (double)tau * ck * win.c[w][k2];
            }
        }
    }
    if constexpr (GRAD)
        if (t >= padding && t < n - padding) rhs = (double)means[((size_t)b * T + (t - padding)) * D + d];       // frame t - padding < len
#pragma unroll
    for (int m = 0; m <= HB; ++m) planes[((size_t)m * n_max + t) * S + sys] = band[m];
    planes[((size_t)(HB + 1) * n_max + t) * S + sys] = rhs;
