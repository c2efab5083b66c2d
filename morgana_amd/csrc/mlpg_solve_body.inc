// The body of mlpg_solve_kernel and of mlpg_solve_pair_kernel (csrc/mlpg.hip), textually: HB, OutT, KEEP, seq_len, B, T, D, padding,
// planes and out are the including kernel's (see mlpg_band_body.inc for why it is text).
    const int S = B * D, n_max = T + 2 * padding;
    const int sys = blockIdx.x * 64 + threadIdx.x;
    if (sys >= S) return;
    const int b = sys / D, d = sys - b * D;
    const int len = (int)(seq_len ? (seq_len[b] < T ? seq_len[b] : (int64_t)T) : (int64_t)T);
    if (len <= 0) return;
    const int n = len + 2 * padding;
    const size_t plane = (size_t)n_max * S;
    double* p = planes + sys;

    // forward: row i of L (unit lower band), d_i, y_i; L[i, i-1-k] goes to plane k + 1, z_i = y_i / d_i to plane HB + 1
    double lprev[HB][HB];        // lprev[r][k]: L[i-1-r, i-1-r-(k+1)]
    double yprev[HB], dinv[HB];
#pragma unroll
    for (int r = 0; r < HB; ++r) {
        yprev[r] = 0.0; dinv[r] = 0.0;
#pragma unroll
        for (int k = 0; k < HB; ++k) lprev[r][k] = 0.0;
    }
    // one row of the factorisation from its band row a[0..HB] and right-hand side a[HB + 1]
    auto fwd_row = [&](const double (&a)[HB + 2], int i) __attribute__((always_inline)) {
        double lw[HB], ud[HB];       // lw[k] = L[i, i-1-k], ud[k] = lw[k] * d_{i-1-k}
#pragma unroll
        for (int m = HB - 1; m >= 0; --m) {           // columns i-HB .. i-1 in increasing order
            double v = a[m + 1];
#pragma unroll
            for (int k = m + 1; k < HB; ++k) v -= ud[k] * lprev[m][k - m - 1];
            ud[m] = v;
            lw[m] = v * dinv[m];                      // dinv = 0 for rows before the first: those entries are 0 anyway
        }
        double di = a[0], yi = a[HB + 1];
#pragma unroll
        for (int k = 0; k < HB; ++k) {
            di -= lw[k] * ud[k];
            yi -= lw[k] * yprev[k];
        }
        const double inv = mlpg_rcp(di);
#pragma unroll
        for (int k = 0; k < HB; ++k) p[(k + 1) * plane + (size_t)i * S] = lw[k];
        p[(HB + 1) * plane + (size_t)i * S] = yi * inv;
#pragma unroll
        for (int q = HB - 1; q > 0; --q) {
            yprev[q] = yprev[q - 1]; dinv[q] = dinv[q - 1];
#pragma unroll
            for (int k = 0; k < HB; ++k) lprev[q][k] = lprev[q - 1][k];
        }
        yprev[0] = yi; dinv[0] = inv;
#pragma unroll
        for (int k = 0; k < HB; ++k) lprev[0][k] = lw[k];
    };
    // blocks of MLPG_ROWS rows; every load is unconditional (row index clamped) so that the block ahead is in flight while this
    // one's chain runs - with per-row branches the compiler drains the memory queue (vmcnt(0)) before the first row
    double cur[MLPG_ROWS][HB + 2], nxt[MLPG_ROWS][HB + 2];
#pragma unroll
    for (int r = 0; r < MLPG_ROWS; ++r)
#pragma unroll
        for (int m = 0; m < HB + 2; ++m) cur[r][m] = p[m * plane + (size_t)min(r, n - 1) * S];
    int i0 = 0;
    for (; i0 + MLPG_ROWS <= n; i0 += MLPG_ROWS) {
#pragma unroll
        for (int r = 0; r < MLPG_ROWS; ++r)
#pragma unroll
            for (int m = 0; m < HB + 2; ++m) nxt[r][m] = p[m * plane + (size_t)min(i0 + MLPG_ROWS + r, n - 1) * S];
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

    // backward: x_i = z_i - sum_k L[i+1+k, i] x_{i+1+k}; per row z_i (plane HB + 1, row i) and L[i+1+k, i] (plane k + 1, row i+1+k,
    // zero past the last row: those x are zero too, so the clamped load is harmless)
    double xn[HB];
#pragma unroll
    for (int k = 0; k < HB; ++k) xn[k] = 0.0;
    OutT* o = out + (size_t)b * T * D + d;
    auto bwd_row = [&](const double (&a)[HB + 1], int i) __attribute__((always_inline)) {
        double x = a[HB];
#pragma unroll
        for (int k = 0; k < HB; ++k) x -= a[k] * xn[k];
        if constexpr (KEEP)
            p[(HB + 1) * plane + (size_t)i * S] = x;
        else if (i >= padding && i < n - padding)
            o[(size_t)(i - padding) * D] = (OutT)x;
#pragma unroll
        for (int k = HB - 1; k > 0; --k) xn[k] = xn[k - 1];
        xn[0] = x;
    };
    auto bwd_load = [&](double (&a)[HB + 1], int i) __attribute__((always_inline)) {
        i = max(i, 0);
        a[HB] = p[(HB + 1) * plane + (size_t)i * S];
#pragma unroll
        for (int k = 0; k < HB; ++k) a[k] = p[(k + 1) * plane + (size_t)min(i + 1 + k, n - 1) * S];
    };
    double bc[MLPG_ROWS][HB + 1], bn[MLPG_ROWS][HB + 1];
#pragma unroll
    for (int r = 0; r < MLPG_ROWS; ++r) bwd_load(bc[r], n - 1 - r);
    i0 = n - 1;
    for (; i0 - MLPG_ROWS >= -1; i0 -= MLPG_ROWS) {
#pragma unroll
        for (int r = 0; r < MLPG_ROWS; ++r) bwd_load(bn[r], i0 - MLPG_ROWS - r);
#pragma unroll
        for (int r = 0; r < MLPG_ROWS; ++r) bwd_row(bc[r], i0 - r);
#pragma unroll
        for (int r = 0; r < MLPG_ROWS; ++r)
#pragma unroll
            for (int k = 0; k <= HB; ++k) bc[r][k] = bn[r][k];
    }
#pragma unroll
    for (int r = 0; r < MLPG_ROWS - 1; ++r)
        if (i0 - r >= 0) bwd_row(bc[r], i0 - r);
