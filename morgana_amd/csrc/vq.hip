// K28 - vector quantisation for VQ-VAE latents, functional.VQFn (van den Oord et al. 2017; the reference has no discrete latent): nearest
// code, quantised rows, loss and usage; the gradients; the EMA codebook of the paper's appendix.
//
//   d[n,k]   = sum_d ( (double)z[n,d] - (double)E[k,d] )^2        ascending d, float64, the DIRECT difference (no |z|^2 - 2 z.e + |e|^2:
//                                                                  codes 1e-3 apart at offset 1e3 differ in the 20th bit of that form)
//   index[n] = the smallest k that attains min_k d[n,k];  a NaN distance never wins;  all NaN: code 0 and a NaN loss
//   q[n]     = E[index[n]]                                         copied, bit for bit
//   vq       = sum_n d[n,index[n]] / (N_valid D),   perplexity = exp( - sum_k p_k ln p_k ),  p_k = counts[k] / N_valid
//
// Assignment, three launches.  (1) vq_assign_kernel: a workgroup owns `rpb` rows (its four waves take them in turn, ONE WAVE PER
// ROW), stages the rows once and the codebook tile by tile in LDS (rows padded to an odd stride: lane l reads code l's column d on
// bank (l Dp + d) % 32, all different inside a half wave), lane l scores codes l, l + 64, ... of the tile and the wave reduces
// (distance, index) by "smaller distance, then smaller index" - an order on pairs, so the result does not depend on the tile size,
// on rpb or on which lane held what.  It writes index, q and the winner's distance (float64, workspace).  (2) vq_count_kernel,
// grid (row chunks, code groups): the chunk's indices in LDS, one thread per code counts them; the y == 0 workgroups sum the chunk's
// distances - thread t the rows t, t + 256, ... in ascending order, then the fixed tree of seq_reduce.h.  (3) vq_finish_kernel, one
// workgroup: N_valid from seq_len, the chunks in ascending order, the two scalars in float64, rounded once.  No atomics, no host
// read: the same bits on every call, capturable.  Floating-point contraction is off: a distance is the rounded square added to the
// rounded sum, as a float64 restatement on the host computes it.
//
// Rows at or past seq_len[b] of a (B, S, D) input are never read: index -1, a zero row, no part in any mean or count.
#include "common.h"

#pragma clang fp contract(off)
#include "seq_reduce.h"

#define VQ_THREADS 256
#define VQ_TILE_FLOATS 8192        // one codebook tile in LDS (32 KB): floor(8192 / Dp) codes
#define VQ_ROWS_FLOATS 4096        // the workgroup's rows in LDS (16 KB)
#define VQ_MAX_RPB 32              // rows per workgroup, at most
#define VQ_CHUNK 2048              // rows per workgroup of the counting launch
#define VQ_NO_CODE 0x7fffffff

static inline int vq_dp(int D) { return D | 1; }                                        // the odd LDS row stride
static inline int vq_tile_codes(int D) { return VQ_TILE_FLOATS / vq_dp(D); }
static inline int64_t vq_chunks(int64_t N) { return mg_ceil_div(N, VQ_CHUNK); }

// The assignment's workspace, each part behind a 256-byte boundary: the winners' distances [N] float64, the chunks' loss sums
// [chunks] float64, the chunks' counts [chunks][K] int32.  (The EMA launches need one float64 of their own: the sum of the new sizes.)
static inline size_t vq_dist_bytes(int64_t N) { return mg_align_up((size_t)N * sizeof(double), 256); }
static inline size_t vq_part_bytes(int64_t N) { return mg_align_up((size_t)vq_chunks(N) * sizeof(double), 256); }
static inline size_t vq_ws_bytes(int64_t N, int K) {
    return vq_dist_bytes(N) + vq_part_bytes(N) + mg_align_up((size_t)vq_chunks(N) * (size_t)K * sizeof(int32_t), 256);
}

__device__ __forceinline__ void vq_merge(double& bd, int& bk, double d, int k) {
    if (d < bd || (d == bd && k < bk)) {        // false for a NaN d: it never wins
        bd = d;
        bk = k;
    }
}

// row n of a (B, S, D) input with lengths: is it a frame of its item?  (seq_len NULL: every row is)
__device__ __forceinline__ bool vq_row_valid(const int64_t* __restrict__ seq_len, int64_t n, int S) {
    if (!seq_len) return true;
    const int64_t b = n / S;
    return n - b * S < mg_valid_frames(seq_len, (int)b, S);
}

__global__ __launch_bounds__(VQ_THREADS) void vq_assign_kernel(const float* __restrict__ z, int64_t ldz, int64_t N, int D,
                                                               const int64_t* __restrict__ seq_len, int S,
                                                               const float* __restrict__ E, int K, int TK, int rpb,
                                                               int64_t* __restrict__ index, float* __restrict__ quant,
                                                               double* __restrict__ dist) {
    __shared__ float s_e[VQ_TILE_FLOATS];
    __shared__ float s_z[VQ_ROWS_FLOATS];
    __shared__ double s_best[VQ_MAX_RPB];
    __shared__ int s_k[VQ_MAX_RPB];
    __shared__ int s_valid[VQ_MAX_RPB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Dp = D | 1;
    const int64_t row0 = (int64_t)blockIdx.x * rpb;
    if (tid < rpb) {
        const int64_t n = row0 + tid;
        s_valid[tid] = n < N && vq_row_valid(seq_len, n, S);
        s_best[tid] = __builtin_inf();
        s_k[tid] = VQ_NO_CODE;
    }
    __syncthreads();
    for (int i = tid; i < rpb * D; i += VQ_THREADS) {
        const int r = i / D, d = i - r * D;
        if (s_valid[r]) s_z[r * Dp + d] = z[(row0 + r) * ldz + d];      // pad rows are not read
    }
    for (int k0 = 0; k0 < K; k0 += TK) {
        const int tk = K - k0 < TK ? K - k0 : TK;
        __syncthreads();                                                  // the rows are in place; the last tile has been read
        const float* tile = E + (int64_t)k0 * D;
        for (int i = tid; i < tk * D; i += VQ_THREADS) {
            const int c = i / D, d = i - c * D;
            s_e[c * Dp + d] = tile[i];
        }
        __syncthreads();
        for (int r = wave; r < rpb; r += VQ_THREADS / 64) {
            if (!s_valid[r]) continue;                                    // wave-uniform
            const float* zr = s_z + r * Dp;
            double bd = __builtin_inf();
            int bk = VQ_NO_CODE;
            for (int c = lane; c < tk; c += 64) {
                const float* e = s_e + c * Dp;
                double acc = 0.0;
                for (int d = 0; d < D; ++d) {
                    const double df = (double)zr[d] - (double)e[d];
                    acc += df * df;
                }
                vq_merge(bd, bk, acc, k0 + c);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double od = __shfl_xor(bd, off, 64);
                const int ok = __shfl_xor(bk, off, 64);
                vq_merge(bd, bk, od, ok);
            }
            if (lane == 0) {                                              // row r is this wave's alone
                double cd = s_best[r];
                int ck = s_k[r];
                vq_merge(cd, ck, bd, bk);
                s_best[r] = cd;
                s_k[r] = ck;
            }
        }
    }
    __syncthreads();
    for (int r = wave; r < rpb; r += VQ_THREADS / 64) {
        const int64_t n = row0 + r;
        if (n >= N) continue;
        float* q = quant + n * D;
        if (!s_valid[r]) {
            for (int d = lane; d < D; d += 64) q[d] = 0.f;
            if (lane == 0) {
                index[n] = -1;
                dist[n] = 0.0;
            }
            continue;
        }
        const int k = s_k[r] == VQ_NO_CODE ? 0 : s_k[r];                 // every distance NaN: code 0 ...
        const float* e = E + (int64_t)k * D;
        for (int d = lane; d < D; d += 64) q[d] = e[d];
        if (lane == 0) {
            index[n] = k;
            dist[n] = s_k[r] == VQ_NO_CODE ? __builtin_nan("") : s_best[r];      // ... and a NaN loss
        }
    }
}

// grid (chunks of VQ_CHUNK rows, groups of 256 codes): part_counts[chunk][k], and from the y == 0 workgroups part_loss[chunk]
__global__ __launch_bounds__(VQ_THREADS) void vq_count_kernel(const int64_t* __restrict__ index, const double* __restrict__ dist, int64_t N,
                                                              int K, int32_t* __restrict__ part_counts, double* __restrict__ part_loss) {
    __shared__ int s_idx[VQ_CHUNK];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int64_t n0 = (int64_t)blockIdx.x * VQ_CHUNK;
    const int len = (int)(N - n0 < VQ_CHUNK ? N - n0 : VQ_CHUNK);
    for (int i = tid; i < len; i += VQ_THREADS) s_idx[i] = (int)index[n0 + i];
    __syncthreads();
    const int k = (int)blockIdx.y * VQ_THREADS + tid;
    if (k < K) {
        int c = 0;
        for (int i = 0; i < len; ++i) c += s_idx[i] == k;
        part_counts[(size_t)blockIdx.x * K + k] = c;
    }
    if (blockIdx.y == 0) {
        double acc = 0.0;
        for (int i = tid; i < len; i += VQ_THREADS) acc += dist[n0 + i];
        const double sum = mg_block_sum_f64(acc, red);
        if (tid == 0) part_loss[blockIdx.x] = sum;
    }
}

// int64 sum over the workgroup (integers: any order gives the same value); red: 256 entries of LDS
__device__ __forceinline__ int64_t vq_block_sum_i64(int64_t v, int64_t* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int off = VQ_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ int64_t vq_count_valid(const int64_t* __restrict__ seq_len, int64_t N, int S, int64_t* red) {
    if (!seq_len) return N;
    const int B = (int)(N / S);
    int64_t mine = 0;
    for (int b = threadIdx.x; b < B; b += VQ_THREADS) mine += mg_valid_frames(seq_len, b, S);
    return vq_block_sum_i64(mine, red);
}

__global__ __launch_bounds__(VQ_THREADS) void vq_finish_kernel(const int64_t* __restrict__ seq_len, int64_t N, int S, int D, int K,
                                                               int64_t chunks, const int32_t* __restrict__ part_counts,
                                                               const double* __restrict__ part_loss, float* __restrict__ vq,
                                                               int32_t* __restrict__ counts, float* __restrict__ perplexity,
                                                               int64_t* __restrict__ n_valid) {
    __shared__ int64_t red_i[VQ_THREADS];
    __shared__ double red_a[4], red_b[4];
    const int tid = threadIdx.x;
    const int64_t nv = vq_count_valid(seq_len, N, S, red_i);
    double ent = 0.0;
    for (int k = tid; k < K; k += VQ_THREADS) {
        int c = 0;
        for (int64_t ch = 0; ch < chunks; ++ch) c += part_counts[(size_t)ch * K + k];
        counts[k] = c;
        if (c > 0) {
            const double p = (double)c / (double)nv;
            ent += p * log(p);
        }
    }
    double loss = 0.0;
    for (int64_t ch = tid; ch < chunks; ch += VQ_THREADS) loss += part_loss[ch];
    const double ent_all = mg_block_sum_f64(ent, red_a);
    const double loss_all = mg_block_sum_f64(loss, red_b);
    if (tid == 0) {
        vq[0] = (float)(loss_all / ((double)nv * (double)D));                        // no valid row: 0 / 0
        perplexity[0] = nv > 0 ? (float)exp(-ent_all) : __builtin_nanf("");
        n_valid[0] = nv;
    }
}

// dz[n,d] = (float)( g_lat[n,d] + g beta 2 (z[n,d] - q[n,d]) / (N_valid D) ), one thread per element; zeros on pad rows
__global__ __launch_bounds__(VQ_THREADS) void vq_dz_kernel(const float* __restrict__ g_lat, const float* __restrict__ g_loss,
                                                           const float* __restrict__ z, int64_t ldz, const float* __restrict__ quant,
                                                           const int64_t* __restrict__ index, const int64_t* __restrict__ n_valid, int64_t N,
                                                           int D, double commitment_weight, float* __restrict__ dz) {
    const int64_t i = (int64_t)blockIdx.x * VQ_THREADS + threadIdx.x;
    if (i >= N * D) return;
    const int64_t n = i / D;
    const int d = (int)(i - n * D);
    if (index[n] < 0) {
        dz[i] = 0.f;
        return;
    }
    const double scale = (double)g_loss[0] * commitment_weight * 2.0 / ((double)n_valid[0] * (double)D);
    const double up = g_lat ? (double)g_lat[i] : 0.0;
    dz[i] = (float)(up + scale * ((double)z[n * ldz + d] - (double)quant[i]));
}

// One workgroup per code: the members of code k in ASCENDING n.  The workgroup walks the indices 256 at a time; the matching rows
// of a step are compacted, in order, into s_mem (ballot and prefix counts: no atomics), and thread d < D adds row after row of it
// into its float64 sum of column d.  `term(n, d)` is what a member contributes.  Returns the member count (in every thread).
template <typename Term>
__device__ __forceinline__ int64_t vq_member_sum(const int64_t* __restrict__ index, int64_t N, int D, int k, double& acc, Term term) {
    __shared__ int s_mem[VQ_THREADS];
    __shared__ int s_cnt[VQ_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t members = 0;
    acc = 0.0;
    for (int64_t n0 = 0; n0 < N; n0 += VQ_THREADS) {
        const int64_t n = n0 + tid;
        const bool mine = n < N && index[n] == (int64_t)k;
        const unsigned long long bal = __ballot(mine);
        if (lane == 0) s_cnt[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < VQ_THREADS / 64; ++w) {
            if (w < wave) before += s_cnt[w];
            total += s_cnt[w];
        }
        if (mine) s_mem[before + __popcll(bal & ((1ull << lane) - 1ull))] = tid;
        __syncthreads();
        if (tid < D)
            for (int j = 0; j < total; ++j) acc += term(n0 + s_mem[j], tid);
        members += total;
        __syncthreads();                                                  // s_cnt and s_mem are rewritten by the next step
    }
    return members;
}

// grid (K): dE[k,d] = (float)( g cw 2 sum_{n in k} (q[n,d] - z[n,d]) / (N_valid D) ), q[n] being E[k] as the assignment read it;
// exactly 0 for a code without members
__global__ __launch_bounds__(VQ_THREADS) void vq_de_kernel(const float* __restrict__ g_loss, const float* __restrict__ z, int64_t ldz,
                                                           const float* __restrict__ quant, const int64_t* __restrict__ index,
                                                           const int64_t* __restrict__ n_valid, int64_t N, int D, double codebook_weight,
                                                           float* __restrict__ dE) {
    const int k = blockIdx.x;
    double acc;
    const int64_t members = vq_member_sum(index, N, D, k, acc, [&](int64_t n, int d) { return (double)quant[n * D + d] - (double)z[n * ldz + d]; });
    if ((int)threadIdx.x >= D) return;
    const double scale = (double)g_loss[0] * codebook_weight * 2.0 / ((double)n_valid[0] * (double)D);
    dE[(int64_t)k * D + threadIdx.x] = members > 0 ? (float)(scale * acc) : 0.f;
}

// EMA, launch 1 (one workgroup): cluster_size[k] <- gamma n_k + (1 - gamma) counts[k], in place, and the sum of the new sizes
__global__ __launch_bounds__(VQ_THREADS) void vq_ema_sizes_kernel(const int32_t* __restrict__ counts, int K, double decay,
                                                                  float* __restrict__ cluster_size, double* __restrict__ total) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int k = threadIdx.x; k < K; k += VQ_THREADS) {
        const float now = (float)(decay * (double)cluster_size[k] + (1.0 - decay) * (double)counts[k]);
        cluster_size[k] = now;
        acc += (double)now;
    }
    const double sum = mg_block_sum_f64(acc, red);
    if (threadIdx.x == 0) total[0] = sum;
}

// EMA, launch 2, grid (K): ema_sum[k] <- gamma m_k + (1 - gamma) sum_{n in k} z[n];  codebook[k] <- that / the smoothed size
__global__ __launch_bounds__(VQ_THREADS) void vq_ema_codes_kernel(const float* __restrict__ z, int64_t ldz, const int64_t* __restrict__ index,
                                                                  int64_t N, int D, int K, double decay, double eps,
                                                                  const float* __restrict__ cluster_size, const double* __restrict__ total,
                                                                  float* __restrict__ ema_sum, float* __restrict__ codebook) {
    const int k = blockIdx.x;
    double acc;
    vq_member_sum(index, N, D, k, acc, [&](int64_t n, int d) { return (double)z[n * ldz + d]; });
    if ((int)threadIdx.x >= D) return;
    const int64_t at = (int64_t)k * D + threadIdx.x;
    const double m = decay * (double)ema_sum[at] + (1.0 - decay) * acc;
    const double all = total[0];
    const double size = ((double)cluster_size[k] + eps) / (all + (double)K * eps) * all;
    ema_sum[at] = (float)m;
    if (size > 0.0) codebook[at] = (float)(m / size);                    // all sizes 0 (nothing ever assigned): the code stays
}

extern "C" {

int mg_vq_tile_codes(int D) { return D > 0 && D <= MG_VQ_MAX_DIM ? vq_tile_codes(D) : 0; }

size_t mg_vq_workspace_bytes(int64_t N, int K) { return N > 0 && K > 0 && K <= MG_VQ_MAX_CODES ? vq_ws_bytes(N, K) : 0; }

int mg_vq_assign_f32(const float* z, int64_t ldz, int64_t N, int D, const int64_t* seq_len, int S, const float* codebook, int K,
                     int64_t* index, float* quantised, float* vq, int32_t* counts, float* perplexity, int64_t* n_valid, void* workspace,
                     size_t workspace_bytes, void* stream) {
    MG_CHECK_ARG(z && codebook && index && quantised && vq && counts && perplexity && n_valid,
                 "mg_vq_assign_f32: z, codebook, index, quantised, vq, counts, perplexity and n_valid must not be NULL");
    MG_CHECK_ARG(N > 0 && D > 0 && K > 0, "mg_vq_assign_f32: bad shape (N=%lld D=%d K=%d)", (long long)N, D, K);
    MG_CHECK_ARG(K <= MG_VQ_MAX_CODES, "mg_vq_assign_f32: K=%d exceeds %d (MG_VQ_MAX_CODES)", K, MG_VQ_MAX_CODES);
    MG_CHECK_ARG(D <= MG_VQ_MAX_DIM, "mg_vq_assign_f32: D=%d exceeds %d (MG_VQ_MAX_DIM)", D, MG_VQ_MAX_DIM);
    MG_CHECK_ARG(N <= MG_VQ_MAX_ROWS, "mg_vq_assign_f32: N=%lld exceeds %lld (MG_VQ_MAX_ROWS)", (long long)N, (long long)MG_VQ_MAX_ROWS);
    MG_CHECK_ARG(ldz >= D, "mg_vq_assign_f32: row stride %lld is below D=%d (negative and overlapping strides are refused)", (long long)ldz, D);
    MG_CHECK_ARG(!seq_len || (S > 0 && N % S == 0), "mg_vq_assign_f32: with seq_len, N=%lld must be B rows of S=%d", (long long)N, S);
    MG_CHECK_ARG(((uintptr_t)z & 3u) == 0 && ((uintptr_t)codebook & 3u) == 0 && ((uintptr_t)quantised & 3u) == 0 && ((uintptr_t)vq & 3u) == 0 &&
                     ((uintptr_t)counts & 3u) == 0 && ((uintptr_t)perplexity & 3u) == 0 && ((uintptr_t)index & 7u) == 0 &&
                     ((uintptr_t)n_valid & 7u) == 0 && ((uintptr_t)seq_len & 7u) == 0 && ((uintptr_t)workspace & 7u) == 0,
                 "mg_vq_assign_f32: float32 and int32 operands must be 4-byte, index, n_valid, seq_len and the workspace 8-byte aligned");
    if (!workspace || workspace_bytes < vq_ws_bytes(N, K)) {
        mg_set_error("mg_vq_assign_f32: workspace of %zu bytes needed, got %zu", vq_ws_bytes(N, K), workspace ? workspace_bytes : (size_t)0);
        return MG_EWORKSPACE;
    }
    const int Dp = vq_dp(D);
    int rpb = VQ_ROWS_FLOATS / Dp;
    if (rpb > VQ_MAX_RPB) rpb = VQ_MAX_RPB;
    rpb -= rpb % 4;                                                        // >= 12 at D = MG_VQ_MAX_DIM
    while (rpb > 4 && mg_ceil_div(N, rpb) < 1024) rpb -= 4;               // few rows: more workgroups, each staging the codebook itself
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    double* dist = (double*)ws;
    double* part_loss = (double*)(ws + vq_dist_bytes(N));
    int32_t* part_counts = (int32_t*)(ws + vq_dist_bytes(N) + vq_part_bytes(N));
    const int64_t chunks = vq_chunks(N);
    hipLaunchKernelGGL(vq_assign_kernel, dim3((unsigned)mg_ceil_div(N, rpb)), dim3(VQ_THREADS), 0, st, z, ldz, N, D, seq_len, S, codebook, K,
                       vq_tile_codes(D), rpb, index, quantised, dist);
    MG_CHECK_LAUNCH("mg_vq_assign_f32/assign");
    hipLaunchKernelGGL(vq_count_kernel, dim3((unsigned)chunks, (unsigned)mg_ceil_div(K, VQ_THREADS)), dim3(VQ_THREADS), 0, st,
                       (const int64_t*)index, (const double*)dist, N, K, part_counts, part_loss);
    MG_CHECK_LAUNCH("mg_vq_assign_f32/count");
    hipLaunchKernelGGL(vq_finish_kernel, dim3(1), dim3(VQ_THREADS), 0, st, seq_len, N, S, D, K, chunks, (const int32_t*)part_counts,
                       (const double*)part_loss, vq, counts, perplexity, n_valid);
    MG_CHECK_LAUNCH("mg_vq_assign_f32/finish");
    return MG_OK;
}

int mg_vq_bwd_f32(const float* g_lat, const float* g_loss, const float* z, int64_t ldz, const float* quantised, const int64_t* index,
                  const int64_t* n_valid, int64_t N, int D, int K, double codebook_weight, double commitment_weight, float* dz, float* dE,
                  void* stream) {
    MG_CHECK_ARG(g_loss && z && quantised && index && n_valid, "mg_vq_bwd_f32: g_loss, z, quantised, index and n_valid must not be NULL");
    MG_CHECK_ARG(dz || dE, "mg_vq_bwd_f32: one of dz and dE must be given");
    MG_CHECK_ARG(N > 0 && D > 0 && K > 0, "mg_vq_bwd_f32: bad shape (N=%lld D=%d K=%d)", (long long)N, D, K);
    MG_CHECK_ARG(K <= MG_VQ_MAX_CODES, "mg_vq_bwd_f32: K=%d exceeds %d (MG_VQ_MAX_CODES)", K, MG_VQ_MAX_CODES);
    MG_CHECK_ARG(D <= MG_VQ_MAX_DIM, "mg_vq_bwd_f32: D=%d exceeds %d (MG_VQ_MAX_DIM)", D, MG_VQ_MAX_DIM);
    MG_CHECK_ARG(N <= MG_VQ_MAX_ROWS, "mg_vq_bwd_f32: N=%lld exceeds %lld (MG_VQ_MAX_ROWS)", (long long)N, (long long)MG_VQ_MAX_ROWS);
    MG_CHECK_ARG(ldz >= D, "mg_vq_bwd_f32: row stride %lld is below D=%d (negative and overlapping strides are refused)", (long long)ldz, D);
    MG_CHECK_ARG(((uintptr_t)g_lat & 3u) == 0 && ((uintptr_t)g_loss & 3u) == 0 && ((uintptr_t)z & 3u) == 0 && ((uintptr_t)quantised & 3u) == 0 &&
                     ((uintptr_t)dz & 3u) == 0 && ((uintptr_t)dE & 3u) == 0 && ((uintptr_t)index & 7u) == 0 && ((uintptr_t)n_valid & 7u) == 0,
                 "mg_vq_bwd_f32: float32 operands must be 4-byte, index and n_valid 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (dz) {
        hipLaunchKernelGGL(vq_dz_kernel, dim3((unsigned)mg_ceil_div(N * D, VQ_THREADS)), dim3(VQ_THREADS), 0, st, g_lat, g_loss, z, ldz, quantised,
                           index, n_valid, N, D, commitment_weight, dz);
        MG_CHECK_LAUNCH("mg_vq_bwd_f32/dz");
    }
    if (dE) {
        hipLaunchKernelGGL(vq_de_kernel, dim3((unsigned)K), dim3(VQ_THREADS), 0, st, g_loss, z, ldz, quantised, index, n_valid, N, D,
                           codebook_weight, dE);
        MG_CHECK_LAUNCH("mg_vq_bwd_f32/dE");
    }
    return MG_OK;
}

int mg_vq_ema_f32(const float* z, int64_t ldz, const int64_t* index, const int32_t* counts, int64_t N, int D, int K, double decay, double eps,
                  float* cluster_size, float* ema_sum, float* codebook, void* workspace, size_t workspace_bytes, void* stream) {
    MG_CHECK_ARG(z && index && counts && cluster_size && ema_sum && codebook,
                 "mg_vq_ema_f32: z, index, counts, cluster_size, ema_sum and codebook must not be NULL");
    MG_CHECK_ARG(N > 0 && D > 0 && K > 0, "mg_vq_ema_f32: bad shape (N=%lld D=%d K=%d)", (long long)N, D, K);
    MG_CHECK_ARG(K <= MG_VQ_MAX_CODES, "mg_vq_ema_f32: K=%d exceeds %d (MG_VQ_MAX_CODES)", K, MG_VQ_MAX_CODES);
    MG_CHECK_ARG(D <= MG_VQ_MAX_DIM, "mg_vq_ema_f32: D=%d exceeds %d (MG_VQ_MAX_DIM)", D, MG_VQ_MAX_DIM);
    MG_CHECK_ARG(N <= MG_VQ_MAX_ROWS, "mg_vq_ema_f32: N=%lld exceeds %lld (MG_VQ_MAX_ROWS)", (long long)N, (long long)MG_VQ_MAX_ROWS);
    MG_CHECK_ARG(ldz >= D, "mg_vq_ema_f32: row stride %lld is below D=%d (negative and overlapping strides are refused)", (long long)ldz, D);
    MG_CHECK_ARG(decay >= 0.0 && decay <= 1.0 && eps > 0.0, "mg_vq_ema_f32: decay=%g must be in [0, 1] and eps=%g positive", decay, eps);
    MG_CHECK_ARG(((uintptr_t)z & 3u) == 0 && ((uintptr_t)counts & 3u) == 0 && ((uintptr_t)cluster_size & 3u) == 0 && ((uintptr_t)ema_sum & 3u) == 0 &&
                     ((uintptr_t)codebook & 3u) == 0 && ((uintptr_t)index & 7u) == 0 && ((uintptr_t)workspace & 7u) == 0,
                 "mg_vq_ema_f32: float32 and int32 operands must be 4-byte, index and the workspace 8-byte aligned");
    if (!workspace || workspace_bytes < sizeof(double)) {
        mg_set_error("mg_vq_ema_f32: workspace of %zu bytes needed, got %zu", sizeof(double), workspace ? workspace_bytes : (size_t)0);
        return MG_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    double* total = (double*)workspace;
    hipLaunchKernelGGL(vq_ema_sizes_kernel, dim3(1), dim3(VQ_THREADS), 0, st, counts, K, decay, cluster_size, total);
    MG_CHECK_LAUNCH("mg_vq_ema_f32/sizes");
    hipLaunchKernelGGL(vq_ema_codes_kernel, dim3((unsigned)K), dim3(VQ_THREADS), 0, st, z, ldz, index, N, D, K, decay, eps,
                       (const float*)cluster_size, (const double*)total, ema_sum, codebook);
    MG_CHECK_LAUNCH("mg_vq_ema_f32/codes");
    return MG_OK;
}

}  // extern "C"
