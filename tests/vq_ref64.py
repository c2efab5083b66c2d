"""NumPy float64 restatement of the vector-quantisation kernels (csrc/vq.hip: mg_vq_assign_f32, mg_vq_bwd_f32, mg_vq_ema_f32), the
decision margin of an assignment, and the inputs the GPU tests use (tests/test_gpu_vq.py) - tests/test_vq_host.py holds all of it
against torch's float64 autograd, finite differences and a hand-computed case, without a GPU.

The decision margin
-------------------
A distance is d = sum_{i < D} x_i^2 with x_i = z_i - e_i, evaluated in float64 (unit roundoff u = 2^-53):

* x_i is one rounded subtraction of two float32 values:            fl(x_i) = x_i (1 + a),            |a| <= u
* its square is one rounded product:                                fl(fl(x_i)^2) = x_i^2 (1 + a)^2 (1 + b),  |b| <= u
* D non-negative terms summed one after the other: term i passes through at most D - 1 rounded additions, each a factor
  (1 + c), |c| <= u.

So every term reaches the sum with a factor inside (1 +- u)^(D + 2), and as all terms are non-negative the evaluated distance is
d (1 + t) with |t| <= (D + 2) u + O(u^2): ANY float64 evaluation of the direct form - the reference's and the kernel's - is within
(D + 2) 2^-53 d of the true distance.  The order of two codes with true distances d1 < d2 can differ between two such evaluations
only if d2 - d1 <= 2 (D + 2) 2^-53 (d1 + d2) = (D + 2) 2^-52 (d1 + d2) (each of the two evaluations may move each of the two
distances by its bound).  MARGIN_FACTOR = 2 on top of that covers the O(u^2) terms and the use of the evaluated distances in place
of the true ones: a row is DECIDED when its best and second-best evaluated distances differ by more than
2 (D + 2) 2^-52 (d1 + d2).  On a decided row every float64 evaluation agrees on the code; on any other row only the distance is
compared.  (An exact tie between bit-identical codes is never "decided" by this rule and needs none: identical operands give
identical distances in every evaluation, and the rule "lowest index" then fixes the code - the tie tests assert the index itself.)
"""
import numpy as np

U32 = 2.0 ** -24            # unit roundoff of float32: one rounding of a result r moves it by at most U32 |r|
U64 = 2.0 ** -53
MARGIN_FACTOR = 2.0
EMA_EPS = 1e-5


def valid_rows(shape, seq_len):
    """(N,) bool: which rows of a (N, D) / (B, S, D) input count (all of them without seq_len)."""
    n = int(np.prod(shape[:-1]))
    if seq_len is None:
        return np.ones(n, dtype=bool)
    b, s = shape[0], shape[1]
    lens = np.clip(np.asarray(seq_len, dtype=np.int64), 0, s)
    return (np.arange(s)[None, :] < lens[:, None]).reshape(-1)


def distances(z, codebook):
    """(N, K) float64: d[n, k] = sum_d (z[n, d] - E[k, d])^2, the direct difference, summed in ascending d."""
    z = np.asarray(z, dtype=np.float64)
    e = np.asarray(codebook, dtype=np.float64)
    acc = np.zeros((z.shape[0], e.shape[0]))
    with np.errstate(invalid='ignore', over='ignore'):
        for d in range(z.shape[1]):
            diff = z[:, d, None] - e[None, :, d]
            acc = acc + diff * diff
    return acc


def assign(z, codebook, seq_len=None):
    """The assignment of mg_vq_assign_f32 -> dict(index (N,) int64 with -1 on pad rows, quantised (N, D) float32, best (N,) float64 the
    winner's distance, vq, perplexity (float64 scalars), counts (K,) int64, n_valid, decided (N,) bool).  z: (N, D) or (B, S, D)."""
    z = np.asarray(z)
    codebook = np.asarray(codebook, dtype=np.float32)
    dim, k = z.shape[-1], codebook.shape[0]
    valid = valid_rows(z.shape, seq_len)
    rows = np.where(valid[:, None], z.reshape(-1, dim), 0.0)              # pad rows are never looked at
    d = distances(rows, codebook)
    ranked = np.where(np.isnan(d), np.inf, d)                             # a NaN distance never wins ...
    index = np.argmin(ranked, axis=1).astype(np.int64)                    # ... and argmin takes the lowest index of equal minima
    best = d[np.arange(d.shape[0]), index]
    all_nan = np.isnan(d).all(axis=1)                                     # every distance NaN: code 0 (argmin of all-inf) and a NaN loss
    best = np.where(all_nan, np.nan, np.where(np.isnan(best), np.inf, best))
    if k > 1:
        second = np.partition(ranked, 1, axis=1)[:, 1]
        with np.errstate(invalid='ignore'):
            decided = second - ranked.min(axis=1) > MARGIN_FACTOR * (dim + 2) * 2.0 ** -52 * (second + ranked.min(axis=1))
    else:
        decided = np.ones(d.shape[0], dtype=bool)
    index = np.where(valid, index, -1)
    best = np.where(valid, best, 0.0)
    quantised = np.where(valid[:, None], codebook[np.maximum(index, 0)], np.float32(0)).astype(np.float32)
    n_valid = int(valid.sum())
    counts = np.bincount(index[valid], minlength=k).astype(np.int64)
    with np.errstate(invalid='ignore', divide='ignore'):
        vq = np.float64(best.sum()) / (np.float64(n_valid) * dim)
        p = counts[counts > 0] / np.float64(n_valid)
        perplexity = np.exp(-(p * np.log(p)).sum()) if n_valid > 0 else np.nan
    return dict(index=index, quantised=quantised, best=best, vq=vq, perplexity=perplexity, counts=counts, n_valid=n_valid,
                decided=decided | ~valid)


def backward(z, quantised, index, n_valid, grad_latent, grad_loss, codebook_weight, commitment_weight, n_codes):
    """(dz (N, D), dE (K, D), members (K,)) in float64: dz = g_lat + g beta 2 (z - q) / (N_valid D), zero on pad rows;
    dE[k] = g cw 2 sum_{index == k} (q - z) / (N_valid D), the members in ascending n."""
    dim = np.asarray(z).shape[-1]
    z = np.asarray(z, dtype=np.float64).reshape(-1, dim)
    q = np.asarray(quantised, dtype=np.float64).reshape(-1, dim)
    index = np.asarray(index).reshape(-1)
    valid = index >= 0
    scale = np.float64(grad_loss) * 2.0 / (np.float64(n_valid) * dim)
    up = np.zeros_like(z) if grad_latent is None else np.asarray(grad_latent, dtype=np.float64).reshape(-1, dim)
    dz = np.where(valid[:, None], up + scale * commitment_weight * (np.where(valid[:, None], z, 0.0) - q), 0.0)
    de = np.zeros((n_codes, dim))
    members = np.zeros(n_codes, dtype=np.int64)
    for n in np.nonzero(valid)[0]:                                         # ascending n
        de[index[n]] += q[n] - z[n]
        members[index[n]] += 1
    return dz, np.where(members[:, None] > 0, scale * codebook_weight * de, 0.0), members


def loss_value(z, codebook, index, n_valid, codebook_weight, commitment_weight):
    """The loss as a function of z and the codebook with the ASSIGNMENTS HELD FIXED (what the finite differences perturb):
    codebook_weight and commitment_weight each times sum_n |z[n] - E[index[n]]|^2 / (N_valid D) -> the two parts."""
    z = np.asarray(z, dtype=np.float64)
    e = np.asarray(codebook, dtype=np.float64)
    valid = index >= 0
    mse = ((z[valid] - e[index[valid]]) ** 2).sum() / (np.float64(n_valid) * z.shape[1])
    return codebook_weight * mse, commitment_weight * mse


def ema_update(z, index, counts, cluster_size, ema_sum, decay, eps=EMA_EPS):
    """One mg_vq_ema_f32 step on float32 states -> (cluster_size, ema_sum, codebook) in float64, BEFORE their rounding to float32
    (the kernel's total is the sum of the ROUNDED new sizes, and so is this one's)."""
    dim = np.asarray(z).shape[-1]
    z = np.asarray(z, dtype=np.float64).reshape(-1, dim)
    index = np.asarray(index).reshape(-1)
    k = len(counts)
    size = decay * np.asarray(cluster_size, dtype=np.float64) + (1.0 - decay) * np.asarray(counts, dtype=np.float64)
    stored = size.astype(np.float32).astype(np.float64)
    total = stored.sum()
    sums = np.zeros((k, dim))
    for n in np.nonzero(index >= 0)[0]:
        sums[index[n]] += z[n]
    m = decay * np.asarray(ema_sum, dtype=np.float64) + (1.0 - decay) * sums
    smoothed = (stored + eps) / (total + k * eps) * total
    return size, m, m / smoothed[:, None]


# ------------------------------------------------------------------------------------------- the inputs of the GPU tests
ASSIGN_N = (1, 5, 64, 257)
ASSIGN_K = (1, 2, 63, 64, 65, 512)
ASSIGN_D = (1, 3, 16, 17, 64)
TILE_FLOATS = 8192          # csrc/vq.hip: one LDS tile holds floor(8192 / (D | 1)) codes (mg_vq_tile_codes(D) says the same)


def tile_codes(dim):
    return TILE_FLOATS // (dim | 1)


def case(n, k, dim, seed=0):
    """(z (n, dim), codebook (k, dim)) float32: codes ~ N(0, 1), rows = a code + N(0, 0.3^2) - clustered, as an encoder's output is."""
    rng = np.random.RandomState((seed * 1000003 + n * 7919 + k * 104729 + dim) % (2 ** 32))
    codebook = rng.standard_normal((k, dim)).astype(np.float32)
    z = (codebook[rng.randint(0, k, size=n)] + 0.3 * rng.standard_normal((n, dim))).astype(np.float32)
    return z, codebook


def assign_cases():
    """Every (n, k, dim) the assignment test runs: the issue's grid, plus for each dim the first K past the LDS tile boundary."""
    for dim in ASSIGN_D:
        for k in ASSIGN_K + (tile_codes(dim) + 1,):
            for n in ASSIGN_N:
                yield n, k, dim
