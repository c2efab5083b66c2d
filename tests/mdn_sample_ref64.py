"""Float64 restatement of the sampled mixture-density generation behind mg_mdn_sample_f32 (include/morgana_hip.h), GIVEN its Philox
words, with a DERIVED fp32 margin around every boundary of the component choice and derived fp32 bounds for the mean and the variance.

Plain numpy, no GPU and no torch.  The Philox block function is passed in (``philox(counter4, key2) -> 4 words``, the library's
host-only mg_philox4x32_10), and the word mapping, u(w) and the Box-Muller noise are tests/sampling_ref64.py's ``words``, ``uniform``
and ``normal_noise``, not restated here.  What is computed, per valid frame with row index r = b T + t (a row of K (1 + 2 D) columns =
K logits a, K D means mu, K D log standard deviations s, component-major; pad frames are not read and hold 0, 0 and 1):

    x_k  = (a_k - max_j a_j) inv_temperature,   w_k = exp(x_k)   (a -inf logit: exactly 0),   S = sum_k w_k,   p_k = w_k / S
    C_k  = (w_0 + ... + w_k) / S                                    the normalised CDF, C_{K-1} = 1
    u    = u(word r % 4 of Philox block r / 4) under the component site
    k*   = the lowest k with u < C_k  (none: the highest k with w_k > 0;  S NaN - every logit -inf: the lowest index among the
           largest logits, mg_mdn_select_f32's component)
    s'   = max(s_{k*,d}, floor),   variance_d = exp(2 s'),   mean_d = mu_{k*,d} + noise_scale exp(s') g_{r D + d}
    g    = the N(0, 1) value of flat element r D + d under the noise site (``normal_noise`` over the flat (B T, D) array)

inv_temperature is the fp32 value the entry point is handed (float32(1 / temperature)): it is an INPUT, not a rounding.

The margin delta.  The kernel decides  fl(u S~) < c~_k  on fp32 values; here U = 2^-24 is the unit roundoff, an elementary operation
returns its exact result times (1 + e), |e| <= U, expf is charged EXP_ULPS = 2 ulp (eps_e = 2 EXP_ULPS U relative; documented at 1),
products of error terms are dropped (first order), as in tests/sampling_ref64.py and tests/mdn_ref64.py.
  * the subtraction a_k - max a rounds once (the maximum itself is exact) and the product with inv_temperature once more: the
    computed x~_k = x_k (1 + 2 e), an ABSOLUTE error 2 U |x_k| in an exponent, i.e. relative in w;
  * expf:  w~_k = w_k (1 + e_k),  |e_k| <= 2 U |x_k| + eps_e.  A w below the normal range is rounded on the subnormal grid or
    flushed: ETA = 2^-149 ... 2^-126 absolute, charged as TINY = 2^-126 per term (S >= 1: it never matters, it is carried);
  * a sum of positive terms: a term that passes through j additions picks up at most j U relative, and in ANY order (a serial loop,
    a scan over lanes, a tree) a partial sum of at most K terms has j <= K - 1.  So, whatever the association,
        |c~_k - c_k| <= sum_{j <= k} w_j |e_j| + (K - 1) U c_k,     |S~ - S| likewise with k = K - 1;
  * the product u S~ rounds once (u is exact in fp32): fl(u S~) = u S~ (1 + e), |e| <= U.
Divide the kernel's test by the exact S > 0:  u (S~ / S)(1 + e) < c~_k / S.  With sigma = S~ / S - 1 and gamma_k = (c~_k - c_k) / S,
        |sigma|, |gamma_k| <= RHO := sum_j p_j (2 U |x_j| + eps_e) + (K - 1) U + K TINY = 2 U H + eps_e + (K - 1) U + K TINY,
H = sum_j p_j |x_j| (|x_j| = -log p_j - log S <= -log p_j since S >= 1, so H is at most the entropy, <= log K <= 4.16), and the
test reads  u (1 + sigma + e) < C_k + gamma_k.  Because u <= 1 it cannot differ from  u < C_k  unless

        |u - C_k| <= DELTA := 2 RHO + U = 2 (2 U H + eps_e + (K - 1) U + K TINY) + U            per frame, from its own H.

At K = 64 and the largest H that is (8.3 + 4 + 63) 2 U + U = 152 U = 9.0e-6; at K = 8, (4.2 + 4 + 7) 2 U + U = 31 U.  (A first
estimate that charges the sum once, (K + 8) U, is half of it: both S~ and c~_k carry the sum's error, in general not the same one.)
A frame is DECIDED when |u - C_k| > DELTA for every interior boundary k = 0 .. K - 2; then every fp32 evaluation of the rule picks
the float64 component.  On an undecided frame it picks a component whose interval [C_{k-1}, C_k] comes within DELTA of u and whose
weight is not 0: the two components next to the boundary (more only where a whole component is narrower than DELTA).  The
fallback "no k: the highest k with w_k > 0" needs u within DELTA of C_{K-1} = 1 and yields that last live component; it is inside
the same statement.  A -inf logit has w = 0 in every evaluation: c_k = c_{k-1} exactly, never the lowest k - never drawn.

Mean, noise_scale > 0, against the float64 value from the float64 noise: exp(s') carries eps_e (s' is exact), g carries RHO_G
(tests/sampling_ref64.py), the products noise_scale exp(s') and (that) g round once each, and the sum rounds once (as an fma the
second product does not round: the bound covers both forms); a result below the normal range adds ETA:
        bound_mean = |noise_scale exp(s') g| (eps_e + RHO_G + 2 U) + U |mean| + ETA
noise_scale == 0: the mean is an exact copy, the bound is 0.  Variance, exp(2 s') with 2 s' exact, or exp(s')^2: tests/mdn_ref64.py's
        bound_variance = variance (2 eps_e + 2 U) + ETA."""
import numpy as np

import mdn_ref64
import sampling_ref64

F64 = np.float64
U = 2.0 ** -24
ETA = 2.0 ** -149
TINY = 2.0 ** -126
EXP_ULPS = mdn_ref64.EXP_ULPS
EPS_E = 2 * EXP_ULPS * U
RHO_G = sampling_ref64.RHO_G
UNDECIDED_CAP = 0.01          # the share of undecided frames a test input may have


def inv_temperature(temperature):
    """What the entry point is handed: float32(1 / temperature), as a Python float."""
    return float(np.float32(1.0 / float(temperature)))


def component_uniforms(rows, seed, site, ctr, philox):
    """u (rows,) float64: frame r draws u(word r % 4 of Philox block r / 4)."""
    w = sampling_ref64.words(rows, seed, site, ctr, philox)
    return np.array([sampling_ref64.uniform(w[r]) for r in range(rows)], dtype=F64)


def weights(logits, temperature=1.0):
    """x, w, S, p (float64) of logits (..., K); a frame whose logits are all -inf (or hold an inf / a NaN) has S = NaN."""
    a = np.asarray(logits, dtype=F64)
    with np.errstate(all='ignore'):
        x = (a - a.max(axis=-1, keepdims=True)) * inv_temperature(temperature)
        w = np.exp(x)
        s = w.sum(axis=-1, keepdims=True)
        return x, w, s, w / s


def delta(p, x, k):
    """DELTA (...,) of the module docstring from p, x (..., K)."""
    with np.errstate(all='ignore'):
        h = np.where(p > 0, p * np.abs(np.where(p > 0, x, 0.0)), 0.0).sum(axis=-1)
    return 2 * (2 * U * h + EPS_E + (k - 1) * U + k * TINY) + U


def choose(logits, u, temperature=1.0):
    """The choice rule on logits (..., K) and uniforms (...,): dict with ``cdf`` (..., K), ``component``, ``decided``, ``delta`` and
    ``lowest`` / ``highest`` (...,) - the range of components an fp32 evaluation may return (both = component on a decided frame;
    inside it only components with a weight > 0 may be returned: ``live`` (..., K))."""
    a = np.asarray(logits, dtype=F64)
    u = np.asarray(u, dtype=F64)
    k = a.shape[-1]
    x, w, s, p = weights(a, temperature)
    broken = np.isnan(s[..., 0])
    with np.errstate(all='ignore'):
        cdf = np.cumsum(w, axis=-1) / s
    cdf[..., -1] = np.where(broken, np.nan, 1.0)
    live = w > 0
    last_live = (k - 1) - np.argmax(live[..., ::-1], axis=-1)
    below = u[..., None] < cdf
    component = np.where(below.any(axis=-1), np.argmax(below, axis=-1), last_live)
    component = np.where(broken, np.argmax(np.where(np.isnan(a), -np.inf, a), axis=-1), component).astype(np.int64)
    dl = delta(p, x, k)
    with np.errstate(all='ignore'):
        decided = (np.abs(u[..., None] - cdf[..., :k - 1]) > dl[..., None]).all(axis=-1) | broken
        # the components whose interval comes within DELTA of u: the lowest k with u - DELTA < C_k ... the lowest k with u + DELTA < C_k
        lo_mask = (u - dl)[..., None] < cdf
        hi_mask = (u + dl)[..., None] < cdf
    lowest = np.where(lo_mask.any(axis=-1), np.argmax(lo_mask, axis=-1), last_live)
    highest = np.where(hi_mask.any(axis=-1), np.argmax(hi_mask, axis=-1), last_live)
    lowest = np.where(broken, component, lowest)
    highest = np.where(broken, component, np.maximum(highest, lowest))
    return {'cdf': cdf, 'component': component, 'decided': decided, 'delta': dl, 'lowest': lowest, 'highest': highest, 'live': live,
            'probability': p, 'broken': broken}


def sample(pred, seq_len, n_components, dim, u, noise=None, min_log_std=None, temperature=1.0, noise_scale=0.0):
    """Float64 values and fp32 bounds.  pred (B, T, K (1 + 2 D)); ``u`` (B, T) the frames' uniforms; ``noise`` (B, T, D) the float64
    N(0, 1) values (needed when noise_scale > 0).  Returns ``choose``'s dict (pad frames: component 0, decided) plus ``mask`` (B, T),
    ``mean`` / ``mean_bound`` (0 on pad frames), ``variance`` / ``variance_bound`` (1 and 0 on pad frames) of the FLOAT64 component
    and ``moments(component)``: the same four for any other (B, T) choice of component (what an undecided frame is held to)."""
    x = np.asarray(pred, dtype=F64)
    b, t, _ = x.shape
    k, d = int(n_components), int(dim)
    n = mdn_ref64.valid_frames(seq_len, b, t)
    mask = np.arange(t)[None, :] < n[:, None]
    x = np.where(mask[:, :, None], x, 0.0)                 # pad frames are not read
    a, mu, s_raw = mdn_ref64.split(x, k, d)
    s = np.maximum(s_raw, min_log_std) if min_log_std is not None else s_raw
    out = choose(a, np.asarray(u, dtype=F64).reshape(b, t), temperature)
    for key in ('component', 'lowest', 'highest'):
        out[key] = np.where(mask, out[key], 0)
    out['decided'] = out['decided'] | ~mask
    out['mask'] = mask
    g = None if noise is None else np.asarray(noise, dtype=F64).reshape(b, t, d)
    if noise_scale != 0.0 and g is None:
        raise ValueError('sample: noise_scale=%r needs the noise' % (noise_scale,))

    def moments(component):
        pick = np.asarray(component, dtype=np.int64)[:, :, None, None]
        m = np.take_along_axis(mu, pick, axis=2)[:, :, 0, :]
        sd = np.take_along_axis(s, pick, axis=2)[:, :, 0, :]
        valid3 = mask[:, :, None]
        with np.errstate(all='ignore'):
            variance = np.where(valid3, np.exp(2.0 * sd), 1.0)
            variance_bound = np.where(valid3, variance * (2 * EPS_E + 2 * U) + ETA, 0.0)
            if noise_scale != 0.0:
                step = float(noise_scale) * np.exp(sd) * g
                mean = np.where(valid3, m + step, 0.0)
                mean_bound = np.where(valid3, np.abs(step) * (EPS_E + RHO_G + 2 * U) + U * np.abs(mean) + ETA, 0.0)
            else:
                mean = np.where(valid3, m, 0.0)
                mean_bound = np.zeros_like(mean)
        return mean, mean_bound, variance, variance_bound

    out['moments'] = moments
    out['mean'], out['mean_bound'], out['variance'], out['variance_bound'] = moments(out['component'])
    return out


def fp32_choice(logits, u, temperature=1.0):
    """The rule of include/morgana_hip.h evaluated in plain fp32 numpy (a serial prefix sum: np.cumsum): not the kernel, an honest
    fp32 evaluation that the margin must cover."""
    f = np.float32
    a = np.asarray(logits, dtype=f)
    k = a.shape[-1]
    with np.errstate(all='ignore'):
        w = np.exp(((a - a.max(axis=-1, keepdims=True)) * f(inv_temperature(temperature))).astype(f)).astype(f)
        c = np.cumsum(w, axis=-1, dtype=f)
        us = (np.asarray(u, dtype=f) * c[..., -1]).astype(f)
        below = us[..., None] < c
    last_live = (k - 1) - np.argmax((w > 0)[..., ::-1], axis=-1)
    component = np.where(below.any(axis=-1), np.argmax(below, axis=-1), last_live)
    broken = np.isnan(c[..., -1])
    return np.where(broken, np.argmax(np.where(np.isnan(a), -np.inf, a), axis=-1), component).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the inputs the tests share
SEED = 0x0123456789ABCDEF
CTR = 5 + (3 << 32)
TEMPERATURES = (0.5, 1.0, 2.0)
# (K, D) -> (B, T, seq_len): ragged, T no multiple of the kernel's 16 frames per workgroup.  K = 64: at least 2000 valid frames (one
# undecided frame among a few dozen would already be above the cap);  D = 1024: few frames - the float64 noise is drawn word by word;
# D = 64 | 65: the widest row whose noise the kernel draws one element per lane and the first it draws one Philox block per lane
# (csrc/mdn.hip: MDN_SAMPLE_ELEMENT_D), 65 = 1 mod 4 so that every row starts at another offset inside its first block
ELEMENT_D = 64
CASES = {(1, 1): (3, 37, (37, 20, 1)), (2, 1): (3, 37, (37, 20, 1)), (8, 3): (3, 37, (37, 20, 1)),
         (64, 3): (4, 637, (637, 600, 500, 301)), (4, 180): (3, 37, (37, 20, 1)), (16, 1024): (3, 7, (7, 4, 1)),
         (2, 64): (3, 21, (21, 9, 1)), (2, 65): (3, 21, (21, 9, 1))}
FREQ_FRAMES = (32, 512)        # 16384 frames that share one logit vector


def case(k, d, seed=20261021):
    """pred (B, T, K (1 + 2 D)) f32 and seq_len of CASES[(k, d)]: logits ~ N(0, 2^2), means ~ N(0, 1), log-stds ~ -0.5 + 0.5 N(0, 1)."""
    b, t, seq_len = CASES[(k, d)]
    rng = np.random.RandomState(seed + 100003 * k + d)
    logits = 2.0 * rng.standard_normal((b, t, k))
    means = rng.standard_normal((b, t, k * d))
    log_std = -0.5 + 0.5 * rng.standard_normal((b, t, k * d))
    return np.concatenate((logits, means, log_std), axis=2).astype(np.float32), np.array(seq_len, dtype=np.int64)


def frequency_case(k, seed=20261022):
    """One logit vector ~ N(0, 2^2) of K components in every one of the 16384 frames, D = 1 -> pred (32, 512, 3 K) f32, p (K,) float64."""
    b, t = FREQ_FRAMES
    rng = np.random.RandomState(seed + k)
    logits = (2.0 * rng.standard_normal(k)).astype(np.float32)
    row = np.concatenate((logits, np.arange(k, dtype=np.float32), np.zeros(k, dtype=np.float32)))
    return np.tile(row, (b, t, 1)), weights(logits)[3]


def frequency_bound(p, n):
    """|f_k - p_k| <= 5 sqrt(p_k (1 - p_k) / n) + 1 / n: five standard deviations of a binomial share, one frame of slack."""
    p = np.asarray(p, dtype=F64)
    return 5.0 * np.sqrt(p * (1.0 - p) / n) + 1.0 / n
