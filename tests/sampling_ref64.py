"""Float64 restatement of the two latent surface samplers (morgana_amd.sampling, reference sampling.py) GIVEN their noise, of their
gradients, and of the Philox mapping include/morgana_hip.h documents for them - with DERIVED fp32 rounding bounds.

Plain numpy, no GPU and no torch.  What is computed:

    sphere      g (rows, D) ~ N(0, 1) given;   unit = g / |g|_2 (per row);   out = centre + radius * unit
                dcentre[c] = sum_r dout[r, c];   dradius = sum_{r, c} dout[r, c] unit[r, c]
    ellipsoid   angles (rows, D - 1) given (column 0 in [0, 2 pi], the others in [0, pi]);
                factor[r, n] = prod_{j < n} sin(angle[r, j]) * cos(angle[r, n]),  empty product = 1,  cos(angle[r, D - 1]) := 1;
                out = radii * factor (the reference's `centre` is NOT added, sampling.py:113);   dradii[n] = sum_r dout[r, n] factor[r, n]

The bounds are properties of fp32 arithmetic and of the documented accuracy of the device's math functions, not of any kernel.
U = 2^-24 is the unit roundoff: an elementary operation returns its exact result times (1 + d), |d| <= U; a function documented at
k units in the last place is good to 2 k U RELATIVE (an ulp of x is at most 2 U |x|); products of error terms are dropped (first
order).  logf, sinpif / cospif / sincospif are documented at 1 ulp in the HIP math API's accuracy table, sqrtf and the division
are correctly rounded in hipcc's default mode; 2 ulp are charged for the first group (LOG_ULPS, TRIG_ULPS), 1 ulp for sqrtf (SQRT_ULPS).

Noise (the Box-Muller value g = R t, R = sqrt(-2 ln u(a)), t = cos or sin of 2 pi u(b)): u is exact in fp32 (an odd multiple of
2^-24), 2 u(b) is exact and the pi-scaled functions take it as it is - no rounded multiple of pi is formed, so the argument carries no
error and the value's error is relative even next to a zero of the function.  ln u: 2 LOG_ULPS U;  times -2: exact;  the square root
halves it and adds 2 SQRT_ULPS U;  t: 2 TRIG_ULPS U;  the product: U.

    RHO_G = LOG_ULPS U + 2 SQRT_ULPS U + 2 TRIG_ULPS U + U            (9 U)

Sphere, against the float64 value computed from the float64 noise.  s = sum_c g_c^2: a square carries 2 RHO_G + U; all terms are
positive, so a term that passes through k additions picks up at most k U relative, and a sum of D terms in ANY order (serial, a
tree over lanes, chunks with a carried partial sum) has k <= D - 1: a gamma_D-style bound, D U with the square's own rounding.  The
square root halves that and adds 2 SQRT_ULPS U;  unit = g / norm adds RHO_G of its numerator and U of the division:

    RHO_UNIT(D) = 2 RHO_G + D U / 2 + 2 SQRT_ULPS U + U                bound_unit = |unit| RHO_UNIT
    bound_out   = |radius unit| (RHO_UNIT + U) + U |out|               (the product, then the sum; an fma only drops a term)

Invariants of the kernel's OWN output (no restated noise: g is then exact and RHO_G drops out): with RHO_OWN(D) = D U / 2 +
2 SQRT_ULPS U + U,   | |unit|_2 - 1 | <= RHO_OWN   and   | |out - centre|_2 - |radius| | <= |radius| (RHO_OWN + U) + U |out|_2.
For D = 1, g / sqrt(g^2) is exactly +-1 (sqrt(fl(x^2)) = |x| in binary floating point) and out is the fp32 sum centre +- radius.

Ellipsoid, against the float64 value from the float64 angles pi u (2 pi u in column 0): TAU = 2 TRIG_ULPS U per sine or cosine (no
argument error, as above).  A product of n sines, however it is associated (a serial loop, a scan over lanes, a carried prefix
between chunks) is formed by n - 1 multiplications, each in exactly one factor's path to the result: n TAU + (n - 1) U.  Times the
cosine: TAU + U.  Times the radius: U.

A long product of sines leaves the normal range (D = 130: 129 factors below 1): a product below TINY = 2^-126 is rounded on the
subnormal grid (2^-150 absolute) or flushed to zero (below TINY absolute), whichever the denormal mode says; the larger is
charged, per multiplication, and passes through the later factors (all <= 1 in magnitude) and the radius unchanged or smaller:

    bound_factor[n] = |factor[n]| (n + 1) (TAU + U) + (n + 1) TINY
    bound_out[n]    = |out[n]| ((n + 1) (TAU + U) + U) + (|radii[n]| (n + 1) + 1) TINY

sum_n factor[n]^2 = 1 is an identity of the construction (cos^2 + sin^2 = 1, folded from the last column down), so for the
kernel's own output | |factor|_2 - 1 | <= D (TAU + U) + D^2 TINY, and with all radii = r: | |out|_2 - r | <= r times that, + U r.

Gradients: fp64 partial sums of fp32 inputs, rounded to fp32 once.  The float64 reference uses the restated unit / factor, the
kernel its own fp32 copy, so the inputs' bounds enter weighted by |dout|; n terms summed in fp64 add n 2^-53 sum |terms|:

    bound_dcentre = U |dcentre| + rows 2^-53 sum_r |dout|
    bound_dradius = sum |dout| bound_unit   + U |dradius| + rows D 2^-53 sum |dout unit|
    bound_dradii  = sum_r |dout| bound_factor + U |dradii| + rows 2^-53 sum_r |dout factor|
"""
import numpy as np

F64 = np.float64
U = 2.0 ** -24
LOG_ULPS = 2.0
TRIG_ULPS = 2.0
SQRT_ULPS = 1.0
RHO_G = LOG_ULPS * U + 2 * SQRT_ULPS * U + 2 * TRIG_ULPS * U + U
TAU = 2 * TRIG_ULPS * U
TINY = 2.0 ** -126


# ------------------------------------------------------------------------------------------------------------ the Philox mapping
def uniform(word):
    """u(w) = ((w >> 8) | 1) 2^-24: inside (0, 1), exact in fp32."""
    return float((int(word) >> 8) | 1) * 2.0 ** -24


def words(n, seed, site, ctr, philox):
    """The Philox words of flat elements 0..n-1: element i is word i % 4 of block i / 4 with counter words (q low, q high, ctr low,
    site ^ ctr high) and key (seed low, seed high).  ``philox(counter4, key2) -> 4 words`` is the block function (mg_philox4x32_10)."""
    out = []
    for q in range((n + 3) // 4):
        out.extend(philox([q & 0xFFFFFFFF, q >> 32, ctr & 0xFFFFFFFF, (site ^ (ctr >> 32)) & 0xFFFFFFFF], [seed & 0xFFFFFFFF, seed >> 32]))
    return out


def normal_noise(rows, d, seed, site, ctr, philox):
    """g (rows, d) float64: a block's words (x, y, z, w) give elements 4q..4q+3 = R(x) cos(2 pi u(y)), R(x) sin(2 pi u(y)),
    R(z) cos(2 pi u(w)), R(z) sin(2 pi u(w)), R(a) = sqrt(-2 ln u(a)).  Blocks run over the FLAT array: they straddle rows."""
    n = rows * d
    w = words(n, seed, site, ctr, philox)
    g = np.empty(4 * ((n + 3) // 4), dtype=F64)
    for q in range((n + 3) // 4):
        x, y, z, v = w[4 * q:4 * q + 4]
        r0, r1 = np.sqrt(-2.0 * np.log(uniform(x))), np.sqrt(-2.0 * np.log(uniform(z)))
        a0, a1 = 2.0 * np.pi * uniform(y), 2.0 * np.pi * uniform(v)
        g[4 * q:4 * q + 4] = (r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1))
    return g[:n].reshape(rows, d)


def uniform_angles(rows, d, seed, site, ctr, philox):
    """angles (rows, d - 1) float64: element i = r (d - 1) + c draws u(word i % 4 of block i / 4); column 0 is 2 pi u, the others pi u."""
    a = d - 1
    w = words(rows * a, seed, site, ctr, philox)
    u = np.array([uniform(w[i]) for i in range(rows * a)], dtype=F64).reshape(rows, a)
    scale = np.full(a, np.pi)
    scale[0] = 2.0 * np.pi
    return u * scale


# ----------------------------------------------------------------------------------------------------------------------- sphere
def rho_unit(d):
    return 2 * RHO_G + d * U / 2 + 2 * SQRT_ULPS * U + U


def rho_own(d):
    return d * U / 2 + 2 * SQRT_ULPS * U + U


def sphere(centre, radius, noise):
    """Float64 values and fp32 bounds from noise (..., D): dict with ``unit`` / ``unit_bound`` and ``out`` / ``out_bound``."""
    g = np.asarray(noise, dtype=F64)
    centre, radius = np.asarray(centre, dtype=F64), float(radius)
    d = g.shape[-1]
    unit = g / np.sqrt((g * g).sum(axis=-1, keepdims=True))
    out = centre + radius * unit
    unit_bound = np.abs(unit) * rho_unit(d)
    out_bound = np.abs(radius * unit) * (rho_unit(d) + U) + U * np.abs(out)
    return {'unit': unit, 'unit_bound': unit_bound, 'out': out, 'out_bound': out_bound}


def sphere_radius_bound(out, radius):
    """Bound of | |out - centre|_2 - |radius| | per row, for the kernel's own rows ``out`` (rows, D)."""
    out = np.asarray(out, dtype=F64)
    return abs(float(radius)) * (rho_own(out.shape[-1]) + U) + U * np.sqrt((out * out).sum(axis=-1))


def sphere_grads(dout, unit, unit_bound):
    """Float64 (dcentre, dradius) and their bounds from dout, unit (rows, D)."""
    dout, unit = np.asarray(dout, dtype=F64), np.asarray(unit, dtype=F64)
    rows, d = dout.shape
    dcentre = dout.sum(axis=0)
    dradius = (dout * unit).sum()
    dcentre_bound = U * np.abs(dcentre) + rows * 2.0 ** -53 * np.abs(dout).sum(axis=0)
    dradius_bound = (np.abs(dout) * unit_bound).sum() + U * abs(dradius) + rows * d * 2.0 ** -53 * np.abs(dout * unit).sum()
    return {'dcentre': dcentre, 'dcentre_bound': dcentre_bound, 'dradius': dradius, 'dradius_bound': dradius_bound}


# -------------------------------------------------------------------------------------------------------------------- ellipsoid
def ellipsoid(radii, angles):
    """Float64 values and fp32 bounds from angles (..., D - 1): dict with ``factor`` / ``factor_bound`` and ``out`` / ``out_bound``."""
    angles = np.asarray(angles, dtype=F64)
    radii = np.asarray(radii, dtype=F64)
    pad = np.ones(angles.shape[:-1] + (1,), dtype=F64)
    cumprod_sin = np.concatenate((pad, np.cumprod(np.sin(angles), axis=-1)), axis=-1)
    cos_padded = np.concatenate((np.cos(angles), pad), axis=-1)
    factor = cumprod_sin * cos_padded
    out = radii * factor
    n = np.arange(factor.shape[-1], dtype=F64)
    factor_bound = np.abs(factor) * (n + 1) * (TAU + U) + (n + 1) * TINY
    out_bound = np.abs(out) * ((n + 1) * (TAU + U) + U) + (np.abs(radii) * (n + 1) + 1) * TINY
    return {'factor': factor, 'factor_bound': factor_bound, 'out': out, 'out_bound': out_bound}


def ellipsoid_norm_rho(d):
    """Relative bound of | |factor|_2 - 1 | for a kernel's own factor row (add U for out with equal radii)."""
    return d * (TAU + U) + d * d * TINY


def ellipsoid_grads(dout, factor, factor_bound):
    dout, factor = np.asarray(dout, dtype=F64), np.asarray(factor, dtype=F64)
    rows = dout.shape[0]
    dradii = (dout * factor).sum(axis=0)
    bound = (np.abs(dout) * factor_bound).sum(axis=0) + U * np.abs(dradii) + rows * 2.0 ** -53 * np.abs(dout * factor).sum(axis=0)
    return {'dradii': dradii, 'dradii_bound': bound}
