"""Float64 numpy restatement of global gradient-norm clipping (torch.nn.utils.clip_grad_norm_(params, c, norm_type=2,
error_if_nonfinite=False)), the reference of tests/test_clip_host.py and tests/test_gpu_clip.py.

    norm64(g)  = sqrt(sum(float64(g)^2))                    over every element of every buffer
    coef       = min(1, c / (norm * inv_world + 1e-6))

with torch's behaviour at the edges written out: a NaN norm gives a NaN coefficient (torch.clamp(nan, max=1) is nan - the
gradients become NaN), an infinite norm gives 0, a zero norm gives min(1, c / 1e-6).  No exception in either case."""
import math

import numpy as np


def norm64(*buffers):
    """2-norm over all elements of all ``buffers``, every square and the sum in float64 (the square of a float32 is exact there)."""
    total = 0.0
    for g in buffers:
        g64 = np.asarray(g, dtype=np.float64).reshape(-1)
        with np.errstate(over='ignore', invalid='ignore'):
            total = total + float(np.sum(g64 * g64))
    return math.sqrt(total) if not math.isnan(total) else float('nan')


def coef(norm, max_norm, inv_world=1.0):
    """The clipping coefficient for the norm of the SUM over ranks ``norm`` (the mean's norm is norm * inv_world)."""
    norm = float(norm) * float(inv_world)
    if math.isnan(norm):
        return float('nan')
    if math.isinf(norm):
        return 0.0
    return min(1.0, float(max_norm) / (norm + 1e-6))


def clip(buffers, max_norm, inv_world=1.0):
    """(norm of the mean gradient, coefficient, [float64 clipped buffers]) - the buffers keep the scale they came in (a sum over ranks
    stays a sum)."""
    n = norm64(*buffers)
    c = coef(n, max_norm, inv_world)
    with np.errstate(invalid='ignore'):
        return n * inv_world, c, [np.asarray(g, dtype=np.float64) * c for g in buffers]
