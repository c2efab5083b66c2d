"""``morgana.sampling`` on the HIP path: latents drawn at a fixed distance from the prior's centre, the partner of
``BaseVAE.predict(features['latent'])`` for controlled, varied renditions of one utterance (reference sampling.py).

The noise is a stated function of (torch's seed, a site per sampler, the device's step counter, element), drawn from Philox4x32-10
inside the kernel (csrc/sampling.hip, mapping in include/morgana_hip.h): ``torch.manual_seed`` makes a run repeatable, every call
and every replay of a captured graph draws new noise, and a test can restate a draw on the host.  There is no CPU path.
"""
import torch
from torch.distributions import Distribution

from . import functional as F_hip
from . import ops


def _n_rows(sample_shape):
    rows = 1
    for s in sample_shape:
        rows *= int(s)
    return rows


class UniformSphereSurfaceSampler(Distribution):
    r"""Samples points uniformly on an n-dimensional sphere's surface: centre + radius * g / \|g\|, g ~ N(0, I).

    centre: (D,) float32 device tensor.  radius: a Python number - staged once, here, as a device scalar (nothing is copied to the
    device at a draw, so a draw can be captured into a graph); it gets no gradient - or a one-element float32 device tensor, which
    does, as ``centre`` does.

    Notes
    -----
    This is the same sampling procedure used by the von Mises-Fisher distribution for :math:`\kappa = 0`.
    """
    arg_constraints = {}
    has_rsample = True

    def __init__(self, centre, radius):
        self.device = centre.device

        self.centre = centre
        self.dim = len(self.centre)
        self.radius = radius
        self._radius = radius if isinstance(radius, torch.Tensor) else torch.tensor([float(radius)], dtype=torch.float32, device=self.device)

        super(UniformSphereSurfaceSampler, self).__init__(validate_args=False)

    def rsample(self, sample_shape=torch.Size()):
        r"""Samples points on the surface of the hypersphere: shape ``sample_shape + (D,)``."""
        sample_shape = tuple(sample_shape)
        ops._require(self.centre, torch.float32, 'centre')
        points = F_hip.SphereSampleFn.apply(self.centre, self._radius, _n_rows(sample_shape))
        return points.view(sample_shape + (self.dim,))


class UniformEllipsoidSurfaceApproximateSampler(Distribution):
    r"""Samples points ~uniformly on an n-dimensional ellipse's surface.

    centre: (..., D) tensor, D >= 2.  As in the reference it fixes the number of dimensions ONLY: ``rsample`` returns
    ``radii * cumprod_sin * cos_padded`` (reference sampling.py:113) - points around the ORIGIN - and so does this class; add the centre
    yourself if you mean it.  radii: (D,) float32 device tensor (differentiable), or a Python number staged once as D equal radii.

    Notes
    -----
    This is not a fair sampler, at the poles (especially for dimensions with large radii) samples will be denser.
    """
    arg_constraints = {}
    has_rsample = True

    def __init__(self, centre, radii):
        super(UniformEllipsoidSurfaceApproximateSampler, self).__init__(validate_args=False)

        self.centre = centre
        self.radii = radii

        self.ndims = centre.shape[-1]
        self._radii = radii if isinstance(radii, torch.Tensor) else torch.full((self.ndims,), float(radii), dtype=torch.float32,
                                                                               device=centre.device)

    def sample_angles(self, sample_shape):
        r"""Samples angles from n-1 uniform distributions: shape ``sample_shape + (n - 1,)``.

        One of these angles is in the range [0, 2*pi] and it determines tha angle in the first two dimensions.
        The remaining n-2 angles are in the range [0, pi] and determine the angle in the remaining dimensions.

        One draw of its own: the angles of the mapping ``rsample`` uses, not those of an earlier or later ``rsample`` call.
        """
        sample_shape = tuple(sample_shape)
        ops._require(self._radii, torch.float32, 'radii')
        seed, used = ops.dropout_seed(), ops.dropout_draw(self._radii.device)
        angles = ops.ellipsoid_angles(_n_rows(sample_shape), self.ndims, self._radii.device, seed, ops.ELLIPSOID_SITE, used)
        return angles.view(sample_shape + (self.ndims - 1,))

    def rsample(self, sample_shape=torch.Size()):
        r"""Computes the transformation for each cartesian dimension `n` (one fused kernel: angles, sines, running product),

        .. math::

            \mathtt{cumprod\_sin}_1 &= 1.

            \mathtt{cumprod\_sin}_n &= \prod_{i=1}^{n-1} \sin( \theta_i )

            \mathtt{cos}_n &= \cos( \theta_n ), \quad \mathtt{cos}_N = 1.

            x_n &= r_n * \mathtt{cumprod\_sin}_n * \mathtt{cos}_n

        Shape ``sample_shape + (D,)``.  The centre is not added (see the class docstring).
        """
        sample_shape = tuple(sample_shape)
        ops._require(self._radii, torch.float32, 'radii')
        radii = self._radii.expand(self.ndims) if self._radii.dim() == 0 else self._radii
        points = F_hip.EllipsoidSampleFn.apply(radii, _n_rows(sample_shape))
        return points.view(sample_shape + (self.ndims,))
