#!/usr/bin/env python
"""Generate tests/golden/g17_sampling.npz by RUNNING THE REFERENCE'S ``sampling`` classes in fp32 on the CPU (build container only).

Usage (from the repo root, in the container that has the reference checkout ``make_golden.py`` imports):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sampling.py

Nothing of the reference's source is written anywhere: the .npz holds inputs, the noise the reference drew and the numbers it
computed.  The noise is re-drawn by re-seeding torch and asking the reference's own distributions again (``sampler.normal`` for the
sphere, ``sampler.sample_angles`` for the ellipsoid): same seed, same shapes, same stream.

Contents: ``cases`` (the case names) and per case ``<case>__centre`` (D,), ``<case>__noise`` (sample_shape + (D,) normal values for
a sphere, sample_shape + (D - 1,) angles for an ellipsoid), ``<case>__output`` (sample_shape + (D,)), all float32, and
``<case>__radius`` () for a sphere / ``<case>__radii`` (D,) for an ellipsoid.

  sphere_d{1,3,16}_s{0,1,2}     sample_shape (), (5,), (2, 3)
  ellipsoid_d{2,3,16}           sample_shape (5,) (the reference's sample_angles needs a list; its default sample_shape fails)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import import_reference  # noqa: E402


def main():
    import torch
    import_reference()
    from morgana import sampling
    torch.set_num_threads(1)
    rng = np.random.RandomState(20261017)
    out, names = {}, []
    seed = 1000
    for d in (1, 3, 16):
        for k, shape in enumerate(((), (5,), (2, 3))):
            seed += 1
            name = 'sphere_d%d_s%d' % (d, k)
            centre, radius = rng.standard_normal(d).astype(np.float32), np.float32(0.5 + rng.rand())
            sampler = sampling.UniformSphereSurfaceSampler(torch.from_numpy(centre.copy()), float(radius))
            torch.manual_seed(seed)
            points = sampler.rsample(shape)
            torch.manual_seed(seed)
            noise = sampler.normal.rsample(list(shape) + [d])
            assert tuple(points.shape) == shape + (d,)
            out[name + '__centre'], out[name + '__radius'] = centre, radius
            out[name + '__noise'], out[name + '__output'] = noise.numpy().astype(np.float32), points.numpy().astype(np.float32)
            names.append(name)
    for d in (2, 3, 16):
        seed += 1
        name = 'ellipsoid_d%d' % d
        centre, radii = rng.standard_normal(d).astype(np.float32), (0.5 + rng.rand(d)).astype(np.float32)
        sampler = sampling.UniformEllipsoidSurfaceApproximateSampler(torch.from_numpy(centre.copy()), torch.from_numpy(radii.copy()))
        torch.manual_seed(seed)
        points = sampler.rsample([5])
        torch.manual_seed(seed)
        angles = sampler.sample_angles([5])
        assert tuple(points.shape) == (5, d) and tuple(angles.shape) == (5, d - 1)
        out[name + '__centre'], out[name + '__radii'] = centre, radii
        out[name + '__noise'], out[name + '__output'] = angles.numpy().astype(np.float32), points.numpy().astype(np.float32)
        names.append(name)
    out['cases'] = np.array(names)
    for key, value in out.items():
        assert key == 'cases' or np.isfinite(value).all(), key
    path = os.path.join(HERE, 'g17_sampling.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes, %d arrays)' % (path, os.path.getsize(path), len(out)))


if __name__ == '__main__':
    main()
