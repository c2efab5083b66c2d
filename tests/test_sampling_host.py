"""CPU-only checks of ``morgana_amd.sampling`` (reference sampling.py): the float64 restatement the GPU tests hold the kernels to
(tests/sampling_ref64.py) reproduces what the reference computed from the same noise (tests/golden/g17_sampling.npz), the module and
its surface exist with the reference's names and signatures, CPU tensors raise, and the entry points of csrc/sampling.hip refuse bad
arguments on the host before any launch."""
import inspect
import os

import numpy as np
import pytest
import torch

import sampling_ref64 as ref
from morgana_amd import _lib, functional as F_hip, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g17_sampling.npz')


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)


def test_module_imports_and_mirrors_the_reference_surface():
    import morgana_amd
    from morgana_amd import sampling                            # fails without the feature
    assert morgana_amd.sampling is sampling
    sphere, ellipsoid = sampling.UniformSphereSurfaceSampler, sampling.UniformEllipsoidSurfaceApproximateSampler
    for cls in (sphere, ellipsoid):
        assert issubclass(cls, torch.distributions.Distribution) and cls.has_rsample
    assert list(inspect.signature(sphere.__init__).parameters) == ['self', 'centre', 'radius']
    assert list(inspect.signature(ellipsoid.__init__).parameters) == ['self', 'centre', 'radii']
    for cls in (sphere, ellipsoid):
        params = inspect.signature(cls.rsample).parameters
        assert list(params) == ['self', 'sample_shape'] and params['sample_shape'].default == torch.Size()
    assert list(inspect.signature(ellipsoid.sample_angles).parameters) == ['self', 'sample_shape']
    s = sphere(torch.zeros(3), 2.0)
    assert s.dim == 3 and s.radius == 2.0 and s.device == torch.device('cpu') and s.centre.shape == (3,)
    e = ellipsoid(torch.zeros(4), torch.ones(4))
    assert e.ndims == 4 and e.radii.shape == (4,)
    for name in ('sphere_sample', 'sphere_sample_backward', 'ellipsoid_sample', 'ellipsoid_sample_backward'):
        assert callable(getattr(ops, name)), name
    for name in ('SphereSampleFn', 'EllipsoidSampleFn'):
        assert issubclass(getattr(F_hip, name), torch.autograd.Function), name
    assert len({ops.SAMPLE_SITE, ops.SPHERE_SITE, ops.ELLIPSOID_SITE}) == 3


def test_restatement_equals_the_reference_on_its_own_noise():
    g = np.load(GOLDEN)
    cases = [str(c) for c in g['cases']]
    assert len(cases) == 12
    shapes = {0: (), 1: (5,), 2: (2, 3)}
    for case in cases:
        noise, want = g[case + '__noise'], g[case + '__output']
        d = g[case + '__centre'].shape[0]
        if case.startswith('sphere'):
            assert want.shape == shapes[int(case[-1])] + (d,) and noise.shape == want.shape
            got = ref.sphere(g[case + '__centre'], g[case + '__radius'], noise)['out']
        else:
            assert want.shape == (5, d) and noise.shape == (5, d - 1)
            got = ref.ellipsoid(g[case + '__radii'], noise)['out']
        assert got.shape == want.shape
        assert rel_err(got, want) < 1e-6, (case, rel_err(got, want))


def test_restatement_identities():
    """Properties of the construction the GPU tests lean on: unit rows, sum factor^2 = 1, D = 1 is +-1, the mapping's ranges."""
    rng = np.random.RandomState(3)
    s = ref.sphere(np.zeros(7), 1.0, rng.standard_normal((11, 7)))
    np.testing.assert_allclose(np.sqrt((s['unit'] ** 2).sum(-1)), 1.0, rtol=1e-14)
    assert np.array_equal(ref.sphere([0.25], 2.0, np.array([[-0.3], [4.0]]))['out'], [[-1.75], [2.25]])
    angles = rng.rand(9, 12) * np.pi
    angles[:, 0] *= 2
    e = ref.ellipsoid(np.full(13, 1.5), angles)
    np.testing.assert_allclose(np.sqrt((e['factor'] ** 2).sum(-1)), 1.0, rtol=1e-14)
    np.testing.assert_allclose(np.sqrt((e['out'] ** 2).sum(-1)), 1.5, rtol=1e-14)
    two = ref.ellipsoid([2.0, 3.0], [[0.5]])
    np.testing.assert_allclose(two['out'], [[2.0 * np.cos(0.5), 3.0 * np.sin(0.5)]], rtol=1e-15)
    assert ref.uniform(0) == 2.0 ** -24 and ref.uniform(0xFFFFFFFF) == 1.0 - 2.0 ** -24


def test_host_mapping_uses_the_library_block_function():
    """normal_noise / uniform_angles through mg_philox4x32_10 (host code, no GPU): flat blocks straddle the rows, the two mappings
    share their words, every value lies where the header says."""
    import ctypes
    lib = _lib.load()

    def philox(counter, key):
        c, k, out = (ctypes.c_uint32 * 4)(*counter), (ctypes.c_uint32 * 2)(*key), (ctypes.c_uint32 * 4)()
        lib.mg_philox4x32_10(c, k, out)
        return [int(v) for v in out]

    seed, ctr = 0x0123456789ABCDEF, 5 + (3 << 32)
    g = ref.normal_noise(5, 3, seed, ops.SPHERE_SITE, ctr, philox)
    assert g.shape == (5, 3) and np.isfinite(g).all() and (g != 0).all()
    flat = ref.normal_noise(1, 15, seed, ops.SPHERE_SITE, ctr, philox)
    assert np.array_equal(flat.reshape(5, 3), g)                                      # a function of the flat element alone
    a = ref.uniform_angles(4, 6, seed, ops.ELLIPSOID_SITE, ctr, philox)
    assert a.shape == (4, 5) and (a > 0).all() and (a[:, 0] < 2 * np.pi).all() and (a[:, 1:] < np.pi).all()
    w = ref.words(20, seed, ops.ELLIPSOID_SITE, ctr, philox)
    assert a[1, 0] == 2 * np.pi * ref.uniform(w[5]) and a[3, 4] == np.pi * ref.uniform(w[19])
    assert not np.array_equal(g, ref.normal_noise(5, 3, seed, ops.SAMPLE_SITE, ctr, philox))


def test_cpu_tensors_raise():
    from morgana_amd import sampling
    with pytest.raises(_lib.MorganaHipError):
        sampling.UniformSphereSurfaceSampler(torch.zeros(3), 1.0).rsample((2,))
    with pytest.raises(_lib.MorganaHipError):
        sampling.UniformSphereSurfaceSampler(torch.zeros(3), torch.ones(1)).sample()
    with pytest.raises(_lib.MorganaHipError):
        sampling.UniformEllipsoidSurfaceApproximateSampler(torch.zeros(3), torch.ones(3)).rsample((2,))
    with pytest.raises(_lib.MorganaHipError):
        sampling.UniformEllipsoidSurfaceApproximateSampler(torch.zeros(3), 2.0).sample_angles([2])
    used = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(_lib.MorganaHipError):
        ops.sphere_sample(torch.zeros(3), torch.ones(1), 2, 1, ops.SPHERE_SITE, used)
    with pytest.raises(_lib.MorganaHipError):
        ops.sphere_sample_backward(torch.zeros(2, 3), torch.zeros(2, 3))
    with pytest.raises(_lib.MorganaHipError):
        ops.ellipsoid_sample(torch.ones(3), 2, 1, ops.ELLIPSOID_SITE, used)
    with pytest.raises(_lib.MorganaHipError):
        ops.ellipsoid_sample_backward(torch.zeros(2, 3), torch.zeros(2, 3))


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    # sphere: null pointers, D < 1, rows < 0; no rows: no launch
    assert lib.mg_sphere_sample_f32(None, 16, 4, 3, 1, 0, None, 16, 16, None) == -1 and 'mg_sphere_sample_f32' in _lib.last_error()
    assert lib.mg_sphere_sample_f32(16, None, 4, 3, 1, 0, None, 16, 16, None) == -1
    assert lib.mg_sphere_sample_f32(16, 16, 4, 3, 1, 0, None, None, 16, None) == -1
    assert lib.mg_sphere_sample_f32(16, 16, 4, 3, 1, 0, None, 16, None, None) == -1
    assert lib.mg_sphere_sample_f32(16, 16, 4, 0, 1, 0, None, 16, 16, None) == -1 and 'D=0' in _lib.last_error()
    assert lib.mg_sphere_sample_f32(16, 16, -1, 3, 1, 0, None, 16, 16, None) == -1 and 'rows=-1' in _lib.last_error()
    assert lib.mg_sphere_sample_f32(16, 16, 0, 3, 1, 0, None, 16, 16, None) == 0
    assert lib.mg_sphere_sample_bwd_f32(None, 16, 4, 3, 16, 16, None) == -1 and 'mg_sphere_sample_bwd_f32' in _lib.last_error()
    assert lib.mg_sphere_sample_bwd_f32(16, 16, 4, 3, None, 16, None) == -1
    assert lib.mg_sphere_sample_bwd_f32(16, 16, 4, 3, 16, None, None) == -1
    assert lib.mg_sphere_sample_bwd_f32(16, 16, 4, 0, 16, 16, None) == -1
    assert lib.mg_sphere_sample_bwd_f32(16, 16, -2, 3, 16, 16, None) == -1 and 'rows=-2' in _lib.last_error()
    # ellipsoid: D < 2 has no well-formed output
    assert lib.mg_ellipsoid_sample_f32(None, 4, 3, 1, 0, None, 16, 16, None) == -1 and 'mg_ellipsoid_sample_f32' in _lib.last_error()
    assert lib.mg_ellipsoid_sample_f32(16, 4, 3, 1, 0, None, None, 16, None) == -1
    assert lib.mg_ellipsoid_sample_f32(16, 4, 3, 1, 0, None, 16, None, None) == -1
    assert lib.mg_ellipsoid_sample_f32(16, 4, 1, 1, 0, None, 16, 16, None) == -1 and 'D=1 must be >= 2' in _lib.last_error()
    assert lib.mg_ellipsoid_sample_f32(16, 4, 0, 1, 0, None, 16, 16, None) == -1
    assert lib.mg_ellipsoid_sample_f32(16, -1, 3, 1, 0, None, 16, 16, None) == -1 and 'rows=-1' in _lib.last_error()
    assert lib.mg_ellipsoid_sample_f32(16, 0, 3, 1, 0, None, 16, 16, None) == 0
    assert lib.mg_ellipsoid_angles_f32(4, 1, 1, 0, None, 16, None) == -1 and 'D=1' in _lib.last_error()
    assert lib.mg_ellipsoid_angles_f32(4, 3, 1, 0, None, None, None) == -1
    assert lib.mg_ellipsoid_angles_f32(-1, 3, 1, 0, None, 16, None) == -1
    assert lib.mg_ellipsoid_angles_f32(0, 3, 1, 0, None, 16, None) == 0
    assert lib.mg_ellipsoid_sample_bwd_f32(None, 16, 4, 3, 16, None) == -1 and 'mg_ellipsoid_sample_bwd_f32' in _lib.last_error()
    assert lib.mg_ellipsoid_sample_bwd_f32(16, None, 4, 3, 16, None) == -1
    assert lib.mg_ellipsoid_sample_bwd_f32(16, 16, 4, 3, None, None) == -1
    assert lib.mg_ellipsoid_sample_bwd_f32(16, 16, 4, 1, 16, None) == -1 and 'D=1' in _lib.last_error()
    assert lib.mg_ellipsoid_sample_bwd_f32(16, 16, -1, 3, 16, None) == -1
    with pytest.raises(ValueError):
        _lib.check(lib.mg_sphere_sample_f32(None, None, 4, 3, 1, 0, None, None, None, None), 'mg_sphere_sample_f32')
