"""The float64 restatement of generation under a global-variance prior (tests/mlpg_gv_ref64.py) held to the problem it restates, on
the CPU: its root is a stationary point of F, no worse than the descent HTS runs, its variance lies between MLPG's and the prior's
mean, the fallbacks fall back - and the inertia rule and the rank-one update the kernel evaluates with agree with a dense solve."""
import numpy as np
import pytest

import mlpg_gv_ref64 as ref

CASES = [(length, padding, factor) for length, padding in ((2, 0), (2, 3), (5, 3), (11, 0), (24, 3), (60, 10)) for factor in (0.5, 2.0, 8.0)]


def _system(length, padding, factor, windows='default', weight=1.0, seed=0):
    rng = np.random.RandomState(100 * length + 10 * padding + seed)
    wins = ref.WINDOWS[windows]
    width = len(wins)
    means = rng.standard_normal((1, length, width)).astype(np.float32)
    variances = ref.make_variances(rng, 'frame', 1, length, width)
    p_mat, rhs = ref.build_system(means, variances, wins, padding, length, 0, 0)
    v0 = ref.variance_over(np.linalg.solve(p_mat, rhs), padding, length)
    mu_v = factor * v0
    return ref.System(p_mat, rhs, padding, length, len(wins), mu_v, (0.1 * mu_v) ** 2, weight)


@pytest.mark.parametrize('length,padding,factor', CASES)
def test_the_root_is_a_stationary_point_between_mlpg_and_the_prior(length, padding, factor):
    system = _system(length, padding, factor)
    x, kappa, h_abs, used, flag = system.solve()
    assert flag == 0 and h_abs <= ref.H_RULE * (1 + abs(kappa))
    assert (np.linalg.eigvalsh(system.matrix(kappa)) > 0).all()
    at_root, at_start = np.abs(system.gradient(x)).max(), np.abs(system.gradient(system.x0)).max()
    print('n=%d padding=%d factor=%g: kappa %.6g after %d evaluations, |grad F| %.3e at the root, %.3e at x0' % (
        length, padding, factor, kappa, used, at_root, at_start))
    assert at_root <= ref.GRAD_RATIO * at_start
    v0, v = system.variance(system.x0), system.variance(x)
    assert min(v0, system.mu_v) <= v <= max(v0, system.mu_v)
    assert system.objective(x) <= system.objective(system.x0)


@pytest.mark.parametrize('length,padding,factor', [(5, 3, 0.5), (24, 3, 2.0), (60, 10, 0.5), (60, 10, 2.0)])
def test_the_root_is_no_worse_than_500_preconditioned_gradient_steps(length, padding, factor):
    system = _system(length, padding, factor)
    x, _, _, _, flag = system.solve()
    _, descended = system.descend(500)
    print('F at the root %.12g, after 500 steps %.12g, at x0 %.12g' % (system.objective(x), descended, system.objective(system.x0)))
    assert flag == 0 and system.objective(x) <= descended


def test_fallbacks_return_the_mlpg_solution():
    one_frame = _system(1, 3, 2.0)
    x, kappa, _, used, flag = one_frame.solve()
    assert flag == 1 and used == 0 and kappa == 0.0 and np.array_equal(x, one_frame.x0)
    no_weight = _system(24, 3, 2.0, weight=0.0)
    x, kappa, _, used, flag = no_weight.solve()
    assert flag == 1 and used == 0 and np.array_equal(x, no_weight.x0)
    # all-zero means: x = 0 and v = 0 whatever kappa, h has no root where A is positive definite - the degenerate fallback
    system = _system(24, 3, 2.0)
    flat = ref.System(system.p_mat, np.zeros_like(system.rhs), 3, 24, 3, system.mu_v, system.sigma2_v)
    x, kappa, h_abs, used, flag = flat.solve()
    assert flag == 1 and h_abs > ref.H_RULE * (1 + abs(kappa)) and not x.any()


@pytest.mark.parametrize('length,padding,factor', CASES)
def test_inertia_rule_and_rank_one_update_equal_the_dense_solve(length, padding, factor):
    """What the kernel evaluates with: B = P + gamma E by unpivoted LDL^T, y = B^-1 rhs, z = B^-1 e, x = y - c (e'y) / (1 + c e'z) z,
    and A positive definite iff (no pivot <= 0 and 1 + c e'z > 0) or (one pivot < 0 and 1 + c e'z < 0) - at the root and around it."""
    system = _system(length, padding, factor)
    _, root, _, _, _ = system.solve()
    lo, _ = system.bracket()
    for kappa in (root, 0.5 * root, 0.9 * lo, 1.1 * lo, 2.0 * abs(root) + 1.0):
        gamma = 2.0 * kappa / (system.length * system.omega)
        b_mat, c = system.p_mat + gamma * np.diag(system.e), -gamma / system.length
        n = len(system.rhs)
        low, diag = np.eye(n), np.zeros(n)
        for i in range(n):                                    # unpivoted LDL^T
            for j in range(i):
                low[i, j] = (b_mat[i, j] - (low[i, :j] * low[j, :j]) @ diag[:j]) / diag[j]
            diag[i] = b_mat[i, i] - (low[i, :i] ** 2) @ diag[:i]
        if (diag == 0).any():
            continue
        y = np.linalg.solve(low.T, np.linalg.solve(low, system.rhs) / diag)
        z = np.linalg.solve(low.T, np.linalg.solve(low, system.e) / diag)
        s = 1.0 + c * (system.e @ z)
        by_inertia = bool(((diag > 0).all() and s > 0) or ((diag < 0).sum() == 1 and s < 0))
        by_spectrum = bool((np.linalg.eigvalsh(system.matrix(kappa)) > 0).all())
        assert by_inertia == by_spectrum, (kappa, diag.min(), s)
        if by_spectrum:
            x = y - c * (system.e @ y) / s * z
            want = np.linalg.solve(system.matrix(kappa), system.rhs)
            assert np.abs(x - want).max() <= 1e-10 * np.abs(want).max()


def test_gpu_cases_flag_exactly_the_one_frame_and_the_degenerate_item():
    for key in ref.CASE_KEYS[:2] + ref.CASE_KEYS[-2:]:
        info = ref.case(*key)[8]
        flagged = {b for b in range(ref.BSZ) if info[b, :, 3].any()}
        assert flagged == {4, ref.DEGENERATE}, (key, flagged)
        assert all(info[b, :, 3].all() for b in flagged)


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    """mg_mlpg_gv_f32's host side: mg_mlpg_f32's checks plus gv_weight and max_iter, each before any launch (fake addresses never
    reach the device), and a workspace of two sets of MLPG's planes."""
    import ctypes
    from morgana_amd import _lib
    lib = _lib.load()
    win_l, win_u = (ctypes.c_int * 3)(0, 1, 1), (ctypes.c_int * 3)(0, 1, 1)
    win_c = (ctypes.c_double * 15)(1.0, 0, 0, 0, 0, -0.5, 0.0, 0.5, 0, 0, 1.0, -2.0, 1.0, 0, 0)
    need = lib.mg_mlpg_gv_workspace_bytes(6, 24, 3, 3, 3, win_l, win_u)
    assert need == 2 * lib.mg_mlpg_workspace_bytes(6, 24, 3, 3, 3, win_l, win_u) == 2 * 4 * 30 * 18 * 8

    def call(means=64, gv_mean=64, b=6, n_windows=3, gv_weight=1.0, max_iter=48, workspace=64, workspace_bytes=need):
        return lib.mg_mlpg_gv_f32(means, 64, 0, gv_mean, 64, 0, None, b, 24, 3, n_windows, win_l, win_u, win_c, 3, gv_weight, max_iter, 64, 0,
                                  None, workspace, workspace_bytes, None)

    for kwargs, message in (({'means': None}, 'null argument'), ({'gv_mean': None}, 'null argument'), ({'b': 0}, 'bad shape'),
                            ({'n_windows': 5}, 'windows supported'), ({'gv_weight': -1.0}, 'gv_weight'),
                            ({'gv_weight': float('nan')}, 'gv_weight'), ({'gv_weight': float('inf')}, 'gv_weight'),
                            ({'max_iter': 2}, 'max_iter')):
        assert call(**kwargs) == _lib.MG_EINVAL and message in _lib.last_error(), kwargs
    assert call(workspace_bytes=need - 1) == _lib.MG_EWORKSPACE and 'workspace' in _lib.last_error()
    assert call(workspace=None) == _lib.MG_EWORKSPACE
    assert _lib.SIGNATURES['mg_mlpg_gv_f32'][1][15] is ctypes.c_double and _lib.SIGNATURES['mg_mlpg_gv_f32'][1][16] is ctypes.c_int
