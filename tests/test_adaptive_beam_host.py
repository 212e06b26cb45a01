"""ula_steering and mvdr_weights -- pure NumPy, importable without a device -- and the conditions the adaptive-beam
scenario of tests/adaptive_crafted.py must meet in fp64 before tests/test_adaptive_beam_gpu.py holds the device to it."""
import numpy as np
import pytest

import adaptive_crafted as A


def hermitian(K, n, seed, batch=()):
    """A sample covariance of n unit-variance snapshots plus a strong rank-one interferer: well conditioned once loaded."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(batch + (K, n)) + 1j * rng.standard_normal(batch + (K, n))) * np.sqrt(0.5)
    x = x + 30.0 * np.exp(2j * np.pi * 0.21 * np.arange(K))[:, None] * (rng.standard_normal(batch + (1, n)) + 0j)
    return x @ np.conj(np.swapaxes(x, -1, -2))


def test_ula_steering_against_the_formula_and_ula_weights():
    from blah2_amd import ula_steering, ula_weights
    angles = [-40.0, 0.0, 17.5, 30.0, 90.0]
    for K, d in ((1, 0.5), (4, 0.5), (5, 0.37), (8, 1.0)):
        a = ula_steering(K, d, angles)
        assert a.shape == (len(angles), K) and a.dtype == np.complex128
        want = np.array([[np.exp(2j * np.pi * k * d * np.sin(np.deg2rad(t))) for k in range(K)] for t in angles])
        assert np.allclose(a, want, rtol=0, atol=4 * np.finfo(np.float64).eps * 2 * np.pi * K * d)
        assert np.allclose(a, np.conj(ula_weights(K, d, angles)) * K, rtol=0, atol=4 * np.finfo(np.float64).eps)
    assert ula_steering(3, 0.5, 10.0).shape == (1, 3)


def test_identity_covariance_gives_the_conventional_weights():
    from blah2_amd import mvdr_weights, ula_steering, ula_weights
    for K in (1, 2, 4, 8):
        a = ula_steering(K, 0.5, [0.0, 20.0, -35.0])
        for loading in (0.0, 1e-3, 2.0):
            w, ok = mvdr_weights(np.eye(K), a, loading)
            assert w.shape == (3, K) and ok.shape == () and ok == 1
            assert np.allclose(w, ula_weights(K, 0.5, [0.0, 20.0, -35.0]), rtol=0, atol=1e-15)


@pytest.mark.parametrize("K", [1, 2, 3, 4, 8])
def test_distortionless_and_equal_to_a_general_solve(K):
    from blah2_amd import mvdr_weights, ula_steering
    R = hermitian(K, 200, seed=K)
    a = ula_steering(K, 0.5, [20.0, 0.0, -50.0])
    loading = 1e-3
    w, ok = mvdr_weights(R, a, loading)
    assert ok == 1
    Rl = R + loading * (np.trace(R).real / K) * np.eye(K)
    for b in range(a.shape[0]):
        assert abs(w[b] @ a[b] - 1.0) <= 1e-12
        x = np.linalg.solve(Rl, a[b])
        h = x / (np.conj(a[b]) @ x)
        assert np.allclose(w[b], np.conj(h), rtol=0, atol=1e-12 * np.linalg.cond(Rl) * np.abs(h).max())


def test_zero_and_nan_covariances_fail_to_the_conventional_weights():
    from blah2_amd import mvdr_weights, ula_steering
    K = 4
    a = ula_steering(K, 0.5, [20.0, 0.0])
    a[1] *= 3.0  # not unit modulus: the fallback divides by a^H a
    conventional = np.conj(a) / (np.abs(a) ** 2).sum(axis=1)[:, None]
    nan_diag, nan_off = hermitian(K, 50, seed=1), hermitian(K, 50, seed=2)
    nan_diag[2, 2] = np.nan
    nan_off[3, 1] = np.nan  # lower triangle
    for R in (np.zeros((K, K)), nan_diag, nan_off, -np.eye(K), np.full((K, K), np.inf)):
        w, ok = mvdr_weights(R, a, 1e-3)
        assert ok == 0
        assert np.array_equal(w, conventional)


def test_batch_dimensions_broadcast():
    from blah2_amd import mvdr_weights, ula_steering
    K = 3
    a = ula_steering(K, 0.5, [10.0, -10.0])
    R = hermitian(K, 40, seed=9, batch=(2, 3))
    R[1, 1] = 0.0
    w, ok = mvdr_weights(R, a, 1e-2)
    assert w.shape == (2, 3, 2, K) and ok.shape == (2, 3) and ok.dtype == np.int32
    assert ok.tolist() == [[1, 1, 1], [1, 0, 1]]
    for i in range(2):
        for j in range(3):
            w1, ok1 = mvdr_weights(R[i, j], a, 1e-2)
            assert ok1 == ok[i, j] and np.array_equal(w1, w[i, j])
    with pytest.raises(ValueError):
        mvdr_weights(R, a, -1.0)
    with pytest.raises(ValueError):
        mvdr_weights(R, np.zeros((1, K)), 0.1)


def test_helpers_import_without_a_device():
    import os
    import subprocess
    import sys
    code = ("import os; os.environ['HIP_VISIBLE_DEVICES'] = ''; os.environ['ROCR_VISIBLE_DEVICES'] = ''\n"
            "import numpy as np\n"
            "from blah2_amd.process import mvdr_weights, ula_steering\n"
            "print(mvdr_weights(np.eye(2), ula_steering(2, 0.5, [0.0]), 0.0)[0].shape)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root)
    assert r.returncode == 0 and "(1, 2)" in r.stdout, r.stderr


def test_the_scenario_meets_its_conditions_in_fp64():
    """The MVDR beam at 20 degrees leaves at least 20 dB less of the interferer than the conventional beam does, and keeps the
    target within 0.5 dB of its injected level: conditions on the scenario, which the GPU test then builds on."""
    maps = A.scene()
    assert maps.shape == (A.K, 1, A.ND, A.NC) and maps.dtype == np.complex64
    R, w, ok, mv = A.pipeline64(maps)
    assert ok.tolist() == [1]
    conv = A.conventional64(maps)
    i_conv, i_mvdr = A.interferer_db(conv[0, 0]), A.interferer_db(mv[0, 0])
    t_mvdr = A.target_db(mv[0, 0])
    print(f"interferer rows: conventional {i_conv:.2f} dB, MVDR {i_mvdr:.2f} dB; target cell {t_mvdr:.2f} dB (injected {A.TARGET_DB} dB)")
    assert i_conv - i_mvdr >= 20.0
    assert abs(t_mvdr - A.TARGET_DB) <= 0.5
    Rl = R[0] + A.LOADING * (np.trace(R[0]).real / A.K) * np.eye(A.K)
    assert np.linalg.cond(Rl) <= 1e5
