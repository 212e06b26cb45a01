"""ula_weights: the conjugate steering vectors of a uniform line array over the element count,
w[b][k] = exp(-2 pi j k d sin(theta_b)) / K -- pure NumPy, importable without a device."""
import numpy as np


def formula(K, d, angles_deg):
    return np.array([[np.exp(-2j * np.pi * k * d * np.sin(np.deg2rad(a))) / K for k in range(K)] for a in angles_deg])


def test_broadside_is_uniform():
    from blah2_amd import ula_weights
    for K in (1, 3, 4, 8):
        w = ula_weights(K, 0.5, [0.0])
        assert w.shape == (1, K) and w.dtype == np.complex128
        assert np.array_equal(w, np.full((1, K), 1.0 / K + 0j))


def test_steered_angles_against_the_formula():
    from blah2_amd import ula_weights
    angles = [-40.0, 0.0, 17.5, 30.0, 90.0]
    for K, d in ((4, 0.5), (5, 0.37), (8, 1.0)):
        w = ula_weights(K, d, angles)
        assert w.shape == (len(angles), K)
        assert np.allclose(w, formula(K, d, angles), rtol=0, atol=4 * np.finfo(np.float64).eps * 2 * np.pi * K * d)
    # 30 degrees at half-wave spacing: a quarter turn from element to element
    w = ula_weights(4, 0.5, [30.0])[0]
    assert np.allclose(w * 4, [1, -1j, -1, 1j], rtol=0, atol=1e-14)  # a few ulp of the largest phase, 3 pi / 2
    # the beam towards an angle has unit gain for a plane wave from it
    a = np.exp(2j * np.pi * np.arange(5) * 0.37 * np.sin(np.deg2rad(17.5)))
    assert abs(ula_weights(5, 0.37, [17.5])[0] @ a - 1.0) < 1e-14


def test_a_scalar_angle_gives_one_beam():
    from blah2_amd import ula_weights
    assert ula_weights(3, 0.5, 10.0).shape == (1, 3)


def test_import_needs_no_device():
    import subprocess
    import sys
    code = ("import os; os.environ['HIP_VISIBLE_DEVICES'] = ''; os.environ['ROCR_VISIBLE_DEVICES'] = ''\n"
            "from blah2_amd.process import ula_weights; print(ula_weights(2, 0.5, [0.0]).shape)")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=__import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
    assert r.returncode == 0 and "(1, 2)" in r.stdout, r.stderr
