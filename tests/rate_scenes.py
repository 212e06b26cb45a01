"""Shared by tests/test_rate_bank_model.py (CPU), tests/test_rate_bank_gpu.py and tests/test_rate_bank_replay_gpu.py: the
banks and the accelerating-echo scene of the Doppler-rate tests, on the geometries, tables and impulse-reference CPIs of
tests/migrate_scenes.py.  No test in here, no GPU, no library call.

The accelerating scene is migrate_scenes.scene -- the 65 x 44 map, a white reference, one echo of amplitude 0.05 on row 62 whose
delay is 20 samples at mid-CPI and falls by ``walk`` samples over it, white noise of sigma 0.3 -- with the echo multiplied by
exp(2 pi i (1/2) (q / T^2) (t - T/2)^2), T = nD nCorr / fs: its Doppler rises by q bins over the CPI and passes row 62 at mid-CPI.
"""
import numpy as np

import migrate_scenes as MS

MAX_RATES = 16  # BLAH2HIP_MAX_RATES
SCENE_Q = 6.0


def scene(seed=5, walk=MS.SCENE_WALK, q=SCENE_Q):
    """(x, y) complex128; ``q`` 0 is migrate_scenes.scene.  The noise is the scene's own second draw, so the echo is what is
    left of y without it."""
    dims = MS.scene_dims()
    x, y = MS.scene(seed, walk)
    n = dims.n_samples
    rng = np.random.default_rng(seed)
    rng.standard_normal(2 * n)  # the reference's draws
    noise = MS.SCENE_SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    T = dims.n_doppler_bins * dims.n_corr / dims.fs
    t = np.arange(n) / dims.fs
    chirp = np.exp(2j * np.pi * 0.5 * (q / T ** 2) * (t - T / 2.0) ** 2)
    return x, (y - noise) * chirp + noise


def uneven_bank(nD):
    """16 unevenly spaced rates up to +-nD/4, 0 among them, in no order."""
    u = np.array([0.0, 0.37, -0.81, 1.0, -2.5, 3.25, 5.0, -7.75, 0.11, -0.043, 0.62, -0.29, 0.9, -0.5, -1.0, 1.0 / 3.0])
    assert u.size == MAX_RATES
    return u / 7.75 * (nD / 4.0)
