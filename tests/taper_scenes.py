"""Shared by tests/test_taper_model.py (CPU) and tests/test_taper_gpu.py: the geometries, the crafted maps and the masking
scene of the Doppler taper's tests.  No test in here, no GPU, no library call.

The masking scene: 101 pulses x 64 delay bins of unit-variance complex noise in the range map; in column 30 an echo of
amplitude 200 per pulse at 10.5 cycles per CPI (between two Doppler bins: its rectangular-window ridge runs along the whole
column at -13 dB and falling) and one of amplitude 2.5 at -20 cycles per CPI.  The map is the Doppler transform of the range
map in the reference's row order, row j at j - 50 cycles per CPI.  The 1-D detector (pfa 1e-4, guard 2, train 6) trains along
delay, so it reports the ridge itself; a "stray" is a detection in column 30 more than 3.6 bins from both echoes.
"""
import numpy as np

from oracle import blah2_oracle as O

# (delayMin, delayMax, dopplerMin, dopplerMax, fs, n), n_doppler_bins -> the map
GEOMS = {
    "odd": ((-10, 100, -100, 100, 1_000_000, 100_000), 0),     # 21 x 111: rows alternate between 16-byte aligned and 8 off
    "even": ((-10, 101, -100, 100, 1_000_000, 100_000), 0),    # 21 x 112
    "thin": ((-10, 250, -40, 40, 1_000_000, 100_000), 0),      # 9 x 261: nD = 2P + 1 at P = 4, two column strips
    "even16": ((-10, 100, -100, 100, 1_000_000, 100_000), 16),  # 16 x 111: the explicit even bin count
}
SHAPES = {"odd": (21, 111), "even": (21, 112), "thin": (9, 261), "even16": (16, 111)}
PRESETS = ("hann", "hamming", "blackman", "blackmanharris", "nuttall", "flattop")
DB_TOL = 1e-3  # the project's gate for noisePower and maxPower, dB

SCENE_PULSES, SCENE_BINS, SCENE_COL = 101, 64, 30
SCENE_STRONG, SCENE_WEAK = (200.0, 10.5), (2.5, -20.0)  # (amplitude per pulse, cycles per CPI)
SCENE_SEEDS = (7, 8, 9)
SCENE_CFAR = dict(pfa=1e-4, n_guard=2, n_train=6)
SCENE_KEEP = 3.6  # Doppler bins around an echo that are not strays


def level(n_maps):
    return 1.0 + 0.25 * ((5 * np.arange(n_maps)) % 7)


def maps(n_maps, nD, nC, seed):
    """complex64 [n_maps, nD, nC] whose cells all differ: |M| = level(map) u, u uniform in [0.7, 1.4] per cell, uniform
    phase (tests/integrate_crafted.py draws its maps the same way)."""
    rng = np.random.default_rng(seed)
    shape = (n_maps, nD, nC)
    phase = rng.uniform(0, 1, shape)
    u = rng.uniform(0.7, 1.4, shape)
    return ((level(n_maps)[:, None, None] * u) * np.exp(2j * np.pi * phase)).astype(np.complex64)


def stencil_bound(m, taps):
    """B = sum_m |t_m| |M[j + m]| per cell (fp64), the scale of the kernel's 2P + 1 roundings: each is at most 2^-24 of it
    per component, sqrt(2) of that for the complex cell."""
    a = np.abs(np.asarray(m).astype(np.complex128))
    t = np.abs(np.asarray(taps, dtype=np.float64))
    B = t[0] * a
    for k in range(1, t.size):
        B = B + t[k] * (np.roll(a, k, axis=-2) + np.roll(a, -k, axis=-2))
    return B


def cell_bound(m, taps):
    P = len(taps) - 1
    return np.sqrt(2.0) * (2 * P + 1) * 2.0 ** -24 * stencil_bound(m, taps)


def set_metrics64(z):
    """Map::set_metrics (Map.cpp:187-206) in fp64: (noisePower, maxPower) of one map."""
    with np.errstate(divide="ignore", invalid="ignore"):
        db = 10.0 * np.log10(np.abs(np.asarray(z).astype(np.complex128)))
    noise = db.mean()
    return noise, max(0.0, db.max()) - noise


def scene_axes():
    return np.arange(SCENE_BINS), np.arange(SCENE_PULSES) - float((SCENE_PULSES - 1) // 2)


def scene_map(seed):
    """The untapered fp64 map [101, 64] of the masking scene."""
    rng = np.random.default_rng(seed)
    nP, nB = SCENE_PULSES, SCENE_BINS
    R = (rng.standard_normal((nP, nB)) + 1j * rng.standard_normal((nP, nB))) / np.sqrt(2.0)
    p = np.arange(nP)
    for amp, cyc in (SCENE_STRONG, SCENE_WEAK):
        R[:, SCENE_COL] += amp * np.exp(2j * np.pi * cyc * p / nP)
    D = np.fft.fft(R, axis=0)
    return D[(np.arange(nP) + nP // 2 + 1) % nP, :]  # Ambiguity.cpp:165


def scene_verdict(delay, doppler):
    """(strays, weak echo detected) of a detection list (delay, doppler in cycles per CPI)."""
    delay, doppler = np.asarray(delay), np.asarray(doppler)
    col = doppler[delay == SCENE_COL]
    far = (np.abs(col - SCENE_STRONG[1]) > SCENE_KEEP) & (np.abs(col - SCENE_WEAK[1]) > SCENE_KEEP)
    return int(far.sum()), bool((col == SCENE_WEAK[1]).any())


def scene_detect(m):
    """The oracle's 1-D detector on a scene map -> (strays, weak echo detected)."""
    delay_axis, doppler_axis = scene_axes()
    noise, _ = O.map_metrics(m)
    d, f, _ = O.cfar1d_fast(m, delay_axis, doppler_axis, noise, SCENE_CFAR["pfa"], SCENE_CFAR["n_guard"], SCENE_CFAR["n_train"],
                            0, 0.0)
    return scene_verdict(d, f)
