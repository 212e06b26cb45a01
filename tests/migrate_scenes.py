"""Shared by tests/test_migrate_model.py (CPU), tests/test_migrate_gpu.py and tests/test_migrate_replay_gpu.py: the
geometries, the tables, the impulse-reference CPIs and the moving-echo scene of the range-migration tests.  No test in here, no
GPU, no library call.

(a) Impulse-reference CPIs.  The reference channel is 1 at the first sample of every pulse and 0 elsewhere, the surveillance
channel has a modulus uniform in [0.5, 1.5] and a uniform phase at every sample, and delayMin is 0: the range map is then
R[i][d] = y[i nCorr + d] (times a phase per pulse where the Doppler limits are asymmetric) -- known, all cells different, all
of one size, so that a sum along a wrong walk misses by a large part of the peak.

(b) The moving-echo scene.  fs 200 kHz, n 40 000, delays -3 .. 40, Doppler +-160 Hz, roundHamming: a 65 x 44 map with nCorr
615.  A unit-power white reference; one echo of amplitude 0.05 on Doppler bin +30 (row 62, 150.09 Hz) whose delay is 20 samples
in the middle of the CPI and falls by 8 samples over it, pulse by pulse (a phase ramp on the FFT of the whole reference per
pulse); white noise of sigma 0.3.  fc = f nCorr nD / 8 makes the physical table walk those 8 samples.
"""
import numpy as np

from oracle import blah2_oracle as O

MAX_MIGRATION = 512  # BLAH2HIP_MAX_MIGRATION

# (delayMin, delayMax, dopplerMin, dopplerMax, fs, n), n_doppler_bins -> nD x nDelay; every one with roundHamming
GEOMS = {
    "g65x44": ((0, 43, -160, 160, 200_000, 40_000), 0),
    "g65x45": ((0, 44, -160, 160, 200_000, 40_000), 0),       # odd cell count: CPI 1 sits 8 bytes off a 16-byte boundary
    "g129x111": ((0, 110, -320, 320, 200_000, 40_000), 0),    # two column strips; shifts cross tile and strip seams
    "g2049x40": ((0, 39, -5000, 5000, 1_000_000, 204_900), 0),  # 65 blocks of 32 pulses
    "g64x44": ((0, 43, -160, 160, 200_000, 40_000), 64),      # the explicit even bin count
    "gasym": ((0, 43, -100, 220, 200_000, 40_000), 0),        # asymmetric Doppler limits: the reference channel is rotated
}
SHAPES = {"g65x44": (65, 44), "g65x45": (65, 45), "g129x111": (129, 111), "g2049x40": (2049, 40), "g64x44": (64, 44),
          "gasym": (65, 44)}
DB_TOL = 1e-3  # the project's gate for noisePower and maxPower, dB


def dims_of(name):
    limits, bins = GEOMS[name]
    d = O.ambiguity_dims(*limits, True, bins)
    assert (d.n_doppler_bins, d.n_delay_bins) == SHAPES[name]
    return d


def impulse_cpis(dims, n_cpi, seed, gap=0):
    """(x, y, stride): complex64 planes of ``n_cpi`` CPIs, ``stride`` samples from one CPI to the next (``gap`` samples of
    NaN between the planes' CPIs, which no kernel may read)."""
    rng = np.random.default_rng(seed)
    used = dims.n_doppler_bins * dims.n_corr
    stride = used + gap
    x = np.full(n_cpi * stride, np.nan + 1j * np.nan, dtype=np.complex64)
    y = x.copy()
    for c in range(n_cpi):
        xc = np.zeros(used, dtype=np.complex64)
        xc[::dims.n_corr] = 1.0
        mod = rng.uniform(0.5, 1.5, used)
        ph = rng.uniform(0.0, 2.0 * np.pi, used)
        x[c * stride:c * stride + used] = xc
        y[c * stride:c * stride + used] = (mod * np.exp(1j * ph)).astype(np.complex64)
    return x, y, stride


def fc_for(dims, cells):
    """The carrier at which the physical table's outermost row walks ``cells`` cells from the middle of the CPI to its end
    (a quarter cell more, so that the figure does not sit on a rounding tie)."""
    return 0.5 * float(np.abs(dims.doppler).max()) * dims.n_corr * (dims.n_doppler_bins - 1) / (cells + 0.25)


def physical(dims, fc):
    return -0.5 * dims.doppler * float(dims.n_corr) / fc


def tables(dims, cells):
    """name -> half walks.  ``physical`` walks ``cells`` cells; ``beyond`` walks past the map's last column, so that its outer
    rows keep only the central pulses; ``limit`` runs from exactly -MAX_MIGRATION to exactly +MAX_MIGRATION; ``jagged`` gives
    neighbouring rows opposite walks of up to the limit (the widest window a workgroup can meet)."""
    nD = dims.n_doppler_bins
    phys = physical(dims, fc_for(dims, cells))
    jag = np.where(np.arange(nD) % 2 == 0, 1.0, -1.0) * np.linspace(0.0, MAX_MIGRATION, nD) / (nD - 1)
    return {
        "physical": phys,
        "reversed": -phys,
        "beyond": physical(dims, fc_for(dims, dims.n_delay_bins + 16)),
        "limit": np.linspace(-MAX_MIGRATION, MAX_MIGRATION, nD) / (nD - 1),
        "jagged": jag,
    }


def zero_rows(half, nD):
    """The rows the library copies: rint(h[j] (nD - 1)) == 0."""
    return np.rint(np.asarray(half, dtype=np.float64) * float(nD - 1)) == 0


def set_metrics64(z):
    """Map::set_metrics (Map.cpp:187-206) in fp64: (noisePower, maxPower) of one map."""
    with np.errstate(divide="ignore", invalid="ignore"):
        db = 10.0 * np.log10(np.abs(np.asarray(z).astype(np.complex128)))
    noise = db.mean()
    return noise, max(0.0, db.max()) - noise


# ---- (b) the moving-echo scene ----------------------------------------------------------------------------------------------
SCENE_LIMITS = (-3, 40, -160, 160, 200_000, 40_000)
SCENE_BIN, SCENE_ROW, SCENE_DELAY, SCENE_COL = 30, 62, 20, 23
SCENE_WALK, SCENE_AMP, SCENE_SIGMA = 8.0, 0.05, 0.3


def scene_dims():
    d = O.ambiguity_dims(*SCENE_LIMITS, True)
    assert (d.n_doppler_bins, d.n_delay_bins, d.n_corr) == (65, 44, 615)
    return d


def scene_fc(dims):
    return float(dims.doppler[SCENE_ROW]) * dims.n_corr * dims.n_doppler_bins / SCENE_WALK


def scene(seed=5, walk=SCENE_WALK):
    """(x, y) complex128 of SCENE_LIMITS[5] samples; ``walk`` 0 is the same echo at a fixed delay."""
    dims = scene_dims()
    n, nD, nC = dims.n_samples, dims.n_doppler_bins, dims.n_corr
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    noise = SCENE_SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    X = np.fft.fft(x)
    k = np.fft.fftfreq(n)  # cycles per sample
    f = float(dims.doppler[SCENE_ROW])
    t = np.arange(n) / dims.fs
    echo = np.zeros(n, dtype=np.complex128)
    for i in range(nD):
        tau = SCENE_DELAY - walk * (i - (nD - 1) / 2.0) / nD  # approaching: the delay falls
        seg = slice(i * nC, (i + 1) * nC if i + 1 < nD else n)
        echo[seg] = np.fft.ifft(X * np.exp(-2j * np.pi * k * tau))[seg]
    y = SCENE_AMP * echo * np.exp(2j * np.pi * f * t) + noise
    return x, y


def level_db(m, row, col):
    return 20.0 * np.log10(np.abs(m[row, col]))
