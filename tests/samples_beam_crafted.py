"""The sample-domain array scene and its fp64 models, shared by tests/test_beam_samples_host.py (NumPy only) and
tests/test_beam_samples_gpu.py.  Nothing here touches the GPU.

A half-wave line array of K = 4 channels in front of the 1 MS/s geometry of the beamformer's tests (21 x 111 cells,
100 000 samples per CPI; a second geometry has 100 001):
  * the reference x: unit-variance complex normal noise,
  * every channel: unit-variance noise of its own,
  * the direct path: x itself, 30 dB over the noise, from -24 degrees (the first sidelobe of the conventional 20 degree
    beam of four elements),
  * an echo: x delayed 37 samples and shifted -40 Hz, 25 dB UNDER the noise per sample, from +20 degrees -- after the
    50 dB of a CPI's integration it stands 25 dB over the map's floor, in row 6 (-40 Hz) and column 47 (lag 37),
  * steering +20 degrees, loading 1e-3.
The int8 variant scales the channels so that their largest component is 100 and x by 30, and rounds both; the models and
the oracle are fed the quantised values.

What the fp64 restatement gives (oracle.ambiguity_process, seeds 7-9): cond(R_l) about 2.0e3 at 30 dB; the conventional
beam's map peaks at the direct path (zero Doppler, lag 0: row 10, column 10), the MVDR beam's at the target cell; the map
of sum_k w_k y_k equals sum_k w_k map(y_k) to 1e-13 of the peak.
"""
import numpy as np

from blah2_amd import beam_samples, mvdr_weights, sample_covariance, ula_steering, ula_weights  # noqa: F401
from oracle import blah2_oracle as O

K = 4
SPACING = 0.5
GEOM = (-10, 100, -100, 100, 1_000_000, 100_000)      # 21 x 111 cells, 100 000 samples
GEOM_ODD = (-10, 100, -100, 100, 1_000_000, 100_001)  # the same map from an odd sample count
DIRECT_DEG, DIRECT_DB = -24.0, 30.0
ECHO_DEG, ECHO_DB, ECHO_LAG, ECHO_HZ = 20.0, -25.0, 37, -40.0
STEER_DEG = 20.0
LOADING = 1e-3
SEEDS = (7, 8, 9)
TARGET_CELL = (6, 47)
DIRECT_CELL = (10, 10)
COND_MAX = 1e5  # what the weight bound of tests/test_adaptive_beam_gpu.py assumes


def dims(geom=GEOM):
    return O.ambiguity_dims(*geom, True)


def _cn(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)


def scene(seed, n=GEOM[5], fs=GEOM[4], direct_db=DIRECT_DB):
    """(x complex64 [n], ys complex64 [K, n]) of one CPI."""
    rng = np.random.default_rng(seed)
    x = _cn(rng, n)
    t = np.arange(n)
    echo = np.concatenate([np.zeros(ECHO_LAG, dtype=np.complex128), x[:n - ECHO_LAG]]) * np.exp(2j * np.pi * ECHO_HZ * t / fs)
    a_d = ula_steering(K, SPACING, [DIRECT_DEG])[0]
    a_e = ula_steering(K, SPACING, [ECHO_DEG])[0]
    ys = np.stack([_cn(rng, n) for _ in range(K)])
    ys = ys + 10.0 ** (direct_db / 20.0) * a_d[:, None] * x[None] + 10.0 ** (ECHO_DB / 20.0) * a_e[:, None] * echo[None]
    return x.astype(np.complex64), ys.astype(np.complex64)


def quantise(x, ys):
    """The int8 variant: (x int8 [n, 2], ys int8 [K, n, 2]), the channels' largest component at 100, x scaled by 30."""
    top = max(np.abs(ys.real).max(), np.abs(ys.imag).max())
    yq = np.rint(np.stack([ys.real, ys.imag], axis=-1).astype(np.float64) * (100.0 / top))
    xq = np.rint(np.stack([x.real, x.imag], axis=-1).astype(np.float64) * 30.0)
    assert np.abs(yq).max() == 100 and np.abs(xq).max() <= 127
    return xq.astype(np.int8), yq.astype(np.int8)


def as_complex(q):
    """int8 pairs [..., 2] -> complex128 [...], exactly."""
    q = np.asarray(q)
    return q[..., 0].astype(np.float64) + 1j * q[..., 1].astype(np.float64)


def batch(fmt_i8, seeds=SEEDS, geom=GEOM):
    """The CPIs of ``seeds`` side by side: (x [n_cpi, n], ys [K, n_cpi, n]) as complex64, or as int8 pairs with a last axis
    of 2 when ``fmt_i8``."""
    xs, yss = [], []
    for s in seeds:
        x, ys = scene(s, n=geom[5], fs=geom[4])
        if fmt_i8:
            x, ys = quantise(x, ys)
        xs.append(x)
        yss.append(ys)
    return np.stack(xs), np.stack(yss, axis=1)


def covariance_int(yq, s0=0, s1=None):
    """int8 pairs [K, ..., n, 2] -> (re, im) int64 [..., K, K, 2]: the covariance in integer arithmetic."""
    q = np.asarray(yq).astype(np.int64)[..., s0:s1, :]
    re, im = q[..., 0], q[..., 1]
    rr = np.einsum("i...n,j...n->...ij", re, re) + np.einsum("i...n,j...n->...ij", im, im)
    ri = np.einsum("i...n,j...n->...ij", im, re) - np.einsum("i...n,j...n->...ij", re, im)
    return np.stack([rr, ri], axis=-1)


def loaded_cond(R, loading=LOADING):
    k = R.shape[-1]
    return float(np.linalg.cond(R + loading * (np.trace(R).real / k) * np.eye(k)))


def steer():
    return ula_steering(K, SPACING, [STEER_DEG])


def conventional():
    """conj(a) / K towards STEER_DEG, [1, K]."""
    return ula_weights(K, SPACING, [STEER_DEG])


def oracle_map(x, y, geom=GEOM):
    return O.ambiguity_process(dims(geom), x, y)


def peak_cell(m):
    return tuple(int(v) for v in np.unravel_index(int(np.argmax(np.abs(m))), np.asarray(m).shape))
