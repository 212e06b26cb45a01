"""The adaptive-beam scenario shared by tests/test_adaptive_beam_host.py (NumPy only) and tests/test_adaptive_beam_gpu.py.

A half-wave line array of K = 4 channels behind a 21 x 111 map (the 1 MS/s geometry of the beamformer's tests):
  * unit-variance complex normal cells per channel (the noise floor of a channel map),
  * an interferer from -24 degrees -- the first sidelobe of the conventional 20 degree beam of four elements -- at 40 dB per
    cell (amplitude 100, a random phase per cell) on the three rows around zero Doppler, across all delays: residual direct
    path and clutter,
  * a target from +20 degrees at 25 dB in one cell outside those rows.
The cells are rounded to complex64, what a device map holds; the fp64 pipeline below starts from those values.
"""
import numpy as np

from blah2_amd import mvdr_weights, ula_steering, ula_weights

K = 4
SPACING = 0.5
ND, NC = 21, 111
INTERFERER_DEG, INTERFERER_DB = -24.0, 40.0
TARGET_DEG, TARGET_DB = 20.0, 25.0
INTERFERER_ROWS = (9, 10, 11)   # zero Doppler is row 10 of 21
TARGET_CELL = (4, 60)           # -60 Hz, delay 50 in that geometry
BEAMS_DEG = (20.0, 0.0)
LOADING = 1e-3
SEED = 2024


def scene(seed=SEED):
    """Channel maps complex64 [K, 1, ND, NC]."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((K, ND, NC)) + 1j * rng.standard_normal((K, ND, NC))) * np.sqrt(0.5)
    a_i = ula_steering(K, SPACING, [INTERFERER_DEG])[0]
    a_t = ula_steering(K, SPACING, [TARGET_DEG])[0]
    phase = np.exp(2j * np.pi * rng.random((len(INTERFERER_ROWS), NC)))
    z[:, list(INTERFERER_ROWS), :] += 10.0 ** (INTERFERER_DB / 20.0) * a_i[:, None, None] * phase[None]
    z[:, TARGET_CELL[0], TARGET_CELL[1]] += 10.0 ** (TARGET_DB / 20.0) * a_t
    return z[:, None].astype(np.complex64)


def covariance64(maps, region=None):
    """R[c][i][j] = sum over the region of M_i conj(M_j) in fp64; maps [K, n_cpi, nD, nC] -> [n_cpi, K, K]."""
    m = np.asarray(maps).astype(np.complex128)
    if region is not None:
        r0, r1, c0, c1 = region
        m = m[:, :, r0:r1, c0:c1]
    return np.einsum("icrq,jcrq->cij", m, np.conj(m))


def beams64(maps, w):
    """M_b(c) = sum_k w[c][b][k] M_k(c) in fp64; maps [K, n_cpi, ...], w [n_cpi, n_beams, K] -> [n_beams, n_cpi, ...]."""
    return np.einsum("cbk,kcrq->bcrq", np.asarray(w, dtype=np.complex128), np.asarray(maps).astype(np.complex128))


def pipeline64(maps, beams_deg=BEAMS_DEG, loading=LOADING):
    """(R, w, ok, beam maps) of the whole-map covariance and the MVDR beams, all fp64 NumPy."""
    R = covariance64(maps)
    w, ok = mvdr_weights(R, ula_steering(K, SPACING, beams_deg), loading)
    return R, w, ok, beams64(maps, w)


def conventional64(maps, beams_deg=BEAMS_DEG):
    w = ula_weights(K, SPACING, beams_deg)
    return beams64(maps, np.broadcast_to(w, (np.asarray(maps).shape[1],) + w.shape))


def interferer_db(beam_map):
    """Mean power of the interferer rows of one beam map [nD, nC], in dB."""
    return 10.0 * np.log10(np.mean(np.abs(np.asarray(beam_map)[list(INTERFERER_ROWS), :].astype(np.complex128)) ** 2))


def target_db(beam_map):
    return 20.0 * np.log10(abs(complex(np.asarray(beam_map)[TARGET_CELL])))
