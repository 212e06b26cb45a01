"""The two-carrier scene and the fp64 restatement chain for the down-converter's tests (test_ddc_model.py,
test_ddc_gpu.py, test_ddc_replay_gpu.py).

Seed 7: fs = 65 536 Hz, two pieces of 32 768 samples (one second in all), two illuminators band-limited to |nu| <= 0.08
cycles per sample and of unit power, at +16 384 Hz (A) and -12 288 Hz (B); x is their sum.  y is 0.2 x plus echo A
(illuminator A delayed by 24 samples, +40 Hz, amplitude 0.05), echo B (illuminator B delayed by 44 samples, -24 Hz, 0.05)
and noise of 0.01 per component.  Down-converted by D = 4 with T = 64 taps (cutoff 0.8, beta 8) each carrier is a
16 384-sample CPI at 16 384 Hz: 1 Hz Doppler bins, echo A at delay 24 / 4 = 6 of carrier A's map, echo B at 44 / 4 = 11 of
carrier B's.  Both channels pass the same taps, so the filter's group delay moves no peak.
"""
import numpy as np

from oracle import blah2_oracle as O

FS, PIECE, PIECES, D, T = 65536, 32768, 2, 4, 64
N = PIECE * PIECES
CARRIERS = (16384.0, -12288.0)
ECHOES = ((24, 40.0, 0.05), (44, -24.0, 0.05))  # (delay in input samples, Doppler in Hz, amplitude), one per carrier
AMB_ARGS = (-4, 20, -64, 64, FS // D, N // D)
PEAKS = ((6, 40.0), (11, -24.0))  # (delay, Doppler) of each carrier's map
ZERO_ROWS = 3.0  # rows with |Doppler| <= this many Hz hold the direct path: "the zero-Doppler rows"


def band_limited(rng, n, band):
    w = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    W = np.fft.fft(w)
    W[np.abs(np.fft.fftfreq(n)) > band] = 0
    x = np.fft.ifft(W)
    return x / np.sqrt(np.mean(np.abs(x) ** 2))


def scene(seed=7):
    """(x, y) complex128 of N samples."""
    rng = np.random.default_rng(seed)
    t = np.arange(N) / FS
    ill = [band_limited(rng, N, 0.08) * np.exp(2j * np.pi * f * t) for f in CARRIERS]
    x = ill[0] + ill[1]
    y = 0.2 * x
    for s, (d, f, a) in zip(ill, ECHOES):
        e = np.zeros(N, dtype=np.complex128)
        e[d:] = s[:N - d]
        y = y + a * e * np.exp(2j * np.pi * f * t)
    y = y + 0.01 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    return x, y


def taps():
    import blah2_amd
    return blah2_amd.ddc_design(D, T, 0.8, 8.0)


def model_planes(x, y, f, g=None):
    """The restatement's (x, y) planes of the carrier at offset f (complex128 [2][N / D])."""
    import blah2_amd
    v, _ = blah2_amd.ddc(np.stack([x, y]), f, FS, D, taps(), g=g)
    return v


def oracle_map(planes):
    dims = O.ambiguity_dims(*AMB_ARGS)
    return dims, O.ambiguity_process(dims, planes[0], planes[1])


def peak_off_zero(m, dims):
    """((delay, Doppler) of the largest cell off the zero-Doppler rows, its dB over the map's median cell)."""
    a = np.abs(np.asarray(m))
    f = np.asarray(dims.doppler)
    masked = np.where((np.abs(f) > ZERO_ROWS)[:, None], a, 0.0)
    i, j = np.unravel_index(int(np.argmax(masked)), a.shape)
    return (int(dims.delay[j]), float(f[i])), float(20.0 * np.log10(a[i, j] / np.median(a)))
