"""Scenes and the fp64 restatement chain for the strong-echo canceller's tests (test_clean_model.py, test_clean_gpu.py,
test_clean_replay_gpu.py).

The demonstration scene: N = 32768 samples at fs = 32768 Hz (one-second CPI, 1 Hz Doppler bins), unit-variance noise, a
reference band-limited to |nu| <= 1/8 and scaled to unit power, a strong echo of amplitude 10 at delay 20.4 samples and
37.3 Hz (off the delay grid and off the Doppler grid), a weak echo of amplitude 0.1 at delay 55 and -12 Hz.  The strong
echo's own sidelobes lift the whole map's floor by about 20 dB and bury the weak echo; fitting a cluster of three delays
and subtracting brings the floor back.

"Floor" below is the median cell POWER, 20 log10 |z|, over the check cells: delays 65 .. 100, every Doppler row further
than 4 Hz from the strong echo and 3 Hz from the weak one.
"""
import types

import numpy as np

from oracle import blah2_oracle as O

N, FS = 32768, 32768
AMB_ARGS = (-10, 100, -64, 64, FS, N)
STRONG = (10.0, 20.4, 37.3)
WEAK = (0.1, 55, -12.0)
DET = dict(pfa=1e-6, nGuard=2, nTrain=8, minDelay=-10, minDoppler=0.0, nCentroid=4)
CLEAN = dict(snr=18.0, echoes=4, sideDelay=1, sideDoppler=1, loading=1e-6)


def band_limited(rng, n, band=0.125):
    """Complex white noise low-passed to |nu| <= band cycles per sample, unit power."""
    w = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    W = np.fft.fft(w)
    W[np.abs(np.fft.fftfreq(n)) > band] = 0
    x = np.fft.ifft(W)
    return x / np.sqrt(np.mean(np.abs(x) ** 2))


def delayed(x, d):
    """x delayed by d >= 0 samples (fractional: a phase ramp on the spectrum), zero in front instead of wrapped."""
    n = x.shape[0]
    if float(d) == int(d):
        out = np.zeros_like(x)
        out[int(d):] = x[:n - int(d)]
        return out
    out = np.fft.ifft(np.fft.fft(x) * np.exp(-2j * np.pi * np.fft.fftfreq(n) * d))
    out[:int(np.ceil(d))] = 0
    return out


def demo_scene(seed=20261021, n=N, fs=FS):
    rng = np.random.default_rng(seed)
    x = band_limited(rng, n)
    noise = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    t = np.arange(n) / fs
    y = noise.copy()
    for a, d, f in (STRONG, WEAK):
        y += a * delayed(x, d) * np.exp(2j * np.pi * f * t)
    return x.astype(np.complex64), y.astype(np.complex64)


def check_cells(dims):
    f, d = np.asarray(dims.doppler)[:, None], np.asarray(dims.delay)[None, :]
    return (d >= 65) & (np.abs(f - STRONG[2]) > 4) & (np.abs(f - WEAK[2]) > 3)


def floor_db(m, dims):
    return float(np.median(20.0 * np.log10(np.abs(m[check_cells(dims)]))))


def cell_db(m, dims, delay, doppler):
    i = int(np.argmin(np.abs(np.asarray(dims.doppler) - doppler)))
    j = int(round(delay)) - int(dims.delay[0])
    return float(20.0 * np.log10(np.abs(m[i, j])))


def detect(dims, m, det=DET):
    """Map -> final records (DET_DTYPE), the restatement of the chain's detector: the oracle's CFAR, then the library's host
    Centroid and Interpolate.  row / col: the cell nearest to the record."""
    import blah2_amd
    noise, peak = O.map_metrics(m)
    rd, rf, rs = O.cfar1d_fast(m, dims.delay, dims.doppler, noise, det["pfa"], det["nGuard"], det["nTrain"], det["minDelay"],
                               det["minDoppler"])
    d = blah2_amd.Detection(np.asarray(rd, dtype=np.float64), np.asarray(rf, dtype=np.float64), np.asarray(rs, dtype=np.float64))
    d = blah2_amd.Centroid(det["nCentroid"], det["nCentroid"], 1 / (dims.n_samples / dims.fs)).process(d)
    mp = types.SimpleNamespace(data=np.asarray(m, dtype=np.complex64), delay=dims.delay, doppler=dims.doppler, noisePower=noise)
    d = blah2_amd.Interpolate(True, True).process(d, mp)
    out = np.zeros(d.get_nDetections(), dtype=blah2_amd.DET_DTYPE)
    out["delay"], out["doppler"], out["snr"] = d.get_delay(), d.get_doppler(), d.get_snr()
    out["row"] = [int(np.argmin(np.abs(np.asarray(dims.doppler) - f))) for f in out["doppler"]]
    out["col"] = np.rint(out["delay"]).astype(np.int64) - int(dims.delay[0])
    return out


def chain(x, y, amb_args=AMB_ARGS, det=DET, clean=CLEAN):
    """The restatement of the replay chain with ``clean``: pass 1, atoms, fit, subtract, pass 2, merge.  Returns a dict
    with both maps, both lists, the atoms, the amplitudes and the merged list."""
    import blah2_amd
    dims = O.ambiguity_dims(*amb_args)
    m1 = O.ambiguity_process(dims, x, y)
    first = detect(dims, m1, det)
    atoms, used = blah2_amd.clean_atoms(first, len(first), clean["snr"], clean["echoes"], clean["sideDelay"], clean["sideDoppler"],
                                        amb_args[0], amb_args[1], dims.cpi)
    a, ok, G, b = blah2_amd.clean_fit(x, y, atoms, dims.fs, clean["loading"])
    y2 = blah2_amd.clean_subtract(x, y, atoms, a, dims.fs) if ok else np.asarray(y, dtype=np.complex128)
    m2 = O.ambiguity_process(dims, x, y2)
    second = detect(dims, m2, det)
    merged = blah2_amd.merge_clean_detections(first, used if ok else [], second, clean["sideDelay"], dims.cpi)
    return dict(dims=dims, m1=m1, m2=m2, first=first, second=second, atoms=atoms, used=used, a=a, ok=ok, G=G, y2=y2, merged=merged)


def near(recs, delay, doppler, d_tol=1.5, f_tol=1.5):
    """Whether a record lies within the tolerances of (delay, doppler)."""
    return bool(np.any((np.abs(recs["delay"] - delay) <= d_tol) & (np.abs(recs["doppler"] - doppler) <= f_tol)))
