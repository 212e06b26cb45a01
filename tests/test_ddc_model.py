"""The digital down-converter's fp64 restatements (blah2_amd.process.ddc_design / ddc_taps / ddc) and the host-only part of
the C ABI (blah2hip_ddc_design, the argument checks of blah2hip_ddc_create): no GPU.

  * ddc_design against the same expression written with np.sinc and np.kaiser, its sum, its symmetry, and the library's
    blah2hip_ddc_design against the twin;
  * ddc (the form the kernel runs: rounded taps, one phasor per output) against the definition's first form -- every
    input sample mixed in fp64, np.convolve with the fp64 taps, every D-th taken: relative difference under T 2^-24, the
    tap rounding (measured 1.5e-8 at T = 64, 2.4e-8 at T = 100);
  * a stream cut at multiples of D, cuts shorter than T - 1 among them, equals the uncut result exactly (measured 0.0);
  * the scene of ddc_scenes.py: carrier A's map peaks off the zero-Doppler rows at delay 6 / 40 Hz, carrier B's at
    delay 11 / -24 Hz; measured here 27.8 dB and 28.9 dB over the map's median cell, asserted at 20 dB;
  * the refusals that need no device.
"""
import ctypes as C
import math

import numpy as np
import pytest

import ddc_scenes as S


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    return blah2_amd


DESIGNS = [(4, 64, 0.8, 8.0), (10, 160, 0.8, 8.0), (1, 1, 1.0, 0.0), (3, 7, 0.5, 5.0), (64, 1024, 0.8, 8.0), (2, 2, 1.0, 2.0),
           (50, 800, 0.8, 8.0), (16, 15, 0.25, 12.0)]


@pytest.mark.parametrize("D, T, cutoff, beta", DESIGNS)
def test_design(b2, D, T, cutoff, beta):
    h = b2.ddc_design(D, T, cutoff, beta)
    t = np.arange(T)
    ref = np.sinc(2.0 * (cutoff / (2.0 * D)) * (t - (T - 1) / 2.0)) * np.kaiser(T, beta)
    ref = ref / math.fsum(ref)
    assert np.max(np.abs(h - ref)) <= 1e-12 * np.max(np.abs(h))
    assert abs(math.fsum(h) - 1.0) <= T * 2.0 ** -52
    assert np.array_equal(h, h[::-1])
    hc = np.full(T, np.nan)
    assert b2.load().blah2hip_ddc_design(D, T, cutoff, beta, C.c_void_p(hc.ctypes.data)) == 0
    assert np.max(np.abs(hc - h)) <= 1e-14 * np.max(np.abs(h))
    assert np.array_equal(hc, hc[::-1]) and abs(math.fsum(hc) - 1.0) <= T * 2.0 ** -52


def test_design_refusals(b2):
    L = b2.load()
    h = np.zeros(2048)
    p = C.c_void_p(h.ctypes.data)
    assert L.blah2hip_ddc_design(4, 64, 0.8, 8.0, None) == -1
    for D, T, c, b in [(0, 64, 0.8, 8.0), (65, 64, 0.8, 8.0), (4, 0, 0.8, 8.0), (4, 1025, 0.8, 8.0), (4, 64, 0.0, 8.0),
                       (4, 64, 1.0001, 8.0), (4, 64, -0.1, 8.0), (4, 64, float("nan"), 8.0), (4, 64, 0.8, -1.0),
                       (4, 64, 0.8, float("inf")), (4, 64, 0.8, float("nan"))]:
        assert L.blah2hip_ddc_design(D, T, c, b, p) == -1, (D, T, c, b)
    assert np.all(h == 0.0)
    for args in [(0, 64), (65, 64), (4, 0), (4, 1025), (4, 64, 0.0), (4, 64, 1.5), (4, 64, 0.8, -1.0), (4, 64, 0.8, float("nan"))]:
        with pytest.raises(ValueError):
            b2.ddc_design(*args)


def test_create_refusals_need_no_device(b2):
    """Every argument is checked before the device is looked for: ERR_INVALID (-1), never ERR_NO_DEVICE (-5)."""
    L = b2.load()
    h = b2.ddc_design(4, 64)
    off = np.array([1000.0, -2000.0])
    hp, op = C.c_void_p(h.ctypes.data), C.c_void_p(off.ctypes.data)
    out = C.c_void_p()
    good = dict(fs=65536.0, D=4, h=hp, T=64, off=op, C=2, max_in=4096, rows=1)

    def create(**kw):
        a = dict(good, **kw)
        return L.blah2hip_ddc_create(a["fs"], a["D"], a["h"], a["T"], a["off"], a["C"], a["max_in"], a["rows"], 0, C.byref(out))

    bad_h = h.copy()
    bad_h[5] = np.inf
    far = np.array([1000.0, 40000.0])
    nan_off = np.array([float("nan"), 0.0])
    for kw in [dict(fs=0.0), dict(fs=-1.0), dict(fs=float("nan")), dict(fs=float("inf")), dict(D=0), dict(D=65), dict(T=0),
               dict(T=1025), dict(h=None), dict(off=None), dict(C=0), dict(C=9), dict(max_in=0), dict(max_in=4098),
               dict(rows=0), dict(rows=65536), dict(h=C.c_void_p(bad_h.ctypes.data)), dict(off=C.c_void_p(far.ctypes.data)),
               dict(off=C.c_void_p(nan_off.ctypes.data))]:
        assert create(**kw) == -1, kw
        assert not out.value
    assert L.blah2hip_ddc_create(65536.0, 4, hp, 64, op, 2, 4096, 1, 0, None) == -1


@pytest.mark.parametrize("D, T, f", [(4, 64, 16384.0), (7, 100, -1234.567), (1, 9, 32768.0), (16, 1, 777.0)])
def test_ddc_equals_the_first_form(b2, D, T, f):
    fs = 65536.0
    rng = np.random.default_rng(3)
    n = 3000 * D
    u = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    h = b2.ddc_design(D, T)
    v, hist = b2.ddc(u, f, fs, D, h)
    nn = np.arange(n)
    mixed = u * np.exp(-2j * np.pi * ((f * nn / fs) % 1.0))
    full = np.convolve(mixed, h)[:n][::D]
    err = np.max(np.abs(v - full)) / np.max(np.abs(full))
    print(f"D {D} T {T}: relative difference {err:.3e}, bound {T * 2.0 ** -24:.3e}")
    assert err < T * 2.0 ** -24
    assert np.array_equal(hist, u[n - (T - 1):])
    # the taps: fp32 of ddc_taps; an override with the same values changes nothing
    g = b2.ddc_taps(h, f, fs).astype(np.complex64)
    v2, _ = b2.ddc(u, f, fs, D, None, g=g)
    assert np.array_equal(v, v2)


@pytest.mark.parametrize("D, T", [(4, 64), (7, 100), (3, 13)])
def test_split_streams_are_exact(b2, D, T):
    fs, f = 65536.0, 9876.54321
    rng = np.random.default_rng(4)
    n = 600 * D
    u = np.stack([rng.standard_normal(n) + 1j * rng.standard_normal(n) for _ in range(2)])
    h = b2.ddc_design(D, T)
    first = 5 * D
    v, hist, Sv = b2.ddc(u, f, fs, D, h, first_sample=first, detail=True)
    assert v.shape == (2, n // D) and Sv.shape == v.shape
    cuts = [D, 2 * D, D * ((T - 2) // D), D * ((T - 1 + D - 1) // D), 299 * D, n - D]
    for cut in [c for c in cuts if 0 < c < n]:
        v1, h1 = b2.ddc(u[:, :cut], f, fs, D, h, first_sample=first)
        v2, h2 = b2.ddc(u[:, cut:], f, fs, D, h, first_sample=first + cut, history=h1)
        assert np.array_equal(np.concatenate([v1, v2], axis=-1), v), cut
        assert np.array_equal(h2, hist), cut
    # ... and piece by piece, every piece shorter than the history
    pieces, hh, pos = [], None, first
    for s in range(0, n, D):
        vv, hh = b2.ddc(u[:, s:s + D], f, fs, D, h, first_sample=pos, history=hh)
        pieces.append(vv)
        pos += D
    assert np.array_equal(np.concatenate(pieces, axis=-1), v)
    with pytest.raises(ValueError):
        b2.ddc(u[:, :D + 1], f, fs, D, h)
    with pytest.raises(ValueError):
        b2.ddc(u[:, :D], f, fs, D, h, first_sample=1) if D > 1 else b2.ddc(u[:, :D], f, fs, D, h, history=np.zeros((2, T)))


def test_phasor_at_large_indices(b2):
    """The phasor comes from the exact product r m: at m = 2^40 it equals what rational arithmetic gives."""
    from fractions import Fraction
    D, T, fs, f = 4, 3, 65536.0, 1234.5678901
    h = b2.ddc_design(D, T)
    u = np.zeros(8 * D, dtype=np.complex128)
    u[::D] = 1.0  # one sample under tap 0 per output
    first = (2 ** 40) * D
    v, _ = b2.ddc(u, f, fs, D, h, first_sample=first)
    g0 = complex(b2.ddc_taps(h, f, fs).astype(np.complex64)[0])
    r = Fraction(f * D / fs)
    for k in range(8):
        fr = float((r * (2 ** 40 + k)) % 1)
        assert abs(v[k] - g0 * np.exp(-2j * np.pi * fr)) <= 1e-15 * abs(g0) * 4


def test_scene_peaks(b2):
    x, y = S.scene()
    measured = (27.8, 28.9)  # dB over the median, measured on this scene; asserted at 20 dB
    for f, want, db in zip(S.CARRIERS, S.PEAKS, measured):
        dims, m = S.oracle_map(S.model_planes(x, y, f))
        assert m.shape == (129, 25)
        (delay, dop), over = S.peak_off_zero(m, dims)
        print(f"carrier {f}: peak at delay {delay}, {dop:.3f} Hz, {over:.1f} dB over the median (measured {db})")
        assert delay == want[0] and abs(dop - want[1]) < 0.5
        assert over >= 20.0  # (7.8 dB and 8.9 dB below the measured figures)
