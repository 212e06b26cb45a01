"""CPU: the Doppler taper's host side -- the named windows, their taps in the library and in process.py, the identity
"window on the pulses = circular stencil on the map" through the unmodified oracle, the gains, the masking scene the GPU
module repeats, and the refusals.  No GPU is touched.

  * presets: ``doppler_window`` against ``scipy.signal.get_window(name, n, fftbins=True)`` to 1e-14;
  * ``blah2hip_doppler_taper`` gives the fp32 roundings of ``doppler_taper``, for both values of ``normalise``;
  * identity: the range correlation is linear in the surveillance channel, so the oracle on ``y w[pulse of the sample]``
    is the windowed map; ``taper_maps`` of the oracle's unwindowed map equals it to 1e-12 of the peak (odd nD, and the
    explicit even bin count);
  * the masking scene (tests/taper_scenes.py): at least 80 strays without a taper, none with Blackman, the weak echo
    detected in both, for seeds 7, 8, 9.
"""
import ctypes as C

import numpy as np
import pytest

import taper_scenes as TS
from oracle import blah2_oracle as O


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    return blah2_amd


@pytest.mark.parametrize("name", TS.PRESETS)
def test_presets_are_scipys_periodic_windows(b2, name):
    from scipy.signal import get_window
    worst = 0.0
    for n in (9, 21, 512, 513):
        worst = max(worst, float(np.abs(b2.doppler_window(name, n) - get_window(name, n, fftbins=True)).max()))
    print(f"{name}: largest distance from scipy's window {worst:.2e}")
    assert worst <= 1e-14
    assert np.array_equal(b2.doppler_window("none", 9), np.ones(9))


@pytest.mark.parametrize("normalise", [False, True])
def test_library_taps_are_the_fp32_roundings(b2, normalise):
    from blah2_amd import _lib
    L = _lib.load()
    for name in ("none",) + TS.PRESETS:
        want = b2.doppler_taper(name, normalise)
        assert want.dtype == np.float64
        taps = np.full(_lib.MAX_TAPER_SIDE + 1, np.nan, dtype=np.float32)
        n_side = C.c_uint32(99)
        assert L.blah2hip_doppler_taper(_lib.TAPER_KINDS[name], int(normalise), taps.ctypes.data_as(C.c_void_p), C.byref(n_side)) == _lib.OK
        P = n_side.value
        assert P == want.size - 1 <= _lib.MAX_TAPER_SIDE
        assert np.array_equal(taps[:P + 1], want.astype(np.float32)) and (taps[P + 1:] == 0).all()
        assert np.array_equal(b2.doppler_taper_f32(name, normalise), want.astype(np.float32))
        if normalise:
            assert want[0] == 1.0
        # the stencil's sum is the window at pulse 0: a cosine-sum window starts at sum_p (-1)^p a_p
        a0 = b2.doppler_taper(name)[0] if normalise else 1.0
        assert abs(want[0] + 2 * want[1:].sum() - b2.doppler_window(name, 64)[0] / a0) < 1e-15
    assert b2.doppler_taper("none").tolist() == [1.0]


@pytest.mark.parametrize("geom", ["odd", "even16"])
def test_identity_through_the_oracle(b2, geom):
    limits, bins = TS.GEOMS[geom]
    dims = O.ambiguity_dims(*limits, True, bins)
    nD = dims.n_doppler_bins
    assert (nD, dims.n_delay_bins) == TS.SHAPES[geom]
    rng = np.random.default_rng(31 + nD)
    n = limits[5]
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    y = 0.3 * np.roll(x, 7) * np.exp(2j * np.pi * 23.0 * np.arange(n) / limits[4]) + rng.standard_normal(n) + 1j * rng.standard_normal(n)
    plain = O.ambiguity_process(dims, x, y)
    pulse = np.minimum(np.arange(n) // dims.n_corr, nD - 1)  # (samples behind the last pulse are not used)
    peak = np.abs(plain).max()
    for name in TS.PRESETS:
        taps = b2.doppler_taper(name)
        if nD < 2 * taps.size - 1:
            continue
        windowed = O.ambiguity_process(dims, x, y * b2.doppler_window(name, nD)[pulse])
        err = float(np.abs(b2.taper_maps(plain, taps) - windowed).max() / peak)
        print(f"{geom} {name}: stencil on the map against window on the pulses, {err:.2e} of the peak")
        assert err <= 1e-12
    # the normalised taps: the same map over a_0
    t = b2.doppler_taper("blackman")
    assert np.allclose(b2.taper_maps(plain, b2.doppler_taper("blackman", True)) * t[0], b2.taper_maps(plain, t), rtol=1e-14, atol=0)


def test_stencil_restatement(b2):
    """taper_maps against the definition, cell by cell, with the wrap at both ends; real and complex input; batches."""
    rng = np.random.default_rng(5)
    m = rng.standard_normal((3, 9, 4)) + 1j * rng.standard_normal((3, 9, 4))
    t = np.array([0.5, -0.2, 0.07, -0.01, 0.003])
    out = b2.taper_maps(m, t)
    for j in range(9):
        want = t[0] * m[:, j]
        for k in range(1, 5):
            want = want + t[k] * (m[:, (j - k) % 9] + m[:, (j + k) % 9])
        assert np.allclose(out[:, j], want, rtol=1e-14, atol=1e-15)
    assert np.array_equal(b2.taper_maps(m, [1.0]), m)
    assert b2.taper_maps(np.ones((5, 2)), [0.5, 0.25]).dtype == np.float64
    one = np.zeros((7, 1))
    one[0, 0] = 1.0
    assert np.array_equal(b2.taper_maps(one, [0.5, -0.25])[:, 0], [0.5, -0.25, 0, 0, 0, 0, -0.25])


def test_gains(b2):
    c, n, enbw, loss = b2.taper_gains(b2.doppler_taper("hamming"))
    assert c == 0.54 and abs(n - (0.54 ** 2 + 2 * 0.23 ** 2)) < 1e-15
    assert abs(enbw - 1.363) < 5e-4 and abs(loss - 1.34) < 5e-3
    c, n, enbw, loss = b2.taper_gains(b2.doppler_taper("blackman"))
    assert c == 0.42 and abs(enbw - 1.727) < 5e-4 and abs(loss - 2.37) < 5e-3
    assert b2.taper_gains(b2.doppler_taper("none")) == (1.0, 1.0, 1.0, 0.0)
    assert abs(b2.taper_gains(b2.doppler_taper("hann"))[2] - 1.5) < 1e-15
    # the ratios do not move with the normalisation; the gains are those of the window: mean(w) and mean(w^2)
    for name in TS.PRESETS:
        g, gn = b2.taper_gains(b2.doppler_taper(name)), b2.taper_gains(b2.doppler_taper(name, True))
        assert gn[0] == 1.0 and abs(g[2] - gn[2]) < 1e-14 and abs(g[3] - gn[3]) < 1e-13
        w = b2.doppler_window(name, 64)
        assert abs(g[0] - w.mean()) < 1e-15 and abs(g[1] - (w * w).mean()) < 1e-15


@pytest.mark.parametrize("seed", TS.SCENE_SEEDS)
def test_masking_scene(b2, seed):
    m = TS.scene_map(seed)
    strays, weak = TS.scene_detect(m)
    tapered = b2.taper_maps(m, b2.doppler_taper("blackman"))
    strays_b, weak_b = TS.scene_detect(tapered)
    print(f"seed {seed}: strays without a taper {strays}, with Blackman {strays_b}; weak echo {weak} / {weak_b}")
    assert strays >= 80 and weak
    assert strays_b == 0 and weak_b


def test_refusals(b2):
    from blah2_amd import _lib
    L = _lib.load()
    taps = np.zeros(_lib.MAX_TAPER_SIDE + 1, dtype=np.float32)
    n_side = C.c_uint32(0)
    p = taps.ctypes.data_as(C.c_void_p)
    for kind in (-1, 7, 100):
        assert L.blah2hip_doppler_taper(kind, 0, p, C.byref(n_side)) == _lib.ERR_INVALID
    assert b"window" in L.blah2hip_last_error()
    assert L.blah2hip_doppler_taper(_lib.TAPER_HANN, 0, None, C.byref(n_side)) == _lib.ERR_INVALID
    assert L.blah2hip_doppler_taper(_lib.TAPER_HANN, 0, p, None) == _lib.ERR_INVALID
    assert sorted(_lib.TAPER_KINDS) == sorted(("none",) + TS.PRESETS)
    for f in (b2.doppler_taper, b2.doppler_taper_f32, lambda s: b2.doppler_window(s, 9)):
        with pytest.raises(ValueError):
            f("taylor")
    with pytest.raises(ValueError):
        b2.taper_maps(np.ones((8, 3)), b2.doppler_taper("flattop"))  # nD < 2P + 1
    with pytest.raises(ValueError):
        b2.taper_maps(np.ones((8, 3)), [])
    assert b2.taper_maps(np.ones((9, 3)), b2.doppler_taper("flattop")).shape == (9, 3)
