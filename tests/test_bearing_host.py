"""CPU: the bearing estimator in NumPy -- blah2_amd.bearing (what blah2hip_amb_bearing_dev computes, restated in fp64),
bearing_degrees and uca_steering.  No GPU, no library call.

The figures test_the_scene prints, fp64 on the -88 .. 88 degree grid (the -90 .. 90 grid gave -23.98, +19.88, 20.07 and
20.06 degrees): Bartlett on the shared cell -23.982, adaptive on it +19.877, Bartlett / adaptive on the clean target cell
+20.066 / +20.065 degrees.
"""
import numpy as np
import pytest

import adaptive_crafted as A
import bearing_crafted as B
from blah2_amd import BEARING_DTYPE, bearing, bearing_degrees, uca_steering, ula_steering


def plane_wave(n_surv, deg, amp=3.0 - 2.0j):
    return amp * ula_steering(n_surv, A.SPACING, [deg])[0]


def independent(snap, steer, R, loading, wrap):
    """cholesky and solve of numpy.linalg, a plain argmax, the same parabola."""
    P, tt = B.powers(snap, steer, R, loading)
    G = P.shape[1]
    out = []
    for i in range(P.shape[0]):
        g = int(np.argmax(P[i]))
        off = 0.0
        if wrap or 0 < g < G - 1:
            pm, p0, pp = P[i, (g - 1) % G], P[i, g], P[i, (g + 1) % G]
            den = pm - 2.0 * p0 + pp
            if den < 0:
                off = 0.5 * (pm - pp) / den
        out.append((g, off, P[i, g], P[i, g] / tt[i]))
    return out


@pytest.mark.parametrize("K", [2, 3, 4, 8])
def test_restatement_against_numpy_linalg(K):
    rng = np.random.default_rng(100 + K)
    maps = B.scene_k(K, 1, seed=200 + K)
    R = A.covariance64(maps)[0]
    cells = [(int(r), int(q)) for r, q in zip(rng.integers(0, A.ND, 40), rng.integers(0, A.NC, 40))] + list(B.CELLS)
    snap = B.snapshots(maps, 0, cells)
    # (two elements on a circle are a line: the azimuths theta and -theta tie exactly, so no circular grid for K = 2)
    for steer, wrap in ((B.ula_table(K), False), (B.uca_table(K), True))[:1 if K == 2 else 2]:
        for Rm, loading in ((None, 0.0), (R, 1e-3), (R, 0.3)):
            idx, off, power, coh, adaptive = bearing(snap, steer, Rm, loading, wrap)
            assert (adaptive == (0 if Rm is None else 1)).all()
            assert (B.top_two_gap(snap, steer, Rm, loading) > 1e-9).all()
            cond = 1.0 if Rm is None else np.linalg.cond(Rm + loading * (np.trace(Rm).real / K) * np.eye(K))
            for i, (g, o, p, c) in enumerate(independent(snap, steer, Rm, loading, wrap)):
                assert idx[i] == g
                # two fp64 solutions of systems of this condition, K terms each; the offset is a ratio of differences
                assert abs(power[i] - p) <= 1e-13 * cond * p and abs(coh[i] - c) <= 1e-13 * cond
                assert abs(off[i] - o) <= 1e-9 * cond
                assert 0.0 <= coh[i] <= 1.0 + 1e-12 and abs(off[i]) <= 0.5 + 1e-12


@pytest.mark.parametrize("K", [2, 4, 8])
def test_a_plane_wave_on_the_grid(K):
    """The parabola's vertex is the peak where the two neighbours are equally far from it in the array's own coordinate,
    sin(theta) for a line array: on a grid uniform in sin(theta) the powers at g - 1 and g + 1 are equal up to rounding.
    (On the grid in degrees that holds at broadside only -- away from it a step towards endfire is a shorter step in
    sin(theta), and the vertex leans that way: 0.015 of a step at -60 degrees, 0.16 at 87 degrees.)"""
    u = np.linspace(-0.99, 0.99, 177)
    steer = np.exp(2j * np.pi * A.SPACING * u[:, None] * np.arange(K)[None, :])  # fp64: the snapshot is a table row exactly
    for g in (1, 20, 88, 131, 175):
        idx, off, power, coh, adaptive = bearing((3.0 - 2.0j) * steer[g], steer)
        assert idx == g and adaptive == 0
        assert abs(off) <= 1e-9 and abs(coh - 1.0) <= 1e-12
        assert abs(power - 13.0 * K) <= 1e-12 * 13.0 * K
    steer = ula_steering(K, A.SPACING, B.ULA_DEG)
    idx, off, power, coh, _ = bearing(plane_wave(K, 0.0), steer)
    assert B.ULA_DEG[idx] == 0.0 and abs(off) <= 1e-9 and abs(coh - 1.0) <= 1e-12
    assert abs(bearing_degrees(idx, off, B.ULA_DEG)) <= 1e-9
    for deg in (-60.0, -1.0, 33.0, 87.0):  # the index and the coherence hold on any grid the source lies on
        idx, off, power, coh, _ = bearing(plane_wave(K, deg), steer)
        assert B.ULA_DEG[idx] == deg and abs(coh - 1.0) <= 1e-12


def test_a_plane_wave_between_grid_points():
    steer = ula_steering(4, A.SPACING, B.ULA_DEG)
    for deg in (-40.5, -0.5, 10.5, 20.5, 59.5):
        idx, off, _, coh, _ = bearing(plane_wave(4, deg), steer)
        where = idx + off - (deg - B.ULA_DEG[0])
        print(f"plane wave from {deg}: index {idx} offset {off:+.4f}, {where:+.4f} of a step off, coherence {coh:.6f}")
        assert abs(where) <= 0.05


def test_the_scene():
    """Where the Bartlett scan reads the interferer the adaptive scan reads the target."""
    maps = B.scene()
    ref = A.scene()
    other = np.ones((A.ND, A.NC), dtype=bool)
    other[B.SHARED_CELL] = False
    assert np.array_equal(maps[:, 0][:, other], ref[:, 0][:, other])
    R = A.covariance64(maps)[0]
    steer = B.ula_table()
    snap = B.snapshots(maps, 0, [B.SHARED_CELL, A.TARGET_CELL])
    bi, bo, _, _, ba = bearing(snap, steer)
    ai, ao, _, _, aa = bearing(snap, steer, R, B.LOADING)
    bart, adap = bearing_degrees(bi, bo, B.ULA_DEG), bearing_degrees(ai, ao, B.ULA_DEG)
    print(f"shared cell {B.SHARED_CELL}: Bartlett {bart[0]:+.3f} deg, adaptive {adap[0]:+.3f} deg; "
          f"target cell {A.TARGET_CELL}: Bartlett {bart[1]:+.3f} deg, adaptive {adap[1]:+.3f} deg")
    assert ba.tolist() == [0, 0] and aa.tolist() == [1, 1]
    assert abs(bart[0] - A.INTERFERER_DEG) <= 0.5
    assert abs(adap[0] - A.TARGET_DEG) <= 0.5
    assert abs(bart[1] - A.TARGET_DEG) <= 0.5 and abs(adap[1] - A.TARGET_DEG) <= 0.5


def test_degenerate_inputs():
    steer = B.ula_table()
    maps = B.scene()
    R = A.covariance64(maps)[0]
    snap = B.snapshots(maps, 0, B.CELLS)
    assert bearing(np.zeros(4), steer) == (-1, 0.0, 0.0, 0.0, 0)
    assert bearing(np.zeros(4), steer, R, 1e-3) == (-1, 0.0, 0.0, 0.0, 0)
    for bad in (np.nan, np.inf, complex(0.0, np.nan)):
        s = snap[0].copy()
        s[2] = bad
        assert bearing(s, steer) == (-1, 0.0, 0.0, 0.0, 0)
        assert bearing(s, steer, R, 1e-3) == (-1, 0.0, 0.0, 0.0, 0)
    # in a batch only the bad rows are marked
    batch = snap.copy()
    batch[1] = 0
    idx, off, power, coh, adaptive = bearing(batch, steer, R, 1e-3)
    assert idx[1] == -1 and adaptive.tolist() == [1, 0, 1] and power[1] == 0 and idx[0] >= 0 and idx[2] >= 0
    # a covariance that cannot be factorised: the Bartlett values, adaptive 0
    want = bearing(snap, steer)
    nan_R = R.copy()
    nan_R[2, 1] = np.nan
    for Rm in (np.zeros((4, 4)), nan_R):
        got = bearing(snap, steer, Rm, 1e-3)
        assert got[4].tolist() == [0, 0, 0]
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    # ... and an identity covariance gives them too, marked adaptive
    got = bearing(snap, steer, np.eye(4), 0.0)
    assert got[4].tolist() == [1, 1, 1]
    for g, w in zip(got[:4], want[:4]):
        assert np.array_equal(g, w)


def test_the_ends_of_the_grid():
    steer = uca_steering(4, B.UCA_RADIUS, B.UCA_DEG)
    # 0.4 and 359.6 degrees peak at index 0 from either side of the seam, 359.4 degrees at index 359
    for deg, end in ((0.4, 0), (359.6, 0), (359.4, 359)):
        s = (1.0 + 2.0j) * uca_steering(4, B.UCA_RADIUS, [deg])[0]
        idx, off, _, _, _ = bearing(s, steer, wrap=False)
        assert (idx, off) == (end, 0.0)
        idx, off, _, _, _ = bearing(s, steer, wrap=True)
        assert idx == end and off != 0.0
        got = bearing_degrees(idx, off, B.UCA_DEG, wrap=True)
        assert abs((got - deg + 180.0) % 360.0 - 180.0) <= 0.05
    # the line array's grid is open: a wave from beyond its end peaks there with offset 0
    steer = ula_steering(4, A.SPACING, np.arange(-30.0, 31.0))
    assert bearing(plane_wave(4, 40.0), steer)[:2] == (60, 0.0)
    assert bearing(plane_wave(4, -40.0), steer)[:2] == (0, 0.0)


def test_an_exact_tie_takes_the_lowest_index():
    steer = ula_steering(4, A.SPACING, np.arange(-30.0, 31.0))
    steer[40] = steer[12]
    steer[55] = steer[12]
    idx, off, _, coh, _ = bearing(plane_wave(4, -18.0), steer)
    assert idx == 12 and abs(coh - 1.0) <= 1e-12
    # a snapshot every table row sees alike (one element only): all of P ties, index 0, a flat parabola, offset 0
    assert bearing(np.array([1.0, 0, 0, 0]), steer)[:2] == (0, 0.0)


def test_bearing_degrees():
    assert bearing_degrees(3, 0.25, B.ULA_DEG) == -84.75
    assert bearing_degrees(359, 0.4, B.UCA_DEG, wrap=True) == pytest.approx(359.4)
    assert bearing_degrees(359, 0.6, B.UCA_DEG, wrap=True) == pytest.approx(359.6)
    assert bearing_degrees(0, -0.4, B.UCA_DEG, wrap=True) == pytest.approx(359.6)
    assert bearing_degrees(0, -0.4, B.UCA_DEG, wrap=False) == pytest.approx(-0.4)
    assert np.isnan(bearing_degrees(-1, 0.0, B.ULA_DEG))
    got = bearing_degrees(np.array([0, -1, 176]), np.array([0.5, 0.0, 0.0]), B.ULA_DEG)
    assert got[0] == -87.5 and np.isnan(got[1]) and got[2] == 88.0
    # a 2 degree grid
    assert bearing_degrees(10, -0.5, np.arange(0.0, 360.0, 2.0), wrap=True) == 19.0


def test_uca_steering():
    n, r = 5, 0.4
    angles = [0.0, 17.0, 123.0, 359.0]
    a = uca_steering(n, r, angles)
    assert a.shape == (4, 5) and a.dtype == np.complex128
    for g, deg in enumerate(angles):
        for k in range(n):
            want = np.exp(2j * np.pi * r * np.cos(np.deg2rad(deg) - 2.0 * np.pi * k / n))
            assert abs(a[g, k] - want) <= 1e-15
    assert np.allclose(np.abs(a), 1.0, rtol=0, atol=1e-15)


def test_the_record_dtype_is_the_struct():
    assert BEARING_DTYPE.itemsize == 32
    assert [BEARING_DTYPE.fields[n][1] for n in ("index", "adaptive", "offset", "power", "coherence")] == [0, 4, 8, 16, 24]
    from blah2_amd import _lib
    import ctypes as C
    assert C.sizeof(_lib.Bearing) == 32 and _lib.Bearing.offset.offset == 8 and _lib.Bearing.coherence.offset == 24
