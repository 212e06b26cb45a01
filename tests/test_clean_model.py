"""Strong-echo cancellation, the fp64 restatements (blah2_amd.process.clean_*): no GPU.

  * a noiseless y = S a gives the amplitudes back to 1e-10 relative and a residual at rounding level;
  * sign and axes: a lone atom's replica peaks in the oracle's map at its (delay, doppler) cell, also with
    doppler_middle != 0 and for a negative delay;
  * the demonstration scene (clean_scenes.py).  With the atoms at the strong echo's true Doppler, measured here: one atom at
    delay 20 drops the floor 14.9 dB (weak cell 12.3 dB over it), three atoms at 19, 20, 21 (cond G = 4.4e2) 25.8 dB (25.4 dB
    over), five atoms (cond 2.0e5) gain nothing more.  Through the whole chain, with the atoms from the interpolated
    detection: the weak echo is missing from the pass-1 list and present in the merged one, and sideDelay = 0 recovers at
    least 8 dB less floor than sideDelay = 1;
  * duplicate atoms: ok = 0 and y unchanged without loading, ok = 1 with loading 1e-6;
  * clean_atoms: ordering, ties, snr_min, clusters clipped at the delay range, a cluster that does not fit dropped whole.
"""
import numpy as np
import pytest

import clean_scenes as S
from oracle import blah2_oracle as O


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    return blah2_amd


@pytest.fixture(scope="module")
def scene():
    return S.demo_scene()


def test_noiseless_fit_recovers_the_amplitudes(b2):
    rng = np.random.default_rng(1)
    x = S.band_limited(rng, 4096)
    atoms = [(-3, 11.0), (5, -40.5), (6, -40.5), (17, 3.25)]
    a0 = rng.standard_normal(4) + 1j * rng.standard_normal(4)
    Sm = b2.clean_replicas(x, atoms, 4096.0)
    y = a0 @ Sm
    a, ok, G, b = b2.clean_fit(x, y, atoms, 4096.0, 0.0)
    assert ok == 1
    assert np.linalg.norm(a - a0) <= 1e-10 * np.linalg.norm(a0)
    r = b2.clean_subtract(x, y, atoms, a, 4096.0)
    assert np.max(np.abs(r)) <= 1e-10 * np.max(np.abs(y))
    assert np.array_equal(G, np.conj(G.T))
    # no atoms: ok = 1 and y comes back
    a, ok, G, b = b2.clean_fit(x, y, [], 4096.0, 0.0)
    assert ok == 1 and a.size == 0 and np.array_equal(b2.clean_subtract(x, y, [], a, 4096.0), y)


@pytest.mark.parametrize("args, atom", [((-10, 40, -32, 32, 8192, 8192), (13, 7.0)),
                                        ((-10, 40, -32, 32, 8192, 8192), (-6, -19.0)),
                                        ((-10, 40, 10, 50, 8192, 8192), (22, 41.0)),
                                        ((-10, 40, -50, -10, 8192, 8192), (-4, -33.0))])
def test_a_lone_atom_peaks_at_its_cell(b2, args, atom):
    dims = O.ambiguity_dims(*args)
    rng = np.random.default_rng(2)
    x = S.band_limited(rng, args[5])
    i0 = int(np.argmin(np.abs(dims.doppler - atom[1])))  # the axis value next to the nominal Doppler: on a bin
    atom = (atom[0], float(dims.doppler[i0]))
    y = b2.clean_replicas(x, [atom], float(args[4]))[0]
    for m in (O.ambiguity_process(dims, x, y),
              np.fft.fft(b2.range_map(dims, x, y), axis=0)[(np.arange(dims.n_doppler_bins) + dims.n_doppler_bins // 2 + 1) % dims.n_doppler_bins]):
        i, j = np.unravel_index(np.argmax(np.abs(m)), m.shape)
        assert (int(dims.delay[j]), int(i)) == (atom[0], i0)


def test_demonstration_scene_with_the_true_doppler(b2, scene):
    x, y = scene
    dims = O.ambiguity_dims(*S.AMB_ARGS)
    m1 = O.ambiguity_process(dims, x, y)
    f1 = S.floor_db(m1, dims)
    assert S.cell_db(m1, dims, S.WEAK[1], S.WEAK[2]) - f1 < 6.0  # buried
    got = {}
    for name, delays in (("one", (20,)), ("three", (19, 20, 21)), ("five", (18, 19, 20, 21, 22))):
        atoms = [(d, S.STRONG[2]) for d in delays]
        a, ok, G, b = b2.clean_fit(x, y, atoms, S.FS, 0.0)
        assert ok == 1
        m2 = O.ambiguity_process(dims, x, b2.clean_subtract(x, y, atoms, a, S.FS))
        f2 = S.floor_db(m2, dims)
        got[name] = (np.linalg.cond(G), f1 - f2, S.cell_db(m2, dims, S.WEAK[1], S.WEAK[2]) - f2)
    print({k: tuple(round(float(v), 2) for v in g) for k, g in got.items()})
    assert got["one"][0] < 1.0 + 1e-9 and 10.0 < got["one"][1] < 18.0
    assert 1e2 < got["three"][0] < 1e3 and got["three"][1] > 23.0 and got["three"][2] > 22.0
    assert got["three"][1] - got["one"][1] > 8.0
    assert got["five"][0] > 1e4 and abs(got["five"][1] - got["three"][1]) < 1.0  # clusters wider than the echo buy nothing


def test_demonstration_scene_through_the_chain(b2, scene):
    x, y = scene
    r1 = S.chain(x, y)
    dims = r1["dims"]
    assert r1["ok"] == 1 and len(r1["used"]) == 1 and len(r1["atoms"]) == 9
    assert S.near(r1["first"], S.STRONG[1], S.STRONG[2]) and not S.near(r1["first"], S.WEAK[1], S.WEAK[2])
    assert S.near(r1["merged"], S.WEAK[1], S.WEAK[2]) and S.near(r1["merged"], S.STRONG[1], S.STRONG[2])
    # the cancelled echo is reported once, from pass 1: what pass 2 finds at its cell is its residual
    g = r1["first"][r1["used"][0]]
    m = r1["merged"]
    assert np.sum((np.abs(m["delay"] - g["delay"]) <= 2) & (np.abs(m["doppler"] - g["doppler"]) <= 1 / dims.cpi)) == 1
    drop1 = S.floor_db(r1["m1"], dims) - S.floor_db(r1["m2"], dims)
    r0 = S.chain(x, y, clean=dict(S.CLEAN, sideDelay=0))
    drop0 = S.floor_db(r0["m1"], dims) - S.floor_db(r0["m2"], dims)
    print(f"floor drop: sideDelay 1 {drop1:.1f} dB, sideDelay 0 {drop0:.1f} dB; weak cell over the floor "
          f"{S.cell_db(r1['m2'], dims, S.WEAK[1], S.WEAK[2]) - S.floor_db(r1['m2'], dims):.1f} dB")
    assert drop1 > 20.0 and drop1 - drop0 >= 8.0


def test_duplicate_atoms_need_loading(b2):
    rng = np.random.default_rng(3)
    x = S.band_limited(rng, 2048)
    y = (rng.standard_normal(2048) + 1j * rng.standard_normal(2048)) + 3 * b2.clean_replicas(x, [(4, 10.0)], 2048.0)[0]
    atoms = [(4, 10.0), (4, 10.0)]
    a, ok, G, b = b2.clean_fit(x, y, atoms, 2048.0, 0.0)
    assert ok == 0 and not a.any()
    assert np.array_equal(b2.clean_subtract(x, y, atoms, a, 2048.0), y)
    a, ok, G, b = b2.clean_fit(x, y, atoms, 2048.0, 1e-6)
    assert ok == 1 and abs(a.sum() - 3) < 0.2
    a, ok, G, b = b2.clean_fit(x, y, [(4, float("nan"))], 2048.0, 1e-6)
    assert ok == 0


def _dets(b2, rows):
    d = np.zeros(len(rows), dtype=b2.DET_DTYPE)
    for k, r in enumerate(rows):
        d[k] = r
    return d


def test_clean_atoms_rules(b2):
    cpi = 0.5
    d = _dets(b2, [(5, 9, 9.2, 3.0, 20.0), (2, 4, 3.6, -7.0, 30.0), (2, 3, 3.4, -7.5, 30.0), (1, 1, 0.0, 1.0, 9.0), (7, 7, 49.6, 2.0, 25.0)])
    # strongest first, ties by row, then col; snr_min drops record 3; rint; order echo, i, j
    at, used = b2.clean_atoms(d, len(d), 10.0, 8, 1, 0, -10, 60, cpi)
    assert used.tolist() == [2, 1, 4, 0]
    assert at["delay"].tolist() == [2, 3, 4, 3, 4, 5, 49, 50, 51, 8, 9, 10]
    assert at["doppler"][:3].tolist() == [-7.5] * 3
    at, used = b2.clean_atoms(d, len(d), 10.0, 2, 0, 1, -10, 60, cpi)
    assert used.tolist() == [2, 1] and at["delay"].tolist() == [3, 3, 3, 4, 4, 4]
    assert at["doppler"][:3].tolist() == [-7.5 - 1.0, -7.5, -7.5 + 1.0]
    # count below the list's length cuts it; a shuffled list gives the same atoms
    at_c, used_c = b2.clean_atoms(d, 2, 10.0, 8, 0, 0, -10, 60, cpi)
    assert used_c.tolist() == [1, 0]
    p = np.array([4, 2, 0, 3, 1])
    at_s, used_s = b2.clean_atoms(d[p], len(d), 10.0, 8, 1, 0, -10, 60, cpi)
    assert np.array_equal(at_s, b2.clean_atoms(d, len(d), 10.0, 8, 1, 0, -10, 60, cpi)[0]) and p[used_s].tolist() == [2, 1, 4, 0]
    # clipped at the delay range: record 4 (delay 50) keeps 49, 50 of its cluster at delay_hi = 50; record 0 keeps 10 at delay_lo = 10
    at, used = b2.clean_atoms(d, len(d), 24.0, 8, 1, 0, -10, 50, cpi)
    assert used.tolist() == [2, 1, 4] and at["delay"].tolist()[-2:] == [49, 50]
    at, used = b2.clean_atoms(d, len(d), 10.0, 8, 1, 0, 10, 60, cpi)
    assert used.tolist() == [4, 0] and at["delay"].tolist() == [49, 50, 51, 10]
    # a cluster that does not fit is dropped whole, a later smaller one still goes in
    at, used = b2.clean_atoms(d, len(d), 10.0, 8, 1, 0, -10, 50, cpi, cap_atoms=8)
    assert used.tolist() == [2, 1, 4] and len(at) == 8
    at, used = b2.clean_atoms(d, len(d), 10.0, 8, 1, 0, -10, 50, cpi, cap_atoms=7)
    assert used.tolist() == [2, 1] and len(at) == 6


def test_merge_rule(b2):
    first = _dets(b2, [(0, 0, 20.4, 37.1, 19.0), (0, 0, 60.0, 5.0, 12.0)])
    second = _dets(b2, [(0, 0, 20.6, 38.0, 15.0), (0, 0, 22.4, 37.0, 9.0), (0, 0, 22.5, 37.0, 9.0), (0, 0, 20.4, 38.2, 9.0), (0, 0, 55.0, -12.0, 12.0)])
    m = b2.merge_clean_detections(first, [0], second, 1, 1.0)
    assert m["delay"].tolist() == [20.4, 22.5, 20.4, 55.0] and m["snr"].tolist() == [19.0, 9.0, 9.0, 12.0]
    assert len(b2.merge_clean_detections(first, [], second, 1, 1.0)) == 5
