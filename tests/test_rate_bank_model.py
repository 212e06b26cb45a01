"""CPU: the Doppler-rate bank's definition restated in blah2_amd.process (doppler_rate, rate_bank, rate_chirps,
rate_bank_maps) on the scenes of tests/rate_scenes.py.  Needs no GPU and no library: tests/test_rate_bank_gpu.py holds the device
to these restatements.

  * rate_bank_maps against a per-cell Python loop of the definition, with and without a walk; bank {0} equals migrate_maps;
    doppler_rate's signs and values; rate_bank; rate_chirps: the entry for q = 0 is exactly 1, every table is even about mid-CPI.
  * The variant table on the impulse-reference CPIs (g65x44 with walk 4, g2049x40 with walk 15 on a spread of rows) at q = 0.5 and
    3: an fp32 emulation of the kernel's sum with the fp32 chirp table stays under PEAK_TOL / 10; every wrong variant -- chirp
    sign flipped, centre off by one pulse, (nD - 1)^2 in the denominator, time counted from pulse 0, no chirp, half the rate --
    misses PEAK_TOL by at least 10 x, so the GPU gate tells them apart.
  * The accelerating scene, seed 5, walk 8, q = +-6, bank -8 .. 8 step 1 (17 hypotheses: the restatement's banks are not bound
    to the library's 16): the compensated level at (62, 23) is at least the static echo's - 2 dB, (62, 23) is the global argmax,
    the winning hypothesis is the scene's q, and the global maxima of the standard, the migration-only and the chirp-only maps
    are each at most the static echo's - 6 dB.
  * Doppler lengths off the grid of 32 pulses (MS.EDGE_GEOMS), with walk_sum_kernel<4, 2>'s groups of 16 rows: ``reach`` shows that the
    GPU cases on them run every block, run and window edge of MS.REACH_ITEMS; the five block-edge mutants of
    MS.block_edge_sum, with the chirp in the sum, each miss PEAK_TOL by 100 x or more at the weakest and the strongest rate of
    every GPU case where they change a read that lands in the map; the variant table above also runs at 95 x 64.

Measured here (printed by the tests).  Block-edge mutants: the smallest miss is 4.8e-2 of the peak, 4813 x the gate (the last
pulse repeated at 95 x 64, no table, q = 0.5).  fp32 emulation against fp64: 1.6e-7 .. 1.7e-7 of the peak at 65 x 44, 1.9e-7 .. 2.2e-7 at
2049 x 40; the fp32 chirp table alone 1.4e-8 .. 2.0e-8.  Smallest miss of a wrong variant: 1.7e-4 of the peak (the denominator
variant at 2049 x 40, q = 0.5); at 65 x 44 the smallest is 5.2e-3 (denominator, q = 0.5).  Scene, seed 5: the same echo static
62.7 dB; standard map 45.5 dB at the cell, global maximum 48.4 dB (-14.3 dB); migration alone 53.6 dB at the cell, global maximum
55.9 dB (-6.8 dB); the chirp bank without the walk 50.4 dB (-12.3 dB); both in one sum 61.4 dB at (62, 23) (-1.3 dB), the global
argmax, won by q = +6; with q = -6 61.3 dB, won by q = -6; with the walk removed from the scene the chirp bank alone 62.8 dB.  The
per-cell maximum over the 17 hypotheses raises the map's mean dB level from 33.4 to 38.4 dB.
"""
import numpy as np
import pytest

import migrate_scenes as MS
import rate_scenes as RS
from blah2_amd.process import doppler_rate, migrate_maps, migration_shifts, migration_table, range_map, rate_bank, rate_bank_maps, rate_chirps
from oracle import blah2_oracle as O
from test_timed_kernels_gpu import PEAK_TOL


def chirped_sum(R, s, c, rows=None):
    """M_k[j][d] of the definition for an integer shift table s[j][i] and one chirp row c[i], fp64; rows not in ``rows`` stay 0."""
    nD, nDelay = R.shape
    i = np.arange(nD)
    d = np.arange(nDelay)
    out = np.zeros((nD, nDelay), dtype=np.complex128)
    for j in (range(nD) if rows is None else np.flatnonzero(rows)):
        w = np.exp(-2j * np.pi * ((i * ((j + nD // 2 + 1) % nD)) % nD) / nD)
        col = d[None, :] + s[j][:, None]
        ok = (col >= 0) & (col < nDelay)
        out[j] = np.sum(np.where(ok, R[i[:, None], np.clip(col, 0, nDelay - 1)], 0.0) * (c * w)[:, None], axis=0)
    return out


def emulate_f32(R, s, c, rows):
    """The kernel's arithmetic on ``rows``: the fp32 cell times the fp32 chirp, then times the fp32 twiddle, fp32 multiply-adds
    in pulse order, blocks of 32 pulses added into a running sum."""
    nD, nDelay = R.shape
    Rf = R.astype(np.complex64)
    W = np.exp(-2j * np.pi * np.arange(nD) / nD).astype(np.complex64)
    cr, ci = c.real.astype(np.float32), c.imag.astype(np.float32)
    d = np.arange(nDelay)
    out = np.zeros((nD, nDelay), dtype=np.complex64)
    for j in np.flatnonzero(rows):
        src = (j + nD // 2 + 1) % nD
        acc_r = np.zeros(nDelay, np.float32)
        acc_i = np.zeros(nDelay, np.float32)
        for ib in range(0, nD, 32):
            br = np.zeros(nDelay, np.float32)
            bi = np.zeros(nDelay, np.float32)
            for i in range(ib, min(nD, ib + 32)):
                col = d + s[j, i]
                ok = (col >= 0) & (col < nDelay)
                r = np.where(ok, Rf[i, np.clip(col, 0, nDelay - 1)], np.complex64(0))
                zr = r.real * cr[i] - r.imag * ci[i]
                zi = r.real * ci[i] + r.imag * cr[i]
                w = W[(i * src) % nD]
                br = br + (zr * w.real - zi * w.imag)
                bi = bi + (zr * w.imag + zi * w.real)
            acc_r = acc_r + br
            acc_i = acc_i + bi
        out[j] = acc_r + 1j * acc_i
    return out


@pytest.fixture(scope="module")
def small():
    dims = MS.dims_of("g65x44")
    x, y, _ = MS.impulse_cpis(dims, 1, seed=11)
    return dims, range_map(dims, x, y)


def test_restatement_against_a_per_cell_loop(small):
    dims, R = small
    nD, nDelay = R.shape
    q = np.array([-3.0, 0.0, 0.5, 7.25])
    for name, h in (("none", None), ("physical", MS.tables(dims, 4)["physical"]), ("jagged", MS.tables(dims, 4)["jagged"])):
        maps, index, every = rate_bank_maps(R, q, h)
        assert maps.shape == R.shape and index.shape == R.shape and index.dtype == np.uint8 and every.shape == (4,) + R.shape
        rng = np.random.default_rng(3)
        for j, d in zip(rng.integers(0, nD, 24), rng.integers(0, nDelay, 24)):
            cand = []
            for k in range(q.size):
                acc = 0.0 + 0.0j
                for i in range(nD):
                    t = 2 * i - (nD - 1)
                    s = 0 if h is None else int(np.rint(h[j] * float(t)))
                    th = np.pi * q[k] * float(t * t) / (4.0 * nD * nD)
                    if 0 <= d + s < nDelay:
                        acc += (R[i, d + s] * complex(np.cos(th), -np.sin(th))) * np.exp(-2j * np.pi * ((i * ((j + nD // 2 + 1) % nD)) % nD) / nD)
                cand.append(acc)
                assert abs(every[k, j, d] - acc) <= 1e-12 * nD, (name, k, j, d)
            best = int(np.argmax(np.abs(cand)))
            assert index[j, d] == best and maps[j, d] == every[best, j, d]
    two, i2, e2 = rate_bank_maps(np.stack([R, 2 * R]), q)  # leading axes are maps
    one, i1, _ = rate_bank_maps(R, q)
    assert np.array_equal(two[0], one) and np.array_equal(i2[0], i1) and np.allclose(two[1], 2 * one) and e2.shape == (4, 2) + R.shape
    dup, idup, _ = rate_bank_maps(R, [0.5, 3.0, 0.5])  # the first of equals
    assert not (idup == 2).any() and (idup == 0).any()
    with pytest.raises(ValueError):
        rate_bank_maps(R, [])


def test_the_bank_of_zero_is_the_migration(small):
    dims, R = small
    for h in (MS.tables(dims, 4)["physical"], MS.tables(dims, 4)["limit"]):
        maps, index, every = rate_bank_maps(R, [0.0], h)
        assert np.array_equal(maps, migrate_maps(R, h)) and not index.any() and np.array_equal(every[0], maps)
    maps, _, _ = rate_bank_maps(R, 0.0)
    assert np.array_equal(maps, migrate_maps(R, np.zeros(dims.n_doppler_bins)))


def test_doppler_rate_signs_and_values():
    dims = MS.dims_of("g65x44")
    T = dims.n_doppler_bins * dims.n_corr / dims.fs
    fc = 204.64e6
    q = doppler_rate(dims, fc, 9.80665)
    assert q == -9.80665 * fc / 299792458.0 * T * T
    assert q < 0 and doppler_rate(dims, fc, -9.80665) == -q and doppler_rate(dims, fc, 0.0) == 0.0
    # a range that accelerates away lowers the Doppler: a fc / c Hz per second, times T seconds, in bins of 1 / T Hz
    assert np.isclose(q, -(9.80665 * fc / 299792458.0) * T / (1.0 / T), rtol=1e-14)
    # the figures of the design notes: 1 g over a 1 s CPI at 204.64 MHz is 6.7 bins, at 600 MHz 19.6
    class OneSecond:
        n_doppler_bins, n_corr, fs = 1000, 1000, 1_000_000
    assert abs(doppler_rate(OneSecond, 204.64e6, -9.80665) - 6.694) < 1e-3 and abs(doppler_rate(OneSecond, 600e6, -9.80665) - 19.627) < 1e-3
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            doppler_rate(dims, bad, 1.0)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            doppler_rate(dims, fc, bad)


def test_rate_bank():
    assert rate_bank(2).tolist() == [-2.0, -1.0, 0.0, 1.0, 2.0] and rate_bank(2).dtype == np.float64
    assert rate_bank(1.0, 0.5).tolist() == [-1.0, -0.5, 0.0, 0.5, 1.0]
    assert rate_bank(0.3, 0.1).size == 7 and rate_bank(0.3, 0.1)[3] == 0.0
    assert rate_bank(0).tolist() == [0.0] and rate_bank(2.9).tolist() == rate_bank(2).tolist()
    assert rate_bank(7).size == 15 and rate_bank(15, 2).size == 15
    for bad in ((8, 1.0), (4, 0.5), (1, 0.0), (1, -1.0), (-1, 1.0), (float("nan"), 1.0), (1, float("inf"))):
        with pytest.raises(ValueError):
            rate_bank(*bad)
    b = rate_bank(3.5, 0.5)
    assert np.array_equal(b, -b[::-1]) and b[b.size // 2] == 0.0


def test_rate_chirps():
    for nD in (64, 65, 2049):
        q = np.array([0.0, 0.5, -3.0, float(nD)])
        c = rate_chirps(q, nD)
        assert c.shape == (4, nD) and c.dtype == np.complex128
        assert (c[0] == 1.0).all()  # q = 0: exactly 1
        assert np.array_equal(c, c[:, ::-1])  # even about mid-CPI
        assert np.allclose(np.abs(c), 1.0, rtol=0, atol=1e-15)
        assert np.array_equal(c[2], np.conj(rate_chirps(3.0, nD)[0]))
        t = 2.0 * np.arange(nD) - (nD - 1)
        assert np.allclose(c[1], np.exp(-1j * np.pi * 0.5 * t * t / (4.0 * nD * nD)), rtol=0, atol=1e-15)
        # |q| = nD: the phase step between the last two pulses is pi (nD - 2) / nD, just short of half the slow-time rate
        step = np.angle(c[3, -1] * np.conj(c[3, -2]))
        assert abs(abs(step) - np.pi * (nD - 2) / nD) < 1e-9
    # a chirp of q bins: the instantaneous Doppler, in bins, runs from -q/2 to +q/2 about the middle
    nD = 65
    ph = np.unwrap(np.angle(np.conj(rate_chirps(6.0, nD)[0])))
    bins = np.diff(ph) / (2.0 * np.pi) * nD
    assert abs(bins[-1] - bins[0] - 6.0 * (nD - 2) / nD) < 1e-9 and abs(bins[nD // 2] + bins[nD // 2 - 1]) < 1e-9


VARIANTS = ("sign", "centre", "denominator", "from0", "none", "half")


def variant_chirp(q, nD, which):
    i = np.arange(nD, dtype=np.float64)
    t = 2.0 * i - (nD - 1)
    den = 4.0 * nD * nD
    if which == "sign":
        q = -q
    elif which == "centre":
        t = t + 2.0
    elif which == "denominator":
        den = 4.0 * (nD - 1) * (nD - 1)
    elif which == "from0":
        t = 2.0 * i
    elif which == "none":
        q = 0.0
    elif which == "half":
        q = 0.5 * q
    return np.exp(-1j * np.pi * q * t * t / den)


@pytest.mark.parametrize("geom,cells", [("g65x44", 4), ("g2049x40", 15), ("g95x64", 4)])
def test_the_gate_tells_every_wrong_variant_from_the_kernel_arithmetic(geom, cells):
    dims = MS.dims_of(geom)
    x, y, _ = MS.impulse_cpis(dims, 1, seed=21)
    R = range_map(dims, x, y)
    nD = dims.n_doppler_bins
    h = MS.tables(dims, cells)["physical"]
    s = migration_shifts(h, nD)
    assert np.abs(s).max() == cells
    rows = np.ones(nD, bool)
    if nD > 100:  # Python loops over rows and pulses: a spread of rows is enough
        rows[:] = False
        rows[np.r_[0:6, nD // 4, nD // 2 - 40, nD // 2, nD - 6:nD]] = True
    for q in (0.5, 3.0):
        c = rate_chirps(q, nD)[0]
        ref = chirped_sum(R, s, c, rows)
        peak = np.max(np.abs(ref))
        c32 = c.real.astype(np.float32).astype(np.float64) + 1j * c.imag.astype(np.float32).astype(np.float64)
        tab = np.max(np.abs(chirped_sum(R, s, c32, rows) - ref)) / peak
        e = np.max(np.abs(emulate_f32(R, s, c, rows)[rows] - ref[rows])) / peak
        print(f"{geom} q={q}: fp32 emulation {e:.2e} of the peak, the fp32 chirp table alone {tab:.2e}")
        assert tab <= PEAK_TOL / 10 and e <= PEAK_TOL / 10
        for which in VARIANTS:
            miss = np.max(np.abs(chirped_sum(R, s, variant_chirp(q, nD, which), rows) - ref)) / peak
            print(f"{geom} q={q}: variant {which} misses by {miss:.2e} of the peak")
            assert miss >= 10 * PEAK_TOL, (which, q)


# ---- Doppler lengths and windows off the 32-pulse grid ------------------------------------------------------------------------
def test_the_gpu_cases_reach_every_block_and_window_edge():
    """walk_sum_kernel<4, 2>'s groups of 16 rows: the (geometry, bank, table) cases of tests/test_rate_bank_gpu.py on the new
    geometries run every item of MS.REACH_ITEMS.  Every bank among them holds a rate other than 0, so every group stages."""
    import test_rate_bank_gpu as G
    assert [c for c in G.CASES if c[0] in MS.EDGE_GEOMS] == MS.EDGE_RATE_CASES
    assert all(np.any(np.asarray(G.banks(MS.SHAPES[g][0])[b]) != 0) for g, b, _ in MS.EDGE_RATE_CASES)
    found = MS.reach_suppliers([(g, t) for g, _, t in MS.EDGE_RATE_CASES], 16, live_only=False)
    for item, by in found.items():
        print(f"16-row groups, {item}: {', '.join(f'{g}-{t}' for g, t in by) or 'NO CASE'}")
    for item, by in found.items():
        assert by, f"no case of 16-row groups runs: {item}"
    # the chirps[] rows behind a partial block and the vmask of a partial group: blocks of 7 .. 31 pulses, groups of 1 .. 15 rows
    assert {MS.SHAPES[g][0] % 32 for g, _, _ in MS.EDGE_RATE_CASES} == {21, 16, 17, 31, 7}
    assert {MS.SHAPES[g][0] % 16 for g, _, _ in MS.EDGE_RATE_CASES} == {5, 0, 1, 15, 7}


@pytest.mark.parametrize("geom,bank,table", MS.EDGE_RATE_CASES, ids=[f"{g}-{b}-{t}" for g, b, t in MS.EDGE_RATE_CASES])
def test_the_gate_tells_every_block_edge_mutant(geom, bank, table):
    """With the chirp in the sum and groups of 16 rows: a kernel that drops, repeats or halves a partial last block, clamps the
    walks of a partial last row group or loses the reads across a strip seam misses PEAK_TOL by 100 x or more wherever it differs
    from the truth at all, at the case's weakest and strongest rate.  Derived: on the impulse-reference CPIs one lost or repeated
    pulse moves a cell by at least 0.5 (the chirp has modulus 1) against a peak of at most 1.5 nD, 3.5e-3 at nD = 95."""
    import test_rate_bank_gpu as G
    dims = MS.dims_of(geom)
    x, y, _ = MS.impulse_cpis(dims, 1, seed=21)
    R = range_map(dims, x, y)
    nD = dims.n_doppler_bins
    h = None if table == "none" else MS.tables(dims, MS.CELLS[geom])[table]
    s = migration_shifts(np.zeros(nD) if h is None else h, nD)
    bank_q = np.asarray(G.banks(nD)[bank], dtype=np.float64)
    nonzero = bank_q[bank_q != 0]
    for q in sorted({float(nonzero[np.argmin(np.abs(nonzero))]), float(nonzero[np.argmax(np.abs(nonzero))])}):
        c = rate_chirps(q, nD)[0]
        ref = MS.block_edge_sum(R, s, None, chirp=c, rows_per_group=16)
        assert np.array_equal(ref, chirped_sum(R, s, c))
        assert np.max(np.abs(ref - rate_bank_maps(R, [q], h)[2][0])) <= 1e-12 * nD
        peak = np.max(np.abs(ref))
        assert peak <= 1.5 * nD
        differ = 0
        for which in MS.BLOCK_EDGE_MUTANTS:
            got = MS.block_edge_sum(R, s, which, chirp=c, rows_per_group=16)
            if MS.block_edge_identity(which, s, dims.n_delay_bins, None, 16):
                assert np.array_equal(got, ref), which
                print(f"{geom} {table} q={q:.3g}: mutant {which} is the identity here")
                continue
            differ += 1
            miss = np.max(np.abs(got - ref)) / peak
            print(f"{geom} {table} q={q:.3g}: mutant {which} misses by {miss:.2e} of the peak, {miss / PEAK_TOL:.0f} x the gate")
            assert miss >= 100 * PEAK_TOL, (which, q)
        assert differ >= 2  # a partial block at every new geometry: dropped and repeated always differ


_scene = {}


def scene_maps(q):
    """The accelerating scene's maps in the restatement, once per q."""
    if q not in _scene:
        dims = MS.scene_dims()
        h = migration_table(dims, MS.scene_fc(dims))
        bank = np.arange(-8.0, 9.0)
        x, y = RS.scene(q=q)
        R = range_map(dims, x, y)
        xs, ys = MS.scene(walk=0.0)
        _scene[q] = dict(dims=dims, bank=bank, static=O.ambiguity_process(dims, xs, ys), std=O.ambiguity_process(dims, x, y),
                         mig=migrate_maps(R, h), chirp=rate_bank_maps(R, bank)[0], both=rate_bank_maps(R, bank, h))
    return _scene[q]


def gmax_db(m):
    return 20.0 * np.log10(np.abs(m).max())


def test_the_scene_helper_keeps_the_migration_scene():
    x0, y0 = MS.scene()
    x, y = RS.scene(q=0.0)
    assert np.array_equal(x, x0) and np.max(np.abs(y - y0)) <= 1e-15
    # what is left of y without the noise is the echo alone: amplitude 0.05 of a unit-power reference
    x6, y6 = RS.scene()
    assert np.array_equal(x6, x0) and abs(np.std(y6 - y0) / (np.sqrt(2.0) * MS.SCENE_AMP) - 1.0) < 0.3


@pytest.mark.parametrize("q", [6.0, -6.0])
def test_the_accelerating_scene(q):
    m = scene_maps(q)
    cell = (MS.SCENE_ROW, MS.SCENE_COL)
    static = MS.level_db(m["static"], *cell)
    maps, index, every = m["both"]
    got = MS.level_db(maps, *cell)
    won = m["bank"][index[cell]]
    print(f"scene q={q:+.0f}: static {static:.1f} dB; standard {MS.level_db(m['std'], *cell):.1f} dB at the cell, global maximum "
          f"{gmax_db(m['std']):.1f} dB ({gmax_db(m['std']) - static:+.1f}); migration alone {MS.level_db(m['mig'], *cell):.1f} dB at the cell, "
          f"global maximum {gmax_db(m['mig']):.1f} dB ({gmax_db(m['mig']) - static:+.1f}); chirp bank without the walk {gmax_db(m['chirp']):.1f} dB "
          f"({gmax_db(m['chirp']) - static:+.1f}); both {got:.1f} dB ({got - static:+.1f}) won by q = {won:+.0f}")
    mean_db = lambda z: float(np.mean(20.0 * np.log10(np.abs(z))))
    print(f"scene q={q:+.0f}: mean level {mean_db(m['mig']):.1f} dB migrated, {mean_db(maps):.1f} dB under the maximum of {m['bank'].size}")
    assert got >= static - 2.0
    assert np.unravel_index(np.argmax(np.abs(maps)), maps.shape) == cell
    assert won == q
    for name in ("std", "mig", "chirp"):
        assert gmax_db(m[name]) <= static - 6.0, name
    assert np.array_equal(every[8], m["mig"])  # the bank's q = 0 is the migration


def test_the_chirp_bank_alone_on_an_echo_that_does_not_walk():
    dims = MS.scene_dims()
    x, y = RS.scene(walk=0.0)
    xs, ys = MS.scene(walk=0.0)
    cell = (MS.SCENE_ROW, MS.SCENE_COL)
    static = MS.level_db(O.ambiguity_process(dims, xs, ys), *cell)
    maps, index, _ = rate_bank_maps(range_map(dims, x, y), np.arange(-8.0, 9.0))
    got = MS.level_db(maps, *cell)
    print(f"no walk: static {static:.1f} dB, chirp bank {got:.1f} dB")
    assert abs(got - static) <= 0.5 and index[cell] == 14 and np.unravel_index(np.argmax(np.abs(maps)), maps.shape) == cell
