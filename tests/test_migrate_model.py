"""CPU: the range-migration definition restated in blah2_amd.process (migration_table, migration_shifts, range_map,
migrate_maps) on the scenes of tests/migrate_scenes.py.  Needs no GPU and no library: tests/test_migrate_gpu.py holds the device
to these restatements.

  * migrate_maps against a per-cell Python loop of the definition; range_map + an unshifted Doppler sum against the oracle's
    ambiguity_process; migration_table's signs and values; migration_shifts' ties to even.
  * Zero-shift rows of migrate_maps(range_map) equal ambiguity_process's rows.
  * The variant table on the impulse-reference CPIs (a): an fp32 emulation of the kernel's sum (blocks of 32 pulses into a
    running sum) stays under PEAK_TOL; every wrong variant -- shift sign flipped, wrap instead of zero, floor or truncate instead
    of rint, centre off by one pulse, no shift -- misses PEAK_TOL by at least 10 x, so the GPU gate tells them apart.
  * The moving-echo scene (b) on the restatement: the compensated level at (62, 23) is at least the static echo's - 1.5 dB, the
    standard map's row maximum is at most the static echo's - 10 dB, and the compensated map's global argmax is (62, 23).
  * Doppler lengths off the grid of 32 pulses (MS.EDGE_GEOMS).  ``reach`` shows that the GPU cases on them run blocks of 7, 16, 17,
    21 and 31 pulses, a run of 17 .. 31 pulses, a wide window staged in runs whose last is short, a window that leaves the map on
    both sides at once and an interior strip's window that leaves it on neither.  Five block-edge mutants -- partial last block
    dropped, padded with its last pulse, its pulses 16 .. 31 dropped; a partial last row group on the last row's walk; reads
    across a strip seam zero -- each miss PEAK_TOL by 100 x or more (derived: one pulse is at least 0.5 against a peak of at most
    1.5 nD) on every GPU case where they change a read that lands in the map; the variant table above also runs at 95 x 64.

Measured here.  Block-edge mutants: the smallest miss is 4.6e-2 of the peak, 4645 x the gate (the last pulse repeated at 95 x 64,
physical table).  Zero-shift rows against ambiguity_process: 4.7e-16 of the peak.  fp32 emulation against fp64: 1.7e-7 of the peak
at 65 x 44 (walk 4), 2.6e-7 at 2049 x 40 (walk 15, a spread of rows).  Smallest miss of a wrong variant: 0.14 of the peak (centre
off by one pulse at 2049 x 40), 0.45 at 65 x 44.  Scene (b), seed 5: the same echo without walk 62.7 dB; standard map 45.1 dB at the
cell and 48.3 dB at the row's maximum (-14.4 dB); compensated map 61.7 dB at (62, 23) (-1.0 dB), which is its global argmax.
"""
import numpy as np
import pytest

import migrate_scenes as MS
from blah2_amd.process import migrate_maps, migration_shifts, migration_table, range_map
from oracle import blah2_oracle as O
from test_timed_kernels_gpu import PEAK_TOL


def doppler_sum(R, s, rows=None):
    """M'[j][d] of the definition for an integer shift table s[j][i], fp64; the rows not in ``rows`` stay zero."""
    nD, nDelay = R.shape
    i = np.arange(nD)
    d = np.arange(nDelay)
    out = np.zeros((nD, nDelay), dtype=np.complex128)
    for j in (range(nD) if rows is None else np.flatnonzero(rows)):
        w = np.exp(-2j * np.pi * ((i * ((j + nD // 2 + 1) % nD)) % nD) / nD)
        c = d[None, :] + s[j][:, None]
        ok = (c >= 0) & (c < nDelay)
        out[j] = np.sum(np.where(ok, R[i[:, None], np.clip(c, 0, nDelay - 1)], 0.0) * w[:, None], axis=0)
    return out


def emulate_f32(R, s, rows):
    """The kernel's arithmetic on ``rows``: fp32 multiply-adds in pulse order, blocks of 32 pulses added into a running sum."""
    nD, nDelay = R.shape
    Rf = R.astype(np.complex64)
    W = np.exp(-2j * np.pi * np.arange(nD) / nD).astype(np.complex64)
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
                c = d + s[j, i]
                ok = (c >= 0) & (c < nDelay)
                r = np.where(ok, Rf[i, np.clip(c, 0, nDelay - 1)], np.complex64(0))
                w = W[(i * src) % nD]
                br = br + (r.real * w.real - r.imag * w.imag)
                bi = bi + (r.real * w.imag + r.imag * w.real)
            acc_r = acc_r + br
            acc_i = acc_i + bi
        out[j] = acc_r + 1j * acc_i
    return out


@pytest.fixture(scope="module")
def small():
    dims = MS.dims_of("g65x44")
    x, y, _ = MS.impulse_cpis(dims, 1, seed=11)
    R = range_map(dims, x, y)
    return dims, x, y, R


def test_impulse_reference_range_map_is_the_surveillance_channel(small):
    dims, x, y, R = small
    nD, nC = dims.n_doppler_bins, dims.n_corr
    want = y.astype(np.complex128)[:nD * nC].reshape(nD, nC)[:, :dims.n_delay_bins]
    assert np.max(np.abs(R - want)) <= 1e-13
    assert np.abs(R).min() >= 0.499 and np.abs(R).max() <= 1.501


def test_range_map_and_an_unshifted_sum_are_the_oracle(small):
    dims, x, y, R = small
    ref = O.ambiguity_process(dims, x, y)
    got = migrate_maps(R, np.zeros(dims.n_doppler_bins))
    assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref))
    dims2 = MS.dims_of("gasym")  # the rotated reference channel
    x2, y2, _ = MS.impulse_cpis(dims2, 1, seed=12)
    ref2 = O.ambiguity_process(dims2, x2, y2)
    got2 = migrate_maps(range_map(dims2, x2, y2), np.zeros(dims2.n_doppler_bins))
    assert np.max(np.abs(got2 - ref2)) <= 1e-12 * np.max(np.abs(ref2))


def test_restatement_against_a_per_cell_loop(small):
    dims, x, y, R = small
    nD, nDelay = R.shape
    for name, h in MS.tables(dims, 4).items():
        got = migrate_maps(R, h)
        rng = np.random.default_rng(3)
        for j, d in zip(rng.integers(0, nD, 40), rng.integers(0, nDelay, 40)):
            acc = 0.0 + 0.0j
            for i in range(nD):
                s = int(np.rint(h[j] * float(2 * i - (nD - 1))))
                if 0 <= d + s < nDelay:
                    acc += R[i, d + s] * np.exp(-2j * np.pi * ((i * ((j + nD // 2 + 1) % nD)) % nD) / nD)
            assert abs(got[j, d] - acc) <= 1e-12 * nD, (name, j, d)
    two = migrate_maps(np.stack([R, 2 * R]), MS.tables(dims, 4)["physical"])  # leading axes are maps
    assert np.array_equal(two[0], migrate_maps(R, MS.tables(dims, 4)["physical"])) and np.allclose(two[1], 2 * two[0])


def test_zero_shift_rows_are_the_oracle_rows(small):
    dims, x, y, R = small
    h = MS.tables(dims, 4)["physical"]
    zero = MS.zero_rows(h, dims.n_doppler_bins)
    assert 0 < zero.sum() < dims.n_doppler_bins and zero[dims.n_doppler_bins // 2]
    ref = O.ambiguity_process(dims, x, y)
    got = migrate_maps(R, h)
    ratio = np.max(np.abs(got[zero] - ref[zero])) / np.max(np.abs(ref))
    print(f"zero-shift rows against ambiguity_process: {ratio:.2e} of the peak")
    assert ratio <= 1e-13
    assert np.max(np.abs(got[~zero] - ref[~zero])) / np.max(np.abs(ref)) > 0.1  # the other rows are not the oracle's


def test_migration_table_signs_and_values():
    dims = MS.dims_of("g65x44")
    fc = 204.64e6
    h = migration_table(dims, fc)
    assert h.dtype == np.float64 and h.shape == (65,)
    assert np.array_equal(h, -0.5 * dims.doppler * float(dims.n_corr) / fc)
    assert h[32] == 0.0 and (h[33:] < 0).all() and (h[:32] > 0).all()  # positive Doppler approaches: the delay falls
    # the walk over the whole CPI, 2 h nD, is -f N / fc samples
    N = dims.n_corr * dims.n_doppler_bins
    assert np.allclose(2.0 * h * dims.n_doppler_bins, -dims.doppler * N / fc, rtol=1e-15)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            migration_table(dims, bad)
    s = migration_shifts([0.25, -0.25, 0.75], 4)  # t = -3, -1, 1, 3: ties go to even
    assert s.tolist() == [[-1, 0, 0, 1], [1, 0, 0, -1], [-2, -1, 1, 2]]
    s = migration_shifts(h, 65)
    assert np.array_equal(s, -s[:, ::-1]) and (np.diff(s, axis=1) * np.sign(h)[:, None] >= 0).all()  # odd about mid-CPI, monotone


VARIANTS = ("sign", "wrap", "floor", "trunc", "centre", "none")


def variant_sum(R, h, which, rows):
    nD, nDelay = R.shape
    t = (2 * np.arange(nD) - (nD - 1)).astype(np.float64)
    p = np.asarray(h, dtype=np.float64)[:, None] * t[None, :]
    if which == "sign":
        s = -np.rint(p)
    elif which == "floor":
        s = np.floor(p)
    elif which == "trunc":
        s = np.trunc(p)
    elif which == "centre":
        s = np.rint(np.asarray(h, dtype=np.float64)[:, None] * (t + 2.0)[None, :])
    elif which == "none":
        s = np.zeros_like(p)
    else:
        s = np.rint(p)
    s = s.astype(np.int64)
    if which == "wrap":  # the map three times side by side: the middle copy's columns see their neighbours modulo nDelay
        assert np.abs(s).max() <= nDelay
        return doppler_sum(np.concatenate([R, R, R], axis=1), s, rows)[:, nDelay:2 * nDelay]
    return doppler_sum(R, s, rows)


@pytest.mark.parametrize("geom,cells", [("g65x44", 4), ("g2049x40", 15), ("g95x64", 4)])
def test_the_gate_tells_every_wrong_variant_from_the_kernel_arithmetic(geom, cells):
    dims = MS.dims_of(geom)
    x, y, _ = MS.impulse_cpis(dims, 1, seed=21)
    R = range_map(dims, x, y)
    nD = dims.n_doppler_bins
    h = MS.tables(dims, cells)["physical"]
    s = migration_shifts(h, nD)
    assert np.abs(s).max() == cells
    rows = ~MS.zero_rows(h, nD)
    if nD > 100:  # Python loops over rows and pulses: a spread of rows is enough
        keep = np.zeros(nD, bool)
        keep[np.r_[0:6, nD // 4, nD // 2 - 40, nD - 6:nD]] = True
        rows &= keep
    ref = doppler_sum(R, s, rows)
    peak = np.max(np.abs(ref))
    emu = emulate_f32(R, s, rows)
    e = np.max(np.abs(emu[rows] - ref[rows])) / peak
    print(f"{geom}: fp32 emulation {e:.2e} of the peak")
    assert e <= PEAK_TOL / 10
    for which in VARIANTS:
        got = variant_sum(R, h, which, rows)
        miss = np.max(np.abs(got - ref)) / peak
        print(f"{geom}: variant {which} misses by {miss:.3f} of the peak")
        assert miss >= 10 * PEAK_TOL, which


# ---- Doppler lengths and windows off the 32-pulse grid ------------------------------------------------------------------------
def test_reach_restates_the_window_arithmetic():
    """reach() on cases worked out by hand from walk_sum_kernel's lines."""
    # no table: one window of the strip's own four tiles, whole runs
    b = MS.reach(21, 64, None, 16)
    assert [(x["strip"], x["group"], x["block"]) for x in b] == [(0, 0, 0), (0, 1, 0)]
    assert all((x["nb"], x["t0"], x["t1"], x["Wc"], x["P"], x["pn"], x["live"]) == (21, 0, 3, 64, 32, (21,), False) for x in b)
    # 48 x 65, half walk 4 / 47 in every row: shifts -4 .. 1 in block 0 (t = -47 .. 15), 1 .. 4 in block 1 (t = 17 .. 47)
    b = MS.reach(48, 65, np.full(48, 4.0 / 47.0), 32)
    assert len(b) == 2 * 2 * 2 and all(x["live"] and x["nTiles"] == 5 and not x["interior"] for x in b)
    first = {(x["strip"], x["block"]): (x["nb"], x["t0"], x["t1"], x["pn"]) for x in b if x["group"] == 1}
    assert first == {(0, 0): (32, -1, 4, (32,)), (0, 1): (16, 0, 4, (16,)), (1, 0): (32, 3, 8, (32,)), (1, 1): (16, 4, 8, (16,))}
    # the widest window: +-512 in one group, 64 + 1024 columns in 68 tiles -> 3 pulses a run, 7 pulses in runs of 3, 3, 1
    b = MS.reach(7, 64, MS.tables(MS.dims_of("g7x64"), 4)["limit"], 32)
    assert len(b) == 1 and (b[0]["t0"], b[0]["t1"], b[0]["Wc"], b[0]["P"], b[0]["pn"]) == (-32, 35, 1088, 3, (3, 3, 1))


def test_the_gpu_cases_reach_every_block_and_window_edge():
    """walk_sum_kernel<8, 1>'s groups of 32 rows: the (geometry, table) cases of tests/test_migrate_gpu.py on the new geometries run
    every item of MS.REACH_ITEMS, in a group that stages (one with a migrated row).  tests/test_rate_bank_model.py has the same
    for walk_sum_kernel<4, 2>'s groups of 16."""
    import test_migrate_gpu as G
    assert [c for c in G.CASES if c[0] in MS.EDGE_GEOMS] == MS.EDGE_MIGRATE_CASES
    found = MS.reach_suppliers(MS.EDGE_MIGRATE_CASES, 32, live_only=True)
    for item, by in found.items():
        print(f"32-row groups, {item}: {', '.join(f'{g}-{t}' for g, t in by) or 'NO CASE'}")
    for item, by in found.items():
        assert by, f"no case of 32-row groups runs: {item}"
    # the partial row groups themselves: 7, 16, 17, 21 and 31 live rows
    assert {MS.SHAPES[g][0] % 32 for g, _ in MS.EDGE_MIGRATE_CASES} == {21, 16, 17, 31, 7}


@pytest.mark.parametrize("geom,table", MS.EDGE_MIGRATE_CASES, ids=lambda v: v)
def test_the_gate_tells_every_block_edge_mutant(geom, table):
    """A kernel that drops, repeats or halves a partial last block, clamps the walks of a partial last row group or loses the
    reads across a strip seam misses PEAK_TOL by 100 x or more wherever it differs from the truth at all.  Derived: on the
    impulse-reference CPIs one lost or repeated pulse moves a cell by at least 0.5 against a peak of at most 1.5 nD, 3.5e-3 of
    the peak at nD = 95."""
    dims = MS.dims_of(geom)
    x, y, _ = MS.impulse_cpis(dims, 1, seed=21)
    R = range_map(dims, x, y)
    nD = dims.n_doppler_bins
    h = MS.tables(dims, MS.CELLS[geom])[table]
    s = migration_shifts(h, nD)
    rows = ~MS.zero_rows(h, nD)
    ref = MS.block_edge_sum(R, s, None, rows)
    assert np.array_equal(ref, doppler_sum(R, s, rows))
    assert np.max(np.abs(ref - migrate_maps(R, h))[rows]) <= 1e-12 * nD
    peak = np.max(np.abs(ref))
    assert peak <= 1.5 * nD
    differ = 0
    for which in MS.BLOCK_EDGE_MUTANTS:
        got = MS.block_edge_sum(R, s, which, rows)
        if MS.block_edge_identity(which, s, dims.n_delay_bins, rows, 32):
            assert np.array_equal(got, ref), which
            print(f"{geom} {table}: mutant {which} is the identity here")
            continue
        differ += 1
        miss = np.max(np.abs(got - ref)) / peak
        print(f"{geom} {table}: mutant {which} misses by {miss:.2e} of the peak, {miss / PEAK_TOL:.0f} x the gate")
        assert miss >= 100 * PEAK_TOL, which
    assert nD % 32 != 0 and differ >= 2  # a partial block and a partial row group at every new geometry


def test_every_block_edge_mutant_differs_on_some_new_geometry():
    """None of the five is the identity everywhere: each is told on at least two of the new geometries."""
    for which in MS.BLOCK_EDGE_MUTANTS:
        hit = set()
        for geom, table in MS.EDGE_MIGRATE_CASES:
            dims = MS.dims_of(geom)
            h = MS.tables(dims, MS.CELLS[geom])[table]
            s = migration_shifts(h, dims.n_doppler_bins)
            if not MS.block_edge_identity(which, s, dims.n_delay_bins, ~MS.zero_rows(h, dims.n_doppler_bins), 32):
                hit.add(geom)
        assert len(hit) >= 2, (which, hit)


def test_the_moving_echo_scene():
    dims = MS.scene_dims()
    assert abs(dims.doppler[MS.SCENE_ROW] - 150.09) < 0.01 and dims.delay[MS.SCENE_COL] == MS.SCENE_DELAY
    h = migration_table(dims, MS.scene_fc(dims))
    s = migration_shifts(h, dims.n_doppler_bins)
    assert s[MS.SCENE_ROW, 0] == 4 and s[MS.SCENE_ROW, -1] == -4
    x, y = MS.scene()
    xs, ys = MS.scene(walk=0.0)
    static = MS.level_db(O.ambiguity_process(dims, xs, ys), MS.SCENE_ROW, MS.SCENE_COL)
    std = O.ambiguity_process(dims, x, y)
    comp = migrate_maps(range_map(dims, x, y), h)
    at_cell = MS.level_db(std, MS.SCENE_ROW, MS.SCENE_COL)
    row_max = 20.0 * np.log10(np.abs(std[MS.SCENE_ROW]).max())
    got = MS.level_db(comp, MS.SCENE_ROW, MS.SCENE_COL)
    print(f"scene: static {static:.1f} dB, standard {at_cell:.1f} dB at the cell, {row_max:.1f} dB row maximum, compensated {got:.1f} dB")
    assert got >= static - 1.5
    assert row_max <= static - 10.0
    assert np.unravel_index(np.argmax(np.abs(comp)), comp.shape) == (MS.SCENE_ROW, MS.SCENE_COL)
