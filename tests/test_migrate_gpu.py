"""GPU: walk_sum_kernel<8, 1> (blah2hip_amb_set_migration / blah2hip_amb_migrate_dev, Ambiguity.set_migration / migrate_dev) on the
impulse-reference CPIs and the moving-echo scene of tests/migrate_scenes.py.  tests/test_migrate_model.py shows on the CPU that
the gate used here tells the kernel's arithmetic from every wrong walk (sign, wrap, floor, truncate, centre, none).

No reference counterpart; the checks are
  * cells: ``max|M' - migrate_maps(range_map(x, y), h)| <= PEAK_TOL max|ref|`` (PEAK_TOL = 1e-5, the project's gate) with hot
    columns and leak compensation off, on six geometries (65 x 44; 65 x 45, an odd cell count; 129 x 111, two column strips;
    2049 x 40, 65 blocks of pulses; the explicit even 64 bins; asymmetric Doppler limits) and five tables (physical; reversed;
    walks beyond the map's last column; exactly +-BLAH2HIP_MAX_MIGRATION; neighbouring rows with opposite walks), 3 CPIs a
    call with NaN gaps between the planes' CPIs, in place and out of place, the outputs between guard words; and on five
    geometries off the grid of 32 pulses (21 x 64, 48 x 65, 81 x 200, 95 x 64, 7 x 64: last blocks of 21, 16, 17, 31 and 7
    pulses, last row groups of as many rows, a strip of exactly 64 columns, one of a single column, two interior strips),
    whose reach tests/test_migrate_model.py proves;
  * zero-shift rows are the process call's bits (hot columns and leak compensation forced on); two calls give the same bits;
    map 0 of a call of one map is map 0 of a call of three;
  * metrics within 1e-3 dB of fp64 Map::set_metrics of the device's own output, with a peak planted along a migrated row's walk;
  * process_multi_dev with 2 channels x 2 CPIs, then four maps, against the restatement per channel;
  * the moving-echo scene: the device's argmax at (62, 23), its level within 0.01 dB of the restatement's;
  * every BLAH2HIP_ERR_INVALID case, with nothing written.

Measured on the MI355X (printed by the tests).  Cells, largest error over the peak: 2.1e-7 .. 6.5e-7 on the maps of 64 .. 129
rows, 1.2e-6 .. 2.2e-6 at 2049 x 40, the same in place and out of place.  Metrics with the planted peak: noisePower 4.9e-7 dB,
maxPower 6.5e-7 dB from fp64 set_metrics of the device's own cells.  Scene: 61.699 dB on the device and in the restatement,
45.1 dB at that cell of the standard map.  With both options forced on, the scene's direct path still does not pass the
hot-column test (0 columns rewritten): the bit-for-bit check of the zero-shift rows holds whatever wrote them.  No defect was found.
Off the grid of 32 pulses: 1.6e-7 .. 5.0e-7 of the peak on the 19 cases of the five new geometries (largest: 95 x 64, ``limit``),
the same in place and out of place; the planted peak at (80, 150) of 81 x 200: noisePower 4.3e-7 dB, maxPower 6.7e-7 dB; two
calls and one map of three give equal bits at 95 x 64.  A library built with pulses 16 .. 31 of a partial block left out of the
staging passed every case from before and failed six of the new ones (21 x 64, 81 x 200 and 95 x 64 with runs of more than 16
pulses).  No defect was found.
"""
import numpy as np
import pytest

import migrate_scenes as MS
from oracle import blah2_oracle as O
from test_timed_kernels_gpu import PEAK_TOL

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces
PAD = 64
MAX_BATCH = 4


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


class Arena:
    """``words`` 32-bit words between two runs of guard words."""

    def __init__(self, torch, words):
        self.words = words
        self.whole = torch.full((PAD + words + PAD,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
        self.ptr = self.whole.data_ptr() + 4 * PAD
        assert self.ptr % 16 == 0

    def read(self, used_words):
        host = self.whole.cpu().numpy().view(np.uint32)
        assert (host[:PAD] == GUARD).all(), "the guard in front was written"
        assert (host[PAD + used_words:] == GUARD).all(), "written behind the output"
        return host[PAD:PAD + used_words].copy()

    def untouched(self):
        return bool((self.whole.cpu().numpy().view(np.uint32) == GUARD).all())


_handles = {}


def handle(b2, name, hot=0, leak=0):
    key = (name, hot, leak)
    if key not in _handles:
        limits, bins = (MS.SCENE_LIMITS, 0) if name == "scene" else MS.GEOMS[name]
        amb = b2.Ambiguity(*limits, True, max_batch=MAX_BATCH, n_doppler_bins=bins)
        amb.set_hot_columns(hot)
        amb.set_leak_compensation(leak)
        _handles[key] = amb
    return _handles[key]


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def upload(torch, z):
    return torch.from_numpy(np.ascontiguousarray(z).view(np.float32).copy()).cuda()


def process(torch, b2, amb, x, y, stride, n_cpi):
    """process_dev into a guarded arena -> (arena, metrics arena, maps [n_cpi, nD, nC] as they stand)."""
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    dx, dy = upload(torch, x), upload(torch, y)
    maps, met = Arena(torch, n_cpi * nD * nC * 2), Arena(torch, n_cpi * 4)
    amb.process_dev(b2.FMT_C32, dx.data_ptr(), dy.data_ptr(), n_cpi, stride, maps.ptr, met.ptr, stream_of(torch))
    torch.cuda.synchronize()
    return maps, met, maps.read(maps.words).view(np.complex64).reshape(n_cpi, nD, nC)


def migrate(torch, amb, maps, n_maps, in_place):
    """migrate_dev on the arena of a process call -> (out [n_maps, nD, nC], metrics [n_maps, 2])."""
    from blah2_amd import _lib
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    before = maps.read(maps.words)
    dst = maps if in_place else Arena(torch, n_maps * nD * nC * 2)
    met = Arena(torch, n_maps * 4)
    amb.migrate_dev(maps.ptr, n_maps, dst.ptr, met.ptr, stream_of(torch))
    torch.cuda.synchronize()
    assert amb.info(_lib.INFO_MIGRATE_GRID) == -(-nC // 64) * -(-nD // 32)
    after = maps.read(maps.words)
    if in_place:
        assert np.array_equal(after[n_maps * nD * nC * 2:], before[n_maps * nD * nC * 2:]), "a map behind n_maps was written"
    else:
        assert np.array_equal(after, before), "the input maps were written"
    out = (after if in_place else dst.read(dst.words))[:n_maps * nD * nC * 2].view(np.complex64).reshape(n_maps, nD, nC)
    return out, met.read(n_maps * 4).view(np.float64).reshape(n_maps, 2)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


_inputs = {}


def inputs(b2, geom, n_cpi, seed):
    """The CPIs of a geometry and their fp64 range maps, drawn once."""
    key = (geom, n_cpi, seed)
    if key not in _inputs:
        dims = MS.dims_of(geom)
        x, y, stride = MS.impulse_cpis(dims, n_cpi, seed, gap=37)
        used = dims.n_doppler_bins * dims.n_corr
        R = np.stack([b2.range_map(dims, x[c * stride:c * stride + used], y[c * stride:c * stride + used]) for c in range(n_cpi)])
        _inputs[key] = dims, x, y, stride, R
    return _inputs[key]


def check_metrics(out, met, tag):
    for i in range(out.shape[0]):
        noise, peak = MS.set_metrics64(out[i])
        assert abs(met[i, 0] - noise) <= MS.DB_TOL and abs(met[i, 1] - peak) <= MS.DB_TOL, (tag, i, met[i], noise, peak)


# ---- 1. cells ---------------------------------------------------------------------------------------------------------------
CELLS = MS.CELLS
TABLES = ("physical", "reversed", "beyond", "limit", "jagged")
CASES = [(g, t) for g in CELLS if g not in MS.EDGE_GEOMS for t in TABLES if g != "g2049x40" or t in ("physical", "limit", "jagged")]
# Doppler lengths off the 32-pulse grid; tests/test_migrate_model.py shows which block, run and window edges each of them runs
CASES += MS.EDGE_MIGRATE_CASES


@pytest.mark.parametrize("geom,table", CASES, ids=[f"{g}-{t}" for g, t in CASES])
def test_cells_against_the_restatement(b2, torch, geom, table):
    n_cpi = 1 if geom == "g2049x40" else 3
    dims, x, y, stride, R = inputs(b2, geom, n_cpi, seed=100 + len(geom))
    amb = handle(b2, geom)
    assert (amb.get_n_doppler_bins(), amb.get_n_delay_bins(), amb.get_n_corr()) == MS.SHAPES[geom] + (dims.n_corr,)
    nD = dims.n_doppler_bins
    h = MS.tables(dims, CELLS[geom])[table]
    s = b2.migration_shifts(h, nD)
    if table == "limit":
        assert s.min() == -MS.MAX_MIGRATION and s.max() == MS.MAX_MIGRATION
    if table == "beyond":
        assert np.abs(s).max() > dims.n_delay_bins
    if table == "physical":
        assert np.abs(s).max() == CELLS[geom]
        assert np.array_equal(amb.migration_table(MS.fc_for(dims, CELLS[geom])), h)  # the library's table is the restatement's
    ref = b2.migrate_maps(R, h)
    peak = np.max(np.abs(ref))
    zero = MS.zero_rows(h, nD)
    amb.set_migration(h)
    for in_place in ((True, False) if table == "physical" else (TABLES.index(table) % 2 == 0,)):
        maps, _, std = process(torch, b2, amb, x, y, stride, n_cpi)
        out, met = migrate(torch, amb, maps, n_cpi, in_place)
        assert np.isfinite(out.view(np.float32)).all()
        err = np.max(np.abs(out.astype(np.complex128) - ref)) / peak
        print(f"migrate {geom} {table} in_place={in_place}: {err:.2e} of the peak, {int(zero.sum())} zero-shift rows")
        assert err <= PEAK_TOL, (geom, table, in_place, err)
        assert same_bits(out[:, zero], std[:, zero])
        check_metrics(out, met, (geom, table))


# ---- 2. bits ----------------------------------------------------------------------------------------------------------------
def test_zero_shift_rows_keep_the_hot_column_and_leak_values(b2, torch):
    from blah2_amd import _lib
    amb = handle(b2, "scene", hot=_lib.LEAK_ALWAYS, leak=_lib.LEAK_ALWAYS)
    dims = MS.scene_dims()
    x, y = MS.scene()
    y = y + 0.8 * x  # a direct path: the zero-delay column is hot
    h = b2.migration_table(dims, MS.scene_fc(dims))
    zero = MS.zero_rows(h, dims.n_doppler_bins)
    assert 0 < zero.sum() < dims.n_doppler_bins
    amb.set_migration(h)
    x32, y32 = x.astype(np.complex64), y.astype(np.complex64)
    for in_place in (True, False):
        maps, _, std = process(torch, b2, amb, x32, y32, x32.size, 1)
        print(f"hot columns rewritten: {amb.hot_columns()}")
        out, met = migrate(torch, amb, maps, 1, in_place)
        assert same_bits(out[:, zero], std[:, zero])
        assert not same_bits(out[:, ~zero], std[:, ~zero])
        check_metrics(out, met, "hot")


def test_equal_inputs_give_equal_bits_at_every_n_maps(b2, torch):
    equal_bits_at_every_n_maps(b2, torch, "g65x45")


def test_equal_inputs_give_equal_bits_with_a_last_block_of_31_pulses(b2, torch):
    equal_bits_at_every_n_maps(b2, torch, "g95x64")  # and a last row group of 31 rows


def equal_bits_at_every_n_maps(b2, torch, geom):
    dims, x, y, stride, R = inputs(b2, geom, 3, seed=55)
    amb = handle(b2, geom)
    amb.set_migration(MS.tables(dims, 4)["physical"])
    maps, _, _ = process(torch, b2, amb, x, y, stride, 3)
    a, ma = migrate(torch, amb, maps, 3, False)
    b, mb = migrate(torch, amb, maps, 3, False)
    one, m1 = migrate(torch, amb, maps, 1, False)
    assert same_bits(a, b) and np.array_equal(ma.view(np.uint64), mb.view(np.uint64))
    assert same_bits(one[0], a[0]) and np.array_equal(m1[0].view(np.uint64), ma[0].view(np.uint64))
    c, mc = migrate(torch, amb, maps, 3, True)  # in place, last: it overwrites the process call's maps
    assert same_bits(c, a) and np.array_equal(mc.view(np.uint64), ma.view(np.uint64))


# ---- 3. metrics -------------------------------------------------------------------------------------------------------------
def test_metrics_with_a_peak_planted_along_a_walk(b2, torch):
    planted_peak(b2, torch, "g129x111", 3, 70)  # a migrated row, a column of the second strip


def test_metrics_with_a_peak_planted_in_the_last_row_group_and_the_third_strip(b2, torch):
    planted_peak(b2, torch, "g81x200", 80, 150)  # 81 rows: the last block has 17 pulses, the last row group 17 rows


def planted_peak(b2, torch, geom, row, col):
    dims = MS.dims_of(geom)
    nD, nC = dims.n_doppler_bins, dims.n_corr
    x, y, stride = MS.impulse_cpis(dims, 2, seed=9)
    h = MS.tables(dims, CELLS[geom])["physical"]
    s = b2.migration_shifts(h, nD)
    assert s[row, 0] != 0 and col + s[row].min() >= 0 and col + s[row].max() < dims.n_delay_bins
    i = np.arange(nD)
    w = np.exp(-2j * np.pi * ((i * ((row + nD // 2 + 1) % nD)) % nD) / nD)
    y = y.copy()
    y[stride + i * nC + col + s[row]] += (3.0 * np.conj(w)).astype(np.complex64)  # CPI 1: R[i][col + s] gains 3 conj(W)
    amb = handle(b2, geom)
    amb.set_migration(h)
    maps, _, _ = process(torch, b2, amb, x, y, stride, 2)
    out, met = migrate(torch, amb, maps, 2, True)
    assert np.unravel_index(np.argmax(np.abs(out[1])), out[1].shape) == (row, col)
    assert abs(out[1, row, col]) > 3.0 * nD - 4.0 * np.sqrt(nD)
    assert met[1, 1] > met[0, 1] + 5.0
    check_metrics(out, met, "planted")
    for c in range(2):
        noise, peak = MS.set_metrics64(out[c])
        print(f"planted peak {geom} ({row}, {col}), map {c}: noisePower off by {abs(met[c, 0] - noise):.2e} dB, maxPower by {abs(met[c, 1] - peak):.2e} dB")


# ---- 4. several channels ----------------------------------------------------------------------------------------------------
def test_two_channels_of_two_cpis(b2, torch):
    geom, K, n_cpi = "g65x44", 2, 2
    dims = MS.dims_of(geom)
    nD, nDelay = MS.SHAPES[geom]
    used = nD * dims.n_corr
    x, y0, stride = MS.impulse_cpis(dims, n_cpi, seed=31, gap=5)
    _, y1, _ = MS.impulse_cpis(dims, n_cpi, seed=32, gap=5)
    h = MS.tables(dims, 4)["physical"]
    amb = handle(b2, geom)
    amb.set_migration(h)
    dx, dys = upload(torch, x), [upload(torch, y0), upload(torch, y1)]
    maps, met = Arena(torch, K * n_cpi * nD * nDelay * 2), Arena(torch, K * n_cpi * 4)
    amb.process_multi_dev(b2.FMT_C32, dx.data_ptr(), [d.data_ptr() for d in dys], n_cpi, stride, maps.ptr, met.ptr, stream_of(torch))
    torch.cuda.synchronize()
    out, om = migrate(torch, amb, maps, K * n_cpi, True)
    for k, yk in enumerate((y0, y1)):
        for c in range(n_cpi):
            seg = slice(c * stride, c * stride + used)
            ref = b2.migrate_maps(b2.range_map(dims, x[seg], yk[seg]), h)
            err = np.max(np.abs(out[k * n_cpi + c].astype(np.complex128) - ref)) / np.max(np.abs(ref))
            assert err <= PEAK_TOL, (k, c, err)
    check_metrics(out, om, "multi")


# ---- 5. the moving echo -----------------------------------------------------------------------------------------------------
def test_the_moving_echo_lands_on_its_mid_cpi_cell(b2, torch):
    dims = MS.scene_dims()
    x, y = MS.scene()
    x32, y32 = x.astype(np.complex64), y.astype(np.complex64)
    h = b2.migration_table(dims, MS.scene_fc(dims))
    ref = b2.migrate_maps(b2.range_map(dims, x32, y32), h)
    amb = handle(b2, "scene")
    amb.set_migration(h)
    maps, _, std = process(torch, b2, amb, x32, y32, x32.size, 1)
    out, met = migrate(torch, amb, maps, 1, False)
    cell = (MS.SCENE_ROW, MS.SCENE_COL)
    assert np.unravel_index(np.argmax(np.abs(out[0])), out[0].shape) == cell
    got, want = MS.level_db(out[0], *cell), MS.level_db(ref, *cell)
    print(f"scene: device {got:.3f} dB, restatement {want:.3f} dB, standard map {MS.level_db(std[0], *cell):.1f} dB at the cell")
    assert abs(got - want) <= 0.01
    assert np.max(np.abs(out[0].astype(np.complex128) - ref)) <= PEAK_TOL * np.max(np.abs(ref))
    assert MS.level_db(std[0], *cell) < got - 10.0
    check_metrics(out, met, "scene")


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def refused(b2, call):
    from blah2_amd import _lib
    with pytest.raises(b2.Blah2HipError) as e:
        call()
    assert e.value.code == _lib.ERR_INVALID, e.value
    return True


def test_refusals_write_nothing(b2, torch):
    import ctypes as C
    from blah2_amd import _lib
    geom = "g65x44"
    dims, x, y, stride, R = inputs(b2, geom, 3, seed=100 + len(geom))
    nD, nDelay = MS.SHAPES[geom]
    words = nD * nDelay * 2
    h = MS.tables(dims, 4)["physical"]
    st = stream_of(torch)
    fresh = b2.Ambiguity(*MS.GEOMS[geom][0], True, max_batch=MAX_BATCH)
    out, met = Arena(torch, 3 * words), Arena(torch, 12)
    # the table
    L = _lib.load()
    buf = np.zeros(nD)
    assert L.blah2hip_migration_table(fresh._h, 1e8, None) == _lib.ERR_INVALID
    assert L.blah2hip_migration_table(None, 1e8, buf.ctypes.data_as(C.c_void_p)) == _lib.ERR_INVALID
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert refused(b2, lambda: fresh.migration_table(bad))
    for bad in (np.nan, np.inf):
        t = h.copy()
        t[5] = bad
        assert refused(b2, lambda: fresh.set_migration(t))
    t = h.copy()
    t[0] = (MS.MAX_MIGRATION + 0.6) / (nD - 1)
    assert refused(b2, lambda: fresh.set_migration(t))
    t[0] = -(MS.MAX_MIGRATION + 0.6) / (nD - 1)
    assert refused(b2, lambda: fresh.set_migration(t))
    # no table; no process call yet
    assert refused(b2, lambda: fresh.migrate_dev(None, 1, out.ptr, met.ptr, st))
    fresh.set_migration(h)
    assert refused(b2, lambda: fresh.migrate_dev(None, 1, out.ptr, met.ptr, st))
    maps, _, std = process(torch, b2, fresh, x, y, stride, 2)
    fresh.set_migration(None)
    assert refused(b2, lambda: fresh.migrate_dev(maps.ptr, 1, out.ptr, met.ptr, st))  # cleared
    fresh.set_migration(h)
    # n_maps 0 or above the last call's two; NULL outputs; alignment; overlaps
    assert refused(b2, lambda: fresh.migrate_dev(maps.ptr, 0, out.ptr, met.ptr, st))
    assert refused(b2, lambda: fresh.migrate_dev(maps.ptr, 3, out.ptr, met.ptr, st))
    assert refused(b2, lambda: fresh.migrate_dev(maps.ptr, 1, None, met.ptr, st))
    assert refused(b2, lambda: fresh.migrate_dev(maps.ptr, 1, out.ptr, None, st))
    assert refused(b2, lambda: fresh.migrate_dev(maps.ptr + 4, 1, out.ptr, met.ptr, st))
    assert refused(b2, lambda: fresh.migrate_dev(maps.ptr, 1, out.ptr + 4, met.ptr, st))
    assert refused(b2, lambda: fresh.migrate_dev(maps.ptr, 2, maps.ptr + 8, met.ptr, st))            # partial overlap
    assert refused(b2, lambda: fresh.migrate_dev(maps.ptr, 2, maps.ptr + 4 * words, met.ptr, st))    # ... by one map
    assert refused(b2, lambda: fresh.migrate_dev(maps.ptr, 1, out.ptr, maps.ptr + 64, st))           # metrics inside the input
    assert refused(b2, lambda: fresh.migrate_dev(maps.ptr, 1, out.ptr, out.ptr + 64, st))            # ... inside the output
    torch.cuda.synchronize()
    assert out.untouched() and met.untouched()
    assert same_bits(maps.read(maps.words).view(np.complex64).reshape(std.shape), std)
    # and the call that is allowed still works on this handle
    got, _ = migrate(torch, fresh, maps, 2, True)
    ref = b2.migrate_maps(R[:2], h)
    assert np.max(np.abs(got.astype(np.complex128) - ref)) <= PEAK_TOL * np.max(np.abs(ref))
    fresh.close()
