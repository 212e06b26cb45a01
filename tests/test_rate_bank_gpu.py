"""GPU: walk_sum_kernel<4, 2> (blah2hip_doppler_rate / blah2hip_amb_set_rates / blah2hip_amb_rate_bank_dev, Ambiguity.doppler_rate /
set_rates / rate_bank_dev) on the impulse-reference CPIs of tests/migrate_scenes.py and the accelerating scene of
tests/rate_scenes.py, in the guarded arenas of tests/test_migrate_gpu.py.  tests/test_rate_bank_model.py shows on the CPU that
the gate used here tells the kernel's arithmetic from every wrong chirp (sign, centre, denominator, origin, none, half the rate).

No reference counterpart; the checks are
  * cells, per cell and with no cell exempt: with kg the device's index and M_ref[k] = rate_bank_maps(range_map(x, y), q, h)'s
    hypotheses, ``|out - M_ref[kg]| <= PEAK_TOL peak`` and ``|M_ref[kg]| >= max_k |M_ref[k]| - 2 PEAK_TOL peak`` (the device may
    pick another of two hypotheses whose levels its fp32 sums cannot tell apart, never a weaker one), hot columns and leak
    compensation off.  Five geometries with banks of 5 and 16 (65 x 44; 65 x 45; 129 x 111, two column strips and nine row
    groups; the even 64 bins; asymmetric Doppler limits) and 2049 x 40 with a bank of 3; single hypotheses at +-0.5 and +-3,
    -2 .. 2, 16 unevenly spaced rates up to +-nD/4, a bank with duplicates whose later copies the index never names; no table,
    the physical one, ``limit`` and ``jagged``.  Nine more cases on the geometries off the grid of 32 pulses (21 x 64, 48 x 65,
    81 x 200, 95 x 64, 7 x 64: row groups of 5, 15, 1 and 7 live rows, blocks of 7 .. 31 pulses), whose reach
    tests/test_rate_bank_model.py proves.  3 CPIs a call (one at 2049 x 40, whose fp64 restatement takes seconds per CPI)
    with NaN gaps between the planes' CPIs, in place and out of place, the outputs between guard words, the maps behind
    n_maps untouched, every index below K, the metrics within 1e-3 dB of fp64 Map::set_metrics of the device's own output;
  * bits: bank {0} with no table is the process call's maps (hot columns and leak compensation forced on); bank {0} with a
    table is migrate_dev's maps, at 65 x 45 and at 95 x 64 (a block of 31 pulses, runs of fewer than 32); two calls give the same bits; map 0 of a call of one map is map 0 of a call of three; a
    single-hypothesis bank {q} equals a larger bank's cells wherever that bank's index names q;
  * the index plane: NULL is accepted and changes no map bit; a peak planted on a chirped walk is named by its rate;
  * process_multi_dev with 2 channels x 2 CPIs;
  * the accelerating scene (bank -7 .. 7: the library's banks end at 16): argmax (62, 23), the index there names q = +6, the level
    within 0.01 dB of the restatement's;
  * every BLAH2HIP_ERR_INVALID case of the three calls, with nothing written and the set bank left as it was;
  * BLAH2HIP_INFO_RATE_GRID = ceil(nDelay / 64) ceil(nD / 16) after every launch.

Measured on the MI355X (printed by the tests).  Cells, largest error over the peak from the named hypothesis: 2.0e-7 .. 6.5e-7 on
the maps of 64 .. 129 rows, 1.5e-6 at 2049 x 40, the same in place and out of place; the named hypothesis at most 3.8e-9 of the
peak below the strongest (0 in most cases: the device and the restatement name the same one).  Metrics with the planted peak:
noisePower 5.7e-7 dB, maxPower 1.7e-6 dB from fp64 set_metrics of the device's own cells.  Scene: 61.444 dB on the device and in
the restatement, 45.5 dB at that cell of the standard map.  As in the migration tests, the scene's direct path does not pass
the hot-column test with both options forced on (0 columns rewritten): the bit checks hold whatever wrote the cells.
Off the grid of 32 pulses: 1.7e-7 .. 3.3e-7 of the peak from the named hypothesis on the nine new cases (largest: 48 x 65, ``dup``,
``limit``), the named hypothesis at most 1.5e-8 of the peak below the strongest, the same in place and out of place; bank {0} is
migrate_dev bit for bit at 95 x 64 under ``physical`` and ``jagged``; the planted peak at (80, 150) of 81 x 200 is named by its
rate, noisePower 4.9e-7 dB, maxPower 1.1e-6 dB.  A library built with the rows of a partial last group on the last row's walk
passed every case from before and failed 21 x 64 ``jagged``, 95 x 64 ``limit``, 7 x 64 ``physical`` and both bank-{0} cases at
95 x 64.  No defect was found.
"""
import numpy as np
import pytest

import migrate_scenes as MS
import rate_scenes as RS
from test_migrate_gpu import Arena, GUARD, MAX_BATCH, check_metrics, handle, inputs, process, refused, same_bits, stream_of, upload
from test_timed_kernels_gpu import PEAK_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def bank_call(torch, amb, maps, n_maps, in_place, want_index=True):
    """rate_bank_dev on the arena of a process call -> (out [n_maps, nD, nC], index [n_maps, nD, nC] or None, metrics [n_maps, 2])."""
    from blah2_amd import _lib
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    words = n_maps * nD * nC * 2
    before = maps.read(maps.words)
    dst = maps if in_place else Arena(torch, words)
    met = Arena(torch, n_maps * 4)
    idx_words = -(-n_maps * nD * nC // 4)
    idx = Arena(torch, idx_words) if want_index else None
    amb.rate_bank_dev(maps.ptr, n_maps, dst.ptr, idx.ptr if idx else None, met.ptr, stream_of(torch))
    torch.cuda.synchronize()
    assert amb.info(_lib.INFO_RATE_GRID) == -(-nC // 64) * -(-nD // 16)
    after = maps.read(maps.words)
    if in_place:
        assert np.array_equal(after[words:], before[words:]), "a map behind n_maps was written"
    else:
        assert np.array_equal(after, before), "the input maps were written"
    out = (after if in_place else dst.read(dst.words))[:words].view(np.complex64).reshape(n_maps, nD, nC)
    index = None
    if idx:
        raw, n = idx.read(idx_words).view(np.uint8), n_maps * nD * nC
        guard = np.tile(np.frombuffer(GUARD.tobytes(), np.uint8), idx_words)
        assert np.array_equal(raw[n:], guard[n:]), "written behind the index plane, inside its last word"
        index = raw[:n].reshape(n_maps, nD, nC).copy()
    return out, index, met.read(n_maps * 4).view(np.float64).reshape(n_maps, 2)


def banks(nD):
    return {"p0.5": [0.5], "m0.5": [-0.5], "p3": [3.0], "m3": [-3.0], "m2to2": [-2.0, -1.0, 0.0, 1.0, 2.0],
            "uneven16": RS.uneven_bank(nD), "dup": [0.5, -1.0, 0.5, 2.0, -1.0], "three": [-3.0, 0.0, 0.5]}


def table_of(dims, geom, name):
    return None if name == "none" else MS.tables(dims, CELLS[geom])[name]


_refs = {}


def reference(b2, geom, n_cpi, seed, bank, table):
    """rate_bank_maps of a case's CPIs, once."""
    key = (geom, n_cpi, seed, bank, table)
    if key not in _refs:
        dims, x, y, stride, R = inputs(b2, geom, n_cpi, seed)
        _refs[key] = b2.rate_bank_maps(R, banks(dims.n_doppler_bins)[bank], table_of(dims, geom, table))
    return _refs[key]


def check_cells(out, index, every, tag):
    K = every.shape[0]
    assert np.isfinite(out.view(np.float32)).all() and (index < K).all(), tag
    mag = np.abs(every)
    peak = mag.max()
    named = np.take_along_axis(every, index[None].astype(np.int64), axis=0)[0]
    err = np.max(np.abs(out.astype(np.complex128) - named)) / peak
    short = np.max(mag.max(axis=0) - np.abs(named)) / peak
    print(f"rate bank {tag}: {err:.2e} of the peak from the named hypothesis, which is at most {short:.2e} of the peak below the strongest")
    assert err <= PEAK_TOL, (tag, err)
    assert short <= 2 * PEAK_TOL, (tag, short)


# ---- 1. cells ---------------------------------------------------------------------------------------------------------------
CELLS = MS.CELLS
CASES = [("g65x44", "m2to2", "none"), ("g65x44", "uneven16", "physical"), ("g65x44", "p0.5", "limit"), ("g65x44", "m3", "jagged"),
         ("g65x44", "dup", "physical"),
         ("g65x45", "m2to2", "physical"), ("g65x45", "uneven16", "jagged"), ("g65x45", "m0.5", "none"),
         ("g129x111", "m2to2", "limit"), ("g129x111", "uneven16", "none"), ("g129x111", "p3", "physical"),
         ("g64x44", "m2to2", "jagged"), ("g64x44", "uneven16", "limit"),
         ("gasym", "m2to2", "physical"), ("gasym", "uneven16", "none"),
         ("g2049x40", "three", "physical")]
# Doppler lengths off the 32-pulse grid; tests/test_rate_bank_model.py shows which block, run and window edges each of them runs
CASES += MS.EDGE_RATE_CASES


@pytest.mark.parametrize("geom,bank,table", CASES, ids=[f"{g}-{b}-{t}" for g, b, t in CASES])
def test_cells_against_the_restatement(b2, torch, geom, bank, table):
    n_cpi = 1 if geom == "g2049x40" else 3
    seed = 100 + len(geom)
    dims, x, y, stride, R = inputs(b2, geom, n_cpi, seed)
    amb = handle(b2, geom)
    nD = dims.n_doppler_bins
    q = np.asarray(banks(nD)[bank], dtype=np.float64)
    assert q.size == {"uneven16": 16, "m2to2": 5, "dup": 5, "three": 3}.get(bank, 1)
    if bank == "uneven16":
        assert np.abs(q).max() == nD / 4.0 and np.unique(q).size == 16
    _, _, every = reference(b2, geom, n_cpi, seed, bank, table)
    amb.set_migration(table_of(dims, geom, table))
    amb.set_rates(q)
    for in_place in (True, False):
        maps, _, std = process(torch, b2, amb, x, y, stride, n_cpi)
        out, index, met = bank_call(torch, amb, maps, n_cpi, in_place)
        check_cells(out, index, every, f"{geom} {bank} {table} in_place={in_place}")
        if bank == "dup":
            assert not np.isin(index, (2, 4)).any(), "the index names the later copy of a duplicate"
            assert all((index == k).any() for k in (0, 1, 3))
        check_metrics(out, met, (geom, bank, table))
    amb.set_rates(None)
    amb.set_migration(None)


# ---- 2. bits ----------------------------------------------------------------------------------------------------------------
def test_the_bank_of_zero_without_a_table_is_the_process_call(b2, torch):
    from blah2_amd import _lib
    amb = handle(b2, "scene", hot=_lib.LEAK_ALWAYS, leak=_lib.LEAK_ALWAYS)
    x, y = MS.scene()
    y = y + 0.8 * x  # a direct path: the zero-delay column is hot
    x32, y32 = x.astype(np.complex64), y.astype(np.complex64)
    amb.set_migration(None)
    amb.set_rates([0.0])
    for in_place in (True, False):
        maps, met0, std = process(torch, b2, amb, x32, y32, x32.size, 1)
        print(f"hot columns rewritten: {amb.hot_columns()}")
        out, index, met = bank_call(torch, amb, maps, 1, in_place)
        assert same_bits(out, std) and not index.any()
        check_metrics(out, met, "zero")
    # with a table the zero-shift rows still are, and the others are migrate_dev's
    dims = MS.scene_dims()
    h = b2.migration_table(dims, MS.scene_fc(dims))
    zero = MS.zero_rows(h, dims.n_doppler_bins)
    amb.set_migration(h)
    maps, _, std = process(torch, b2, amb, x32, y32, x32.size, 1)
    out, _, _ = bank_call(torch, amb, maps, 1, False)
    assert same_bits(out[:, zero], std[:, zero]) and not same_bits(out[:, ~zero], std[:, ~zero])
    amb.set_rates(None)
    amb.set_migration(None)


# g95x64: the two kernels must add a block of 31 pulses, and under ``jagged`` runs of fewer than 32, in the same order
@pytest.mark.parametrize("geom,table", [("g65x45", "physical"), ("g65x45", "jagged"), ("g95x64", "physical"), ("g95x64", "jagged")],
                         ids=["physical", "jagged", "g95x64-physical", "g95x64-jagged"])
def test_the_bank_of_zero_with_a_table_is_migrate_dev(b2, torch, geom, table):
    dims, x, y, stride, R = inputs(b2, geom, 3, seed=55)
    amb = handle(b2, geom)
    amb.set_migration(MS.tables(dims, CELLS[geom])[table])
    amb.set_rates([0.0])
    maps, _, std = process(torch, b2, amb, x, y, stride, 3)
    assert (std.view(np.float32) != 0).all()  # no zero cells: c = (1, -0) keeps every bit
    mig, mm = Arena(torch, maps.words), Arena(torch, 12)
    amb.migrate_dev(maps.ptr, 3, mig.ptr, mm.ptr, stream_of(torch))
    torch.cuda.synchronize()
    want = mig.read(mig.words).view(np.complex64).reshape(std.shape)
    out, index, met = bank_call(torch, amb, maps, 3, False)
    assert same_bits(out, want) and not same_bits(out, std) and not index.any()
    assert np.array_equal(met.view(np.uint64), mm.read(12).view(np.uint64).reshape(3, 2))
    out2, _, _ = bank_call(torch, amb, maps, 3, True)
    assert same_bits(out2, want)
    amb.set_rates(None)
    amb.set_migration(None)


def test_equal_inputs_give_equal_bits(b2, torch):
    geom = "g65x45"
    dims, x, y, stride, R = inputs(b2, geom, 3, seed=55)
    nD = dims.n_doppler_bins
    amb = handle(b2, geom)
    amb.set_migration(MS.tables(dims, 4)["physical"])
    big = RS.uneven_bank(nD)
    amb.set_rates(big)
    maps, _, _ = process(torch, b2, amb, x, y, stride, 3)
    a, ia, ma = bank_call(torch, amb, maps, 3, False)
    b, ib, mb = bank_call(torch, amb, maps, 3, False)
    one, i1, m1 = bank_call(torch, amb, maps, 1, False)
    assert same_bits(a, b) and np.array_equal(ia, ib) and np.array_equal(ma.view(np.uint64), mb.view(np.uint64))
    assert same_bits(one[0], a[0]) and np.array_equal(i1[0], ia[0]) and np.array_equal(m1[0].view(np.uint64), ma[0].view(np.uint64))
    # NULL index plane: the same maps and metrics
    c, ic, mc = bank_call(torch, amb, maps, 3, False, want_index=False)
    assert ic is None and same_bits(c, a) and np.array_equal(mc.view(np.uint64), ma.view(np.uint64))
    # a hypothesis alone, at position 0, gives the bits it gives at its position in the bank (0: the zero rate, whose
    # candidates in zero-shift rows are the input cells; 5 and 14: the second and the first hypothesis of a pass)
    for k in (0, 5, 14):
        amb.set_rates([big[k]])
        s, i_s, _ = bank_call(torch, amb, maps, 3, False)
        sel = ia == k
        assert sel.any() and not i_s.any()
        assert np.array_equal(s.view(np.uint64)[sel], a.view(np.uint64)[sel]), k
    amb.set_rates(big)
    d, idd, md = bank_call(torch, amb, maps, 3, True)  # in place, last: it overwrites the process call's maps
    assert same_bits(d, a) and np.array_equal(idd, ia) and np.array_equal(md.view(np.uint64), ma.view(np.uint64))
    amb.set_rates(None)
    amb.set_migration(None)


# ---- 3. the index plane and the metrics ---------------------------------------------------------------------------------------
def test_a_peak_planted_on_a_chirped_walk_is_named_by_its_rate(b2, torch):
    planted_peak(b2, torch, "g129x111", 3, 70)  # a migrated row, a column of the second strip


def test_a_peak_planted_in_the_last_row_group_and_the_third_strip_is_named_by_its_rate(b2, torch):
    planted_peak(b2, torch, "g81x200", 80, 150)  # 81 rows: the last block has 17 pulses, the last row group is row 80 alone


def planted_peak(b2, torch, geom, row, col):
    dims = MS.dims_of(geom)
    nD, nC = dims.n_doppler_bins, dims.n_corr
    x, y, stride = MS.impulse_cpis(dims, 2, seed=9)
    h = MS.tables(dims, CELLS[geom])["physical"]
    s = b2.migration_shifts(h, nD)
    q = np.array([-2.0, -1.0, 0.0, 1.0, 2.0])
    k = 4  # the rate +2
    assert s[row, 0] != 0 and col + s[row].min() >= 0 and col + s[row].max() < dims.n_delay_bins
    i = np.arange(nD)
    w = np.exp(-2j * np.pi * ((i * ((row + nD // 2 + 1) % nD)) % nD) / nD)
    c = b2.rate_chirps(q, nD)[k]
    y = y.copy()
    y[stride + i * nC + col + s[row]] += (3.0 * np.conj(w * c)).astype(np.complex64)  # CPI 1: R[i][col + s] gains 3 conj(c W)
    amb = handle(b2, geom)
    amb.set_migration(h)
    amb.set_rates(q)
    maps, _, _ = process(torch, b2, amb, x, y, stride, 2)
    out, index, met = bank_call(torch, amb, maps, 2, True)
    assert np.unravel_index(np.argmax(np.abs(out[1])), out[1].shape) == (row, col)
    assert index[1, row, col] == k
    assert abs(out[1, row, col]) > 3.0 * nD - 4.0 * np.sqrt(nD)
    assert met[1, 1] > met[0, 1] + 5.0
    check_metrics(out, met, "planted")
    for m in range(2):
        noise, peak = MS.set_metrics64(out[m])
        print(f"planted peak {geom} ({row}, {col}), map {m}: noisePower off by {abs(met[m, 0] - noise):.2e} dB, maxPower by {abs(met[m, 1] - peak):.2e} dB")
    amb.set_rates(None)
    amb.set_migration(None)


# ---- 4. several channels ----------------------------------------------------------------------------------------------------
def test_two_channels_of_two_cpis(b2, torch):
    geom, K, n_cpi = "g65x44", 2, 2
    dims = MS.dims_of(geom)
    nD, nDelay = MS.SHAPES[geom]
    used = nD * dims.n_corr
    x, y0, stride = MS.impulse_cpis(dims, n_cpi, seed=31, gap=5)
    _, y1, _ = MS.impulse_cpis(dims, n_cpi, seed=32, gap=5)
    h = MS.tables(dims, 4)["physical"]
    q = [-2.0, -1.0, 0.0, 1.0, 2.0]
    amb = handle(b2, geom)
    amb.set_migration(h)
    amb.set_rates(q)
    dx, dys = upload(torch, x), [upload(torch, y0), upload(torch, y1)]
    maps, met = Arena(torch, K * n_cpi * nD * nDelay * 2), Arena(torch, K * n_cpi * 4)
    amb.process_multi_dev(b2.FMT_C32, dx.data_ptr(), [d.data_ptr() for d in dys], n_cpi, stride, maps.ptr, met.ptr, stream_of(torch))
    torch.cuda.synchronize()
    out, index, om = bank_call(torch, amb, maps, K * n_cpi, True)
    R = np.stack([b2.range_map(dims, x[c * stride:c * stride + used], yk[c * stride:c * stride + used]) for yk in (y0, y1) for c in range(n_cpi)])
    check_cells(out, index, b2.rate_bank_maps(R, q, h)[2], "2 channels x 2 CPIs")
    check_metrics(out, om, "multi")
    amb.set_rates(None)
    amb.set_migration(None)


# ---- 5. the accelerating echo -----------------------------------------------------------------------------------------------
def test_the_accelerating_echo_lands_on_its_mid_cpi_cell(b2, torch):
    dims = MS.scene_dims()
    x, y = RS.scene()
    x32, y32 = x.astype(np.complex64), y.astype(np.complex64)
    h = b2.migration_table(dims, MS.scene_fc(dims))
    bank = b2.rate_bank(7)
    assert bank.size == 15 and bank[13] == RS.SCENE_Q
    ref, ref_index, every = b2.rate_bank_maps(b2.range_map(dims, x32, y32), bank, h)
    amb = handle(b2, "scene")
    amb.set_migration(h)
    amb.set_rates(bank)
    maps, _, std = process(torch, b2, amb, x32, y32, x32.size, 1)
    out, index, met = bank_call(torch, amb, maps, 1, False)
    cell = (MS.SCENE_ROW, MS.SCENE_COL)
    assert np.unravel_index(np.argmax(np.abs(out[0])), out[0].shape) == cell
    assert index[0][cell] == 13 and ref_index[cell] == 13
    got, want = MS.level_db(out[0], *cell), MS.level_db(ref, *cell)
    print(f"scene: device {got:.3f} dB, restatement {want:.3f} dB, standard map {MS.level_db(std[0], *cell):.1f} dB at the cell")
    assert abs(got - want) <= 0.01
    check_cells(out, index, every[:, None], "scene")
    assert MS.level_db(std[0], *cell) < got - 10.0
    check_metrics(out, met, "scene")
    amb.set_rates(None)
    amb.set_migration(None)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(b2, torch):
    import ctypes as C
    from blah2_amd import _lib
    geom = "g65x44"
    dims, x, y, stride, R = inputs(b2, geom, 3, seed=100 + len(geom))
    nD, nDelay = MS.SHAPES[geom]
    words = nD * nDelay * 2
    st = stream_of(torch)
    fresh = b2.Ambiguity(*MS.GEOMS[geom][0], True, max_batch=MAX_BATCH)
    out, met, idx = Arena(torch, 3 * words), Arena(torch, 12), Arena(torch, 3 * words // 8 + 1)
    L = _lib.load()
    # doppler_rate
    one = C.c_double(7.0)
    assert L.blah2hip_doppler_rate(fresh._h, 1e8, 1.0, None) == _lib.ERR_INVALID
    assert L.blah2hip_doppler_rate(None, 1e8, 1.0, C.byref(one)) == _lib.ERR_INVALID
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert refused(b2, lambda: fresh.doppler_rate(bad, 1.0))
    for bad in (float("nan"), float("inf")):
        assert refused(b2, lambda: fresh.doppler_rate(1e8, bad))
    assert fresh.doppler_rate(204.64e6, -9.80665) == b2.doppler_rate(dims, 204.64e6, -9.80665) > 0  # the library's is the restatement's
    # no bank; no process call yet
    assert refused(b2, lambda: fresh.rate_bank_dev(None, 1, out.ptr, idx.ptr, met.ptr, st))
    fresh.set_rates([0.0, 1.0])
    assert refused(b2, lambda: fresh.rate_bank_dev(None, 1, out.ptr, idx.ptr, met.ptr, st))
    maps, _, std = process(torch, b2, fresh, x, y, stride, 2)
    for clear in (None, []):
        fresh.set_rates(clear)
        assert refused(b2, lambda: fresh.rate_bank_dev(maps.ptr, 1, out.ptr, idx.ptr, met.ptr, st))  # cleared
        fresh.set_rates([0.0, 1.0])
    # set_rates: too many, not finite, beyond nD -- and the set bank stays
    good = [-1.5, 2.5]
    fresh.set_rates(good)
    assert refused(b2, lambda: fresh.set_rates(np.linspace(-1, 1, RS.MAX_RATES + 1)))
    assert L.blah2hip_amb_set_rates(None, np.zeros(1).ctypes.data_as(C.c_void_p), 1) == _lib.ERR_INVALID
    for bad in (np.nan, np.inf, -np.inf, nD + 0.001, -(nD + 0.001)):
        assert refused(b2, lambda: fresh.set_rates([0.0, bad]))
    fresh.set_rates([float(nD), -float(nD)])  # the bound itself is allowed
    fresh.set_rates(good)
    # n_maps 0 or above the last call's two; NULL outputs; alignment; overlaps
    assert refused(b2, lambda: fresh.rate_bank_dev(maps.ptr, 0, out.ptr, idx.ptr, met.ptr, st))
    assert refused(b2, lambda: fresh.rate_bank_dev(maps.ptr, 3, out.ptr, idx.ptr, met.ptr, st))
    assert refused(b2, lambda: fresh.rate_bank_dev(maps.ptr, 1, None, idx.ptr, met.ptr, st))
    assert refused(b2, lambda: fresh.rate_bank_dev(maps.ptr, 1, out.ptr, idx.ptr, None, st))
    assert refused(b2, lambda: fresh.rate_bank_dev(maps.ptr + 4, 1, out.ptr, idx.ptr, met.ptr, st))
    assert refused(b2, lambda: fresh.rate_bank_dev(maps.ptr, 1, out.ptr + 4, idx.ptr, met.ptr, st))
    assert refused(b2, lambda: fresh.rate_bank_dev(maps.ptr, 2, maps.ptr + 8, idx.ptr, met.ptr, st))            # partial overlap
    assert refused(b2, lambda: fresh.rate_bank_dev(maps.ptr, 2, maps.ptr + 4 * words, idx.ptr, met.ptr, st))    # ... by one map
    assert refused(b2, lambda: fresh.rate_bank_dev(maps.ptr, 1, out.ptr, idx.ptr, maps.ptr + 64, st))           # metrics inside the input
    assert refused(b2, lambda: fresh.rate_bank_dev(maps.ptr, 1, out.ptr, idx.ptr, out.ptr + 64, st))            # ... inside the output
    assert refused(b2, lambda: fresh.rate_bank_dev(maps.ptr, 1, out.ptr, maps.ptr + 3, met.ptr, st))            # index inside the input
    assert refused(b2, lambda: fresh.rate_bank_dev(maps.ptr, 1, out.ptr, out.ptr + 4 * words - 1, met.ptr, st))  # ... on the output's last byte
    assert refused(b2, lambda: fresh.rate_bank_dev(maps.ptr, 1, out.ptr, met.ptr - 1, met.ptr, st))             # ... over the metrics
    torch.cuda.synchronize()
    assert out.untouched() and met.untouched() and idx.untouched()
    assert same_bits(maps.read(maps.words).view(np.complex64).reshape(std.shape), std)
    # and the call that is allowed still works on this handle, with the bank that the refused set_rates calls left alone
    got, index, _ = bank_call(torch, fresh, maps, 2, True)
    check_cells(got, index, b2.rate_bank_maps(R[:2], good)[2], "after the refusals")
    assert (index == 0).any() and (index == 1).any()
    fresh.close()
