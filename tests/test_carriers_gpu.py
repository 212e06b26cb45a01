"""GPU: multi-carrier integration (blah2hip_carrier_table / blah2hip_amb_set_carriers / blah2hip_amb_fuse_carriers_dev:
carrier_sum_kernel) through the C ABI, into guarded planes: a NaN-payload guard word on both sides, the maps 8 bytes off a
16-byte boundary as well as on one.  No reference counterpart; the check is the fp64 NumPy restatement
``blah2_amd.fuse_carriers`` WITH THE DEVICE'S OWN TABLE, cell by cell with none exempt.  Inputs are integrate_crafted.maps,
where every cell differs.  Geometries, the smallest at which the tile logic (64 columns x 8 rows, two rows a wave) can go
wrong, on the handles of tests/test_tracks_gpu.py: 21 x 111 (an odd cell count), 21 x 112, 48 x 64 (every tile whole), 48 x 65
(a strip of one live lane), and one case at 513 x 411.  The CPU proof of what the gate catches is tests/test_carriers_model.py.

Bounds
  * cells: ``|out - ref| <= (C + 8) 2^-24 ref``, derived, not measured: at most 4 roundings up to q, one per carrier in S,
    one for the scale -- first-order relative errors on non-negative terms, halved by the square root -- plus at most 2
    units for sqrtf (include/blah2hip.h); the imaginary parts are exactly zero.
  * metrics: 1e-3 dB (the project's DB_TOL) against fp64 Map::set_metrics of the device's OWN output cells.
  * bits: all ratios 1 against blah2hip_nci_process_dev at W = 1; a map alone against the same map in a batch of 5; either
    placement.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import integrate_crafted as IC

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces
PAD = 64
MAX_BATCH = 40  # 8 carriers x 5 CPIs
SMALL = (-10, 100, -100, 100, 1_000_000, 100_000)    # 21 x 111
EVEN = (-10, 101, -100, 100, 1_000_000, 100_000)     # 21 x 112
CFG2 = (-10, 400, -256, 256, 2_000_000, 2_000_000)   # 513 x 411
WHOLE = (0, 63, -160, 160, 200_000, 40_000)          # 48 x 64 with 48 explicit bins
LONE = (0, 64, -160, 160, 200_000, 40_000)           # 48 x 65 with 48 explicit bins
BINS = {WHOLE: 48, LONE: 48}
GEOMS = {"21x111": SMALL, "21x112": EVEN, "48x64": WHOLE, "48x65": LONE}
DB_TOL = 1e-3
RATIO_SETS = {
    "ones": (1.0,),
    "physical": (1.0, 1.004, 0.996, 1.02),
    "exaggerated": (1.0, 1.25, 0.8, 1.1),
    "clamped": (1.0, 2.0, 0.5),
}
WEIGHTS = (1.0, 0.25, 4.0, 2.0, 0.5, 1.0, 3.0, 0.125)
INTERPS = ("nearest", "linear")


def ratios(name, n):
    r = RATIO_SETS[name]
    return [r[c % len(r)] for c in range(n)]


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


_handles = {}


def handle(b2, geom, max_batch=MAX_BATCH):
    if geom not in _handles:
        _handles[geom] = b2.Ambiguity(*geom, True, max_batch=max_batch, n_doppler_bins=BINS.get(geom, 0))
    return _handles[geom]


def shape_of(amb):
    return amb.get_n_doppler_bins(), amb.get_n_delay_bins()


def guarded(torch, shape, dtype, off_bytes=0):
    """(whole, view): ``shape`` of ``dtype`` between guard words, the view ``off_bytes`` behind a 256-byte boundary."""
    item = torch.empty(0, dtype=dtype).element_size()
    nbytes = int(np.prod(shape)) * item
    assert nbytes % 4 == 0 and off_bytes % 4 == 0
    words = nbytes // 4
    lead = PAD + off_bytes // 4
    whole = torch.full((lead + words + PAD,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    assert whole.data_ptr() % 256 == 0
    view = whole[lead:lead + words].view(torch.uint8)[:nbytes].view(dtype).view(shape)
    return whole, view


def guards_intact(whole, n_words, off_bytes=0):
    w = whole.cpu().numpy().view(np.uint32)
    lead = PAD + off_bytes // 4
    return bool((w[:lead] == GUARD).all() and (w[lead + n_words:] == GUARD).all())


def untouched(whole):
    return bool((whole.cpu().numpy().view(np.uint32) == GUARD).all())


def fuse(torch, amb, maps, w=None, off=0):
    """``maps`` complex64 [C, n_cpi, nD, nC] along the table set on ``amb`` -> (out complex64 [n_cpi, nD, nC], metrics
    [n_cpi, 2]); input and outputs between guards, the maps ``off`` bytes behind a 256-byte boundary."""
    nD, nC = shape_of(amb)
    n_cpi = maps.shape[1]
    win, d_in = guarded(torch, maps.shape, torch.complex64, off)
    wo, out = guarded(torch, (n_cpi, nD, nC), torch.complex64, off)
    wm, met = guarded(torch, (n_cpi, 2), torch.float64)
    d_in.copy_(torch.from_numpy(np.ascontiguousarray(maps)))
    amb.fuse_carriers_dev(d_in.data_ptr(), n_cpi, out.data_ptr(), met.data_ptr(), w, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert guards_intact(win, maps.size * 2, off) and guards_intact(wo, out.numel() * 2, off) and guards_intact(wm, n_cpi * 4)
    assert np.array_equal(d_in.cpu().numpy().view(np.uint32), np.ascontiguousarray(maps).view(np.uint32))  # the input is only read
    return out.cpu().numpy(), met.cpu().numpy()


def set_metrics64(z):
    """Map::set_metrics (Map.cpp:187-206) in fp64."""
    with np.errstate(divide="ignore"):
        db = 10.0 * np.log10(np.abs(z.astype(np.complex128)))
    noise = db.mean()
    return noise, max(0.0, db.max()) - noise


def gate(b2, out, met, maps, table, w, tag):
    """Every cell against the restatement under the derived bound, zero imaginary parts, the metrics of the device's own cells.
    Returns the largest error over the bound."""
    C_ = maps.shape[0]
    ref = b2.fuse_carriers(maps, table, w)
    assert out.shape == ref.shape and (out.imag == 0).all() and np.isfinite(out.real).all(), tag
    rel = np.abs(out.real.astype(np.float64) - ref) / ((C_ + 8) * 2.0 ** -24 * ref)
    assert (rel <= 1.0).all(), (tag, float(rel.max()))
    for i in range(out.shape[0]):
        noise, peak = set_metrics64(out[i])
        assert abs(met[i, 0] - noise) <= DB_TOL and abs(met[i, 1] - peak) <= DB_TOL, (tag, i, met[i], noise, peak)
    return float(rel.max())


_inputs = {}


def crafted(shape, seed=11):
    """integrate_crafted.maps for 8 carriers and 5 CPIs of a geometry, made once; a case takes its leading carriers and CPIs."""
    if shape not in _inputs:
        _inputs[shape] = IC.maps(8, 5, shape[0], shape[1], seed)
    return _inputs[shape]


@pytest.mark.parametrize("geom", list(GEOMS))
def test_the_cross_of_cases(b2, torch, geom):
    amb = handle(b2, GEOMS[geom])
    nD, nC = shape_of(amb)
    assert f"{nD}x{nC}" == geom
    base, worst, n = crafted((nD, nC)), 0.0, 0
    for name, interp, C_ in itertools.product(RATIO_SETS, INTERPS, (1, 2, 3, 8)):
        r = ratios(name, C_)
        amb.set_carriers(r, interp)
        table = amb.carrier_table(r, interp)
        for n_cpi, w in itertools.product((1, 2, 5), (None, WEIGHTS[:C_])):
            maps = np.ascontiguousarray(base[:C_, :n_cpi])
            off = 8 * (n % 2)
            out, met = fuse(torch, amb, maps, w, off)
            worst = max(worst, gate(b2, out, met, maps, table, w, (geom, name, interp, C_, n_cpi, w is not None, off)))
            assert amb.info(b2._lib.INFO_CARRIER_GRID) == -(-nC // 64) * -(-nD // 8)
            n += 1
    print(f"{geom}: {n} cases, largest error / bound {worst:.3f}")
    assert n == 4 * 2 * 4 * 3 * 2


def test_a_large_map(b2, torch):
    amb = handle(b2, CFG2, max_batch=8)
    nD, nC = shape_of(amb)
    assert (nD, nC) == (513, 411)
    maps = IC.maps(3, 2, nD, nC, seed=12)
    r, w = ratios("physical", 3), WEIGHTS[:3]
    amb.set_carriers(r, "linear")
    out, met = fuse(torch, amb, maps, w, off=8)
    worst = gate(b2, out, met, maps, amb.carrier_table(r, "linear"), w, "513x411")
    print(f"513x411: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("geom", ["21x111", "48x65"])
def test_the_library_table_is_the_restatement(b2, geom):
    amb = handle(b2, GEOMS[geom])
    for name, interp, C_ in itertools.product(RATIO_SETS, INTERPS, (1, 3, 8)):
        mine, ref = amb.carrier_table(ratios(name, C_), interp), b2.carrier_table(amb.doppler, ratios(name, C_), interp)
        for k in ("row", "a_lo", "a_hi", "covered"):
            assert np.array_equal(mine[k], ref[k]) and mine[k].dtype == ref[k].dtype, (name, interp, C_, k)
    out = amb.carrier_table([1.0, 2.0], "nearest")
    assert out["covered"].min() == 1 and out["covered"].max() == 2


@pytest.mark.parametrize("interp", INTERPS)
def test_the_device_sums_along_the_table_the_host_reports(b2, torch, interp):
    """Row r of every map holds sqrt(r + 1), one carrier at a time with weight 1 and the others 0: the output's square is
    a_lo (row + 1) + a_hi (row + 2), which names the device's row and a_hi per (carrier, output row)."""
    amb = handle(b2, SMALL)
    nD, nC = shape_of(amb)
    r = ratios("exaggerated", 4)
    amb.set_carriers(r, interp)
    table = amb.carrier_table(r, interp)
    ramp = np.sqrt(np.arange(nD) + 1.0)[None, None, :, None] * np.ones((4, 1, 1, nC))
    maps = ramp.astype(np.complex64)
    for c in range(4):
        w = [1.0 if k == c else 0.0 for k in range(4)]
        out, _ = fuse(torch, amb, maps, w)
        power = out.real.astype(np.float64) ** 2
        want = (table["a_lo"][c].astype(np.float64) * (table["row"][c] + 1.0) +
                table["a_hi"][c].astype(np.float64) * np.minimum(table["row"][c] + 2.0, nD))
        assert np.all(np.abs(power[0] - want[:, None]) <= 4e-6 * want[:, None]), (interp, c)  # rows are 1 apart: 5 % at the top


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("C_", [1, 3, 8])
def test_all_ratios_one_gives_the_integrator_bits(b2, torch, C_, interp):
    amb = handle(b2, SMALL)
    nD, nC = shape_of(amb)
    maps = np.ascontiguousarray(crafted((nD, nC))[:C_, :5])
    amb.set_carriers([1.0] * C_, interp)
    st = torch.cuda.current_stream().cuda_stream
    for w in (None, WEIGHTS[:C_]):
        out, met = fuse(torch, amb, maps, w)
        integ = b2.MapIntegrator(amb, C_, 1, 1)
        d_in = torch.from_numpy(maps).cuda()
        d_out = torch.zeros((5, nD, nC), dtype=torch.complex64, device="cuda")
        d_met = torch.zeros((5, 2), dtype=torch.float64, device="cuda")
        n_out, _ = integ.process_dev(d_in.data_ptr(), 5, d_out.data_ptr(), d_met.data_ptr(), 5, w, st)
        torch.cuda.synchronize()
        integ.close()
        assert n_out == 5
        assert np.array_equal(out.view(np.uint32), d_out.cpu().numpy().view(np.uint32)), (C_, interp, w)
        assert np.allclose(met, d_met.cpu().numpy(), rtol=0, atol=DB_TOL)  # another thread mapping: the same values, not the same bits


@pytest.mark.parametrize("geom", ["21x111", "48x65"])
def test_a_map_alone_has_its_bits_in_a_batch_and_at_either_placement(b2, torch, geom):
    amb = handle(b2, GEOMS[geom])
    nD, nC = shape_of(amb)
    maps = np.ascontiguousarray(crafted((nD, nC))[:3, :5])
    amb.set_carriers(ratios("exaggerated", 3), "linear")
    out, met = fuse(torch, amb, maps, WEIGHTS[:3], off=0)
    out8, met8 = fuse(torch, amb, maps, WEIGHTS[:3], off=8)
    assert np.array_equal(out.view(np.uint32), out8.view(np.uint32)) and np.array_equal(met.view(np.uint64), met8.view(np.uint64))
    for i in range(5):
        one, met1 = fuse(torch, amb, np.ascontiguousarray(maps[:, i:i + 1]), WEIGHTS[:3], off=8 * (i % 2))
        assert np.array_equal(one[0].view(np.uint32), out[i].view(np.uint32)), i
        assert np.array_equal(met1[0].view(np.uint64), met[i].view(np.uint64)), i


@pytest.mark.parametrize("interp", INTERPS)
def test_a_nan_reaches_the_cells_whose_entries_read_it(b2, torch, interp):
    amb = handle(b2, LONE)
    nD, nC = shape_of(amb)
    r = ratios("clamped", 3)
    amb.set_carriers(r, interp)
    table = amb.carrier_table(r, interp)
    # (carrier, row, column): the bottom row of the carrier that is clamped there, a middle row of the compressed one, the
    # top row on the lone lane, a row of the reference carrier
    for c, row, col in ((1, 0, 5), (2, 24, 63), (1, nD - 1, 64), (0, 17, 0)):
        maps = np.ascontiguousarray(crafted((nD, nC))[:3, :2]).copy()
        maps[c, 1, row, col] = np.nan
        out, _ = fuse(torch, amb, maps, (1.0, 0.0, 2.0))  # a zero weight does not hide it: 0 x NaN
        reads = (table["row"][c] == row) | ((table["row"][c] == row - 1) & (table["a_hi"][c] != 0))
        want = np.zeros(out.shape, dtype=bool)
        want[1, reads, col] = True
        assert reads.any() and np.array_equal(np.isnan(out.real), want), (interp, c, row, col, int(reads.sum()))
        assert (out.imag == 0).all()


@pytest.mark.parametrize("at", [(1, 63), (2, 64), (7, 0), (8, 63), (47, 64)])
def test_metrics_with_the_peak_on_a_seam(b2, torch, at):
    """The strongest cell on the last lane of a wave's first strip, the first lane of the next strip under the next wave,
    either side of a workgroup's row seam, and on the lone lane of the last row."""
    amb = handle(b2, LONE)
    nD, nC = shape_of(amb)
    maps = np.ascontiguousarray(crafted((nD, nC))[:2, :2]).copy()
    maps[:, 1, at[0], at[1]] = 1e4
    amb.set_carriers([1.0, 1.0], "linear")
    out, met = fuse(torch, amb, maps)
    assert np.unravel_index(np.argmax(out[1].real), (nD, nC)) == at
    for i in range(2):
        noise, peak = set_metrics64(out[i])
        assert abs(met[i, 0] - noise) <= DB_TOL and abs(met[i, 1] - peak) <= DB_TOL, (at, i, met[i], noise, peak)
    assert met[1, 1] > met[0, 1] + 30.0


def test_the_internal_map_behind_a_process_call(b2, torch):
    amb = handle(b2, SMALL)
    nD, nC = shape_of(amb)
    C_, n_cpi, n = 3, 2, amb.get_n_samples()
    rng = np.random.default_rng(13)
    x, y = (torch.from_numpy((rng.standard_normal((C_ * n_cpi, n)) + 1j * rng.standard_normal((C_ * n_cpi, n))).astype(np.complex64)).cuda()
            for _ in range(2))
    st = torch.cuda.current_stream().cuda_stream
    d_map = torch.zeros((C_, n_cpi, nD, nC), dtype=torch.complex64, device="cuda")
    d_met = torch.zeros((C_ * n_cpi, 2), dtype=torch.float64, device="cuda")
    amb.process_dev(b2.FMT_C32, x.data_ptr(), y.data_ptr(), C_ * n_cpi, n, d_map.data_ptr(), d_met.data_ptr(), st)
    amb.process_dev(b2.FMT_C32, x.data_ptr(), y.data_ptr(), C_ * n_cpi, n, None, None, st)  # the same maps, in the handle
    r = ratios("physical", C_)
    amb.set_carriers(r, "linear")
    wo, out = guarded(torch, (n_cpi, nD, nC), torch.complex64)
    wm, met = guarded(torch, (n_cpi, 2), torch.float64)
    amb.fuse_carriers_dev(None, n_cpi, out.data_ptr(), met.data_ptr(), None, st)
    torch.cuda.synchronize()
    assert guards_intact(wo, out.numel() * 2) and guards_intact(wm, n_cpi * 4)
    maps = d_map.cpu().numpy()
    gate(b2, out.cpu().numpy(), met.cpu().numpy(), maps, amb.carrier_table(r, "linear"), None, "internal map")
    ref, ref_met = fuse(torch, amb, maps)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(met.cpu().numpy().view(np.uint64), ref_met.view(np.uint64))


def test_refusals_leave_outputs_and_guards_untouched(b2, torch):
    L, lib = b2.load(), b2._lib
    amb = b2.Ambiguity(*SMALL, True, max_batch=6)
    two = b2.Ambiguity(-10, 100, 0, 0, 1_000_000, 1000, True, max_batch=1)  # limits that hold one Doppler bin
    try:
        assert two.get_n_doppler_bins() == 1
        nD, nC = shape_of(amb)
        h, st = amb._h, torch.cuda.current_stream().cuda_stream
        win, d_in = guarded(torch, (2, 3, nD, nC), torch.complex64)
        wo, out = guarded(torch, (3, nD, nC), torch.complex64)
        wm, met = guarded(torch, (3, 2), torch.float64)
        snapshot = win.clone()

        def dbl(*v):
            return (C.c_double * len(v))(*v)

        def flt(*v):
            return (C.c_float * len(v))(*v)

        def refused(rc, code=lib.ERR_INVALID):
            torch.cuda.synchronize()
            assert rc == code, (rc, L.blah2hip_last_error())
            assert untouched(wo) and untouched(wm) and bool((win == snapshot).all())

        i, o, m = d_in.data_ptr(), out.data_ptr(), met.data_ptr()
        refused(L.blah2hip_amb_fuse_carriers_dev(h, i, 1, None, o, m, st))  # no table set
        row = np.full((2, nD), -7, dtype=np.int32)
        for args in ((None, 2, 0), (dbl(1, 1), 0, 0), (dbl(*[1.0] * 9), 9, 0), (dbl(1, float("nan")), 2, 0), (dbl(1, float("inf")), 2, 0),
                     (dbl(1, 0.49), 2, 0), (dbl(1, 2.01), 2, 0), (dbl(1, 1), 2, 2), (dbl(1, 1), 2, -1)):
            assert L.blah2hip_carrier_table(h, args[0], args[1], args[2], row.ctypes.data, None, None, None) == lib.ERR_INVALID, args
            assert (row == -7).all()
            if args[1] != 0:  # (0 carriers clears the table)
                assert L.blah2hip_amb_set_carriers(h, *args) == lib.ERR_INVALID, args
            refused(L.blah2hip_amb_fuse_carriers_dev(h, i, 1, None, o, m, st))  # ... and nothing was set
        assert L.blah2hip_carrier_table(two._h, dbl(1.0), 1, 0, None, None, None, None) == lib.ERR_INVALID  # n_doppler < 2
        assert L.blah2hip_amb_set_carriers(two._h, dbl(1.0), 1, 0) == lib.ERR_INVALID
        assert L.blah2hip_carrier_table(h, dbl(1.0, 1.25), 2, 1, None, None, None, None) == lib.OK  # every output may be NULL

        amb.set_carriers([1.0, 1.25], "linear")
        refused(L.blah2hip_amb_fuse_carriers_dev(h, i, 0, None, o, m, st))
        refused(L.blah2hip_amb_fuse_carriers_dev(h, i, 4, None, o, m, st))       # 2 x 4 above max_batch 6
        refused(L.blah2hip_amb_fuse_carriers_dev(h, i, 3, None, None, m, st))
        refused(L.blah2hip_amb_fuse_carriers_dev(h, i, 3, None, o, None, st))
        for w in (flt(1, -1), flt(1, float("nan")), flt(float("inf"), 1), flt(0, 0)):
            refused(L.blah2hip_amb_fuse_carriers_dev(h, i, 3, w, o, m, st))
        refused(L.blah2hip_amb_fuse_carriers_dev(h, i + 4, 1, None, o, m, st))   # off 8-byte alignment
        refused(L.blah2hip_amb_fuse_carriers_dev(h, i, 1, None, o + 4, m, st))
        cells = nD * nC * 8
        refused(L.blah2hip_amb_fuse_carriers_dev(h, i, 3, None, i, m, st))                    # in place
        refused(L.blah2hip_amb_fuse_carriers_dev(h, i, 3, None, i + 5 * cells, m, st))        # the output starts in the last input map
        refused(L.blah2hip_amb_fuse_carriers_dev(h, i, 3, None, o, i + 6 * cells - 16, st))   # the metrics end in it
        refused(L.blah2hip_amb_fuse_carriers_dev(h, i, 3, None, o, o + 8, st))                # the metrics inside the output
        assert L.blah2hip_amb_fuse_carriers_dev(None, i, 3, None, o, m, st) == lib.ERR_INVALID
        # cleared: refused again; then the good call writes exactly its outputs
        amb.set_carriers(None)
        refused(L.blah2hip_amb_fuse_carriers_dev(h, i, 3, None, o, m, st))
        amb.set_carriers([1.0, 1.25], "linear")
        d_in.copy_(torch.from_numpy(IC.maps(2, 3, nD, nC, seed=14)))
        amb.fuse_carriers_dev(i, 3, o, m, None, st)
        torch.cuda.synchronize()
        assert guards_intact(wo, out.numel() * 2) and guards_intact(wm, 12) and np.isfinite(out.cpu().numpy().real).all()
        with pytest.raises(ValueError):
            amb.fuse_carriers_dev(i, 3, o, m, (1.0, 1.0, 1.0), st)  # three weights for two carriers
    finally:
        amb.close()
        two.close()
