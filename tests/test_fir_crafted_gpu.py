"""GPU: the fused FIR range kernel (range_fir_kernel, csrc/kernels.hpp) on crafted taps and forced grids, against the fp64
oracle chain (tests/fir_crafted.py: the oracle's filter with GIVEN taps, then oracle.blah2_oracle.ambiguity_process).

Every run: transform length 4096, the taps from a device tensor (Ambiguity.set_fir(tensor, delay_min)), a batch of distinct
census CPIs -- one of them with an all-zero surveillance channel, so that its map is the filter term alone -- at input stride
n + 5 with the gaps and the planes' surroundings filled with samples of modulus 1000, taps, map and metrics in guarded
allocations, hot columns and leak compensation off (one case repeats a row with both at their defaults), RANGE_FIR asserted.
Gate: max|M - ref| <= 1e-5 max|ref| per CPI (PEAK_TOL of tests/test_timed_kernels_gpu.py); every planted product is at least
1.9e-3 of the peak and each wrong edge handling moves the map by 1.9e-2 of it or more (tests/test_fir_crafted_model.py), so one
lost, extra or misplaced product misses the gate by 190 times.  Map::set_metrics is compared wherever the reference map has no
zero cell (the dense scene); a census map has columns no pair reaches, whose cells are rounding noise in any implementation.

What runs: every row of fir_crafted.GEOMS (pulse ends on, 5 past, 5 short of a block boundary, the shortest pulse, five
blocks, |delayMin| = 0, 1, 8, 24, 260, `head` reaching block 1) with the largest tap at lag 0 and strong taps at every
anticipatory index and at the window's end; the largest tap at index 0, at another anticipatory index (the `tail` loop's
skip), at nBins - 1, at 255 / 256 / 2047 / 2048, twice, nowhere (all zero), alone; four classes of it in one batch; filters
of 1, |delayMin|, nDelay - 101, 600 and 2049 taps; int16 words; the pulse walk forced to 1, 4 and 5 workgroups (bit-identical
to the natural grid, CPI by CPI); a dense noise scene under twelve multipath taps; and the launcher's acceptance boundaries,
each met and missed by one.

Measured on the MI355X, worst err / peak over the file (FIGURES below): 3.9e-6 for fp32 planes and for int16 words alike, on
the row with 263 pulses; 6.3e-7 on every other row (4.5e-7 with taps; the larger figure is the all-zero set, whose peak is the
plain y x* term alone); 2.8e-7 on the dense scene.  The forced grids, the repeated CPI and the two sample formats of the dense
scene reproduce the natural grid's bits.  No case came within a factor of two of the gate: the kernel was wrong nowhere.

Every case prints its worst err / peak."""
import numpy as np
import pytest

import fir_crafted as FC
from oracle import blah2_oracle as O
from test_timed_kernels_gpu import CELL_TOL, PEAK_TOL, assert_cpi

pytestmark = pytest.mark.gpu

assert PEAK_TOL == 1e-5 and CELL_TOL == 1e-4
GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces
DB_TOL = 1e-3
# A cell of the fp64 reference that no planted pair reaches is not 0.0 but the rounding of its transforms, below 1e-12 of the
# peak (tests/test_fir_crafted_model.py: the FFT form against the sparse sums); a cell that a pair reaches is a sum of
# multiples of 1/8.  Below this fraction of the peak a reference cell counts as a zero cell
ZERO_CELL = 1e-9

# worst err / peak per sample format over this file's census and boundary cases, and over the dense scene (MI355X); a record
# of what was measured, not a bound: every case is held to PEAK_TOL
FIGURES = {"FMT_C32": 3.878e-06, "FMT_I16": 3.878e-06, "FMT_C32 without the 263-pulse row": 6.277e-07,
           "FMT_I16 without the 263-pulse row": 3.142e-07, "dense": 2.761e-07}


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


def guarded(torch, shape, dtype, pad=64):
    words = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size() // 4
    whole = torch.full((words + pad,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    return whole, whole[:words].view(dtype).view(shape)


def guard_intact(whole, pad=64):
    return bool((whole[-pad:].cpu().numpy().view(np.uint32) == GUARD).all())


def run(b2, g, xs, ys, w, fmt_name="FMT_C32", grid=0, features="off"):
    """One process_dev call on a fresh handle.  Returns (maps [B, nD, nDelay] complex64, metrics [B, 2], workgroups)."""
    import torch
    from blah2_amd import _lib
    B, n = len(xs), xs[0].shape[0]
    fmt = getattr(b2, fmt_name)
    amb = b2.Ambiguity(*FC.args_of(g), True, max_batch=B)
    amb.set_fft_len(4096)
    assert amb.dims.fft_len == 4096 and amb.dims.n_samples == n
    assert (amb.get_n_doppler_bins(), amb.get_n_corr()) == (2 * g.f_max + 1, g.n_corr)
    if features == "off":
        amb.set_hot_columns("off")
        amb.set_leak_compensation("off")
    if grid:
        amb.set_range_grid(grid)
    w32 = torch.from_numpy(np.ascontiguousarray(w, dtype=np.complex64))
    assert np.array_equal(w32.numpy().astype(np.complex128), w), "the taps are not exact in fp32"
    ww, wt = guarded(torch, w.shape, torch.complex64)
    wt.copy_(w32)
    assert amb.fir_fusable(w.shape[1], fmt, g.delay_min) is None and amb.fir_fusable(wt, fmt, g.delay_min) is None
    amb.set_fir(wt, g.delay_min)
    stride = n + FC.IN_GAP
    hx, hy, off = FC.host_planes(fmt_name, xs, ys, stride)
    tx = torch.from_numpy(hx).cuda()
    px = tx.data_ptr() + off * hx.itemsize * (hx.size // hx.shape[0])
    ty, py = None, None
    if hy is not None:
        ty = torch.from_numpy(hy).cuda()
        py = ty.data_ptr() + off * hy.itemsize
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    wo, out = guarded(torch, (B, nD, nC), torch.complex64)
    wm, met = guarded(torch, (B, 2), torch.float64)
    amb.process_dev(fmt, px, py, B, stride, out.data_ptr(), met.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert guard_intact(wo) and guard_intact(wm) and guard_intact(ww)
    assert torch.equal(wt.cpu(), w32), "the taps were written"
    assert amb.info(_lib.INFO_LAST_RANGE_KERNEL) == _lib.RANGE_FIR
    used_grid = amb.info(_lib.INFO_RANGE_GRID)
    got, m = out.cpu().numpy(), met.cpu().numpy()
    amb.set_fir(None)
    amb.close()
    assert not np.isnan(m).any(), f"NaN in the metrics {m.tolist()}"
    return got, m, used_grid


def gate(got, met, refs, tag, tol=PEAK_TOL):
    """The peak gate on every CPI (prints every CPI's err / peak before it asserts), and the metrics where the reference map
    has no zero cell.  Returns the worst err / peak."""
    ratios, where = [], []
    for c, ref in enumerate(refs):
        m = got[c].astype(np.complex128)
        assert np.isfinite(m.view(np.float64)).all(), f"{tag} cpi {c}: NaN or Inf in the map"
        peak = np.abs(ref).max()
        if peak == 0:  # no taps and no surveillance channel
            assert not m.any(), f"{tag} cpi {c}: the reference map is zero"
            ratios.append(0.0)
            where.append(None)
            continue
        err = np.abs(m - ref)
        ratios.append(float(err.max() / peak))
        where.append(tuple(int(v) for v in np.unravel_index(np.argmax(err), err.shape)))
    print(f"\n[{tag}] worst err / peak {max(ratios):.3e} (gate {tol:.3e}); per CPI, with its (row, column): "
          + " ".join(f"{r:.3e} {w}" for r, w in zip(ratios, where)))
    for c, r in enumerate(ratios):
        assert r <= tol, f"{tag} cpi {c}: err / peak {r:.3e} > {tol:.3e} at (row, column) {where[c]}"
    for c, ref in enumerate(refs):
        if np.abs(ref).min() > ZERO_CELL * np.abs(ref).max():
            noise, mx = O.map_metrics(ref)
            print(f"[{tag}] cpi {c} metrics - reference: noise {met[c, 0] - noise:+.2e} dB, peak {met[c, 1] - mx:+.2e} dB")
            assert abs(met[c, 0] - noise) <= DB_TOL and abs(met[c, 1] - mx) <= DB_TOL, f"{tag} cpi {c}: metrics {met[c]} vs {(noise, mx)}"
    return max(ratios)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def run_case(b2, case, fmt_name="FMT_C32", **kw):
    name, cls, nb = case
    g = FC.GEOM_BY_NAME[name]
    b = FC.batch(g, cls, nb, B=4 if cls == "mixed" else 3)
    got, met, grid = run(b2, g, b["xs"], b["ys"], b["w"], fmt_name, **kw)
    k0 = [FC.k0_of(r) for r in b["w"]]
    worst = gate(got, met, b["refs"], f"{FC.case_id(case)} {fmt_name} k0 {k0} grid {grid}")
    return got, met, grid, worst


# ---- 1. every row, every tap set, the filter lengths ------------------------------------------------------------------------
@pytest.mark.parametrize("case", FC.CASES, ids=[FC.case_id(c) for c in FC.CASES])
def test_fused_kernel_on_the_census(b2, case):
    run_case(b2, case)


@pytest.mark.parametrize("name", ["min-pulse", "past-5", "head-block1", "wide-dmin"])
def test_int16_words(b2, name):
    run_case(b2, (name, "a", None), "FMT_I16")


def test_hot_columns_and_leak_compensation_at_their_defaults(b2):
    run_case(b2, ("past-5", "a", None), features="default")


# ---- 2. the pulse walk ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", [("past-5", 3), ("dmin1", 4)])
def test_forced_grids_give_the_natural_grids_bits(b2, name, B):
    """1, 4 and 5 workgroups walk 63 (20) pulses of 3 (4) CPIs: every workgroup runs three pulses or more, crosses CPI
    boundaries (1 workgroup: every one of them) and reloads H, w and k0 there (the largest tap sits elsewhere in every CPI); 4 and 5 are coprime to 21, so a workgroup's
    pulses change their place in the CPI.  The kernel has no atomics and a pulse's arithmetic does not depend on which
    workgroup runs it: the maps and the metrics are the natural grid's, bit for bit."""
    g = FC.GEOM_BY_NAME[name]
    b = FC.batch(g, "mixed", None, B=B)
    assert len({FC.k0_of(r) for r in b["w"]}) == 3  # the largest tap moves from CPI to CPI
    pulses = B * (2 * g.f_max + 1)
    nat, nat_met, nat_grid = run(b2, g, b["xs"], b["ys"], b["w"])
    assert nat_grid >= pulses
    gate(nat, nat_met, b["refs"], f"{name} B {B} natural grid {nat_grid}")
    for grid in (1, 4, 5):
        assert pulses >= 3 * grid
        got, met, used = run(b2, g, b["xs"], b["ys"], b["w"], grid=grid)
        assert used == grid
        worst = gate(got, met, b["refs"], f"{name} B {B} forced grid {grid}: {-(-pulses // grid)} pulses per workgroup")
        for c in range(B):
            assert np.array_equal(bits(got[c]), bits(nat[c])), f"{name} grid {grid} cpi {c}: the map differs from the natural grid's (err / peak {worst:.3e})"
            assert np.array_equal(bits(met[c]), bits(nat_met[c])), f"{name} grid {grid} cpi {c}: metrics"


@pytest.mark.parametrize("grid", [0, 4])
def test_the_same_cpi_at_batch_positions_0_and_2(b2, grid):
    g = FC.GEOM_BY_NAME["past-5"]
    b = FC.batch(g, "a")
    xs, ys = [b["xs"][0], b["xs"][1], b["xs"][0]], [b["ys"][0], b["ys"][1], b["ys"][0]]
    w = np.stack([b["w"][0], b["w"][1], b["w"][0]])
    got, met, _ = run(b2, g, xs, ys, w, grid=grid)
    gate(got, met, [b["refs"][0], b["refs"][1], b["refs"][0]], f"past-5 CPI 0 at positions 0 and 2, grid {grid}")
    assert np.array_equal(bits(got[0]), bits(got[2])) and np.array_equal(bits(met[0]), bits(met[2]))
    assert not np.array_equal(bits(got[0]), bits(got[1]))


# ---- 3. the dense complement ------------------------------------------------------------------------------------------------
def test_dense_scene_under_multipath_taps(b2):
    """int16-valued noise through twelve taps of modulus 0.1 .. 0.6 per CPI, anticipatory ones included: the H V path with
    many strong taps at once, cell by cell (assert_cpi: peak gate, CELL_TOL on the cells above the mean, metrics), on the
    natural grid and on 5 workgroups."""
    g = FC.GEOM_BY_NAME["past-5"]
    d = FC.dims_of(g)
    B = 2
    w = FC.multipath_taps(g, B)
    xy = [FC.dense_scene(g, 70 + c) for c in range(B)]
    xs, ys = [v[0] for v in xy], [v[1] for v in xy]
    refs = [FC.reference(d, xs[c], ys[c], w[c], g.delay_min) for c in range(B)]
    runs = {}
    for grid in (0, 5):
        for fmt_name in ("FMT_C32", "FMT_I16"):
            got, met, used = run(b2, g, xs, ys, w, fmt_name, grid=grid)
            assert grid == 0 or used == grid
            worst = gate(got, met, refs, f"dense past-5 {fmt_name} grid {used}")
            for c in range(B):
                assert_cpi(got[c], met[c], refs[c], f"dense past-5 {fmt_name} grid {used} cpi {c}")
            runs[(grid, fmt_name)] = got
    for fmt_name in ("FMT_C32", "FMT_I16"):
        assert np.array_equal(bits(runs[(0, fmt_name)]), bits(runs[(5, fmt_name)]))


# ---- 4. the acceptance boundaries -------------------------------------------------------------------------------------------
G = FC.GEOM_BY_NAME
BOUNDARIES = {  # name: (accepted case, refused row, refused n_bins, what the refusal says)
    "nCorr 2056 | 2055 at delayMin -8": (("min-pulse", "a", None), G["min-pulse"]._replace(n_corr=2055), 308, "shorter"),
    "spare 8 | 7": (("min-pulse", "a", None), G["min-pulse"]._replace(spare=7), 308, "look-ahead"),
    "one anticipatory tap, spare 1 | 0": (("dmin1", "a", None), G["dmin1"]._replace(spare=0), 41, "look-ahead"),
    "2049 | 2050 taps": (("dmin0", "d", 2049), G["dmin0"], 2050, "2049 taps"),
    "|delayMin| | |delayMin| - 1 taps": (("past-5", "a", 8), G["past-5"], 7, "reach lag 0"),
    "2049 | 2050 delay bins": (("dmin0", "a", None), G["dmin0"]._replace(delay_max=2049), 2049, "2049 delay bins"),
}


@pytest.mark.parametrize("name", list(BOUNDARIES))
def test_acceptance_boundaries(b2, name):
    import torch
    from blah2_amd import _lib
    case, bad, nb, why = BOUNDARIES[name]
    run_case(b2, case)  # the accepted side runs and passes the map gate
    d = FC.dims_of(bad)
    assert (d.n_corr, d.n_samples - d.n_doppler_bins * d.n_corr) == (bad.n_corr, bad.spare)
    assert FC.unfusable(d, nb, bad.delay_min) is not None
    amb = b2.Ambiguity(*FC.args_of(bad), True, max_batch=1)
    amb.set_fft_len(4096)
    assert amb.dims.fft_len == 4096
    for fmt in (b2.FMT_C32, b2.FMT_I16):
        assert why in amb.fir_fusable(nb, fmt, bad.delay_min), amb.fir_fusable(nb, fmt, bad.delay_min)
    wt = torch.zeros((1, nb), dtype=torch.complex64, device="cuda")
    x = torch.zeros(d.n_samples, dtype=torch.complex64, device="cuda")
    amb.set_fir(wt, bad.delay_min)
    with pytest.raises(b2.Blah2HipError) as e:
        amb.process_dev(b2.FMT_C32, x.data_ptr(), x.data_ptr(), 1, d.n_samples)
    assert e.value.code == _lib.ERR_UNSUPPORTED and why in str(e.value), str(e.value)
    amb.set_fir(None)  # the handle stays usable
    amb.process_dev(b2.FMT_C32, x.data_ptr(), x.data_ptr(), 1, d.n_samples)
    torch.cuda.synchronize()
    amb.close()


def test_more_cpis_than_rows_of_taps_is_refused(b2):
    """process_dev's CPI-count check uses the tensor's row count."""
    import torch
    g = FC.GEOM_BY_NAME["dmin1"]
    n = FC.dims_of(g).n_samples
    amb = b2.Ambiguity(*FC.args_of(g), True, max_batch=3)
    amb.set_fft_len(4096)
    wt = torch.zeros((2, 41), dtype=torch.complex64, device="cuda")
    amb.set_fir(wt, g.delay_min)
    x = torch.zeros(3 * n, dtype=torch.complex64, device="cuda")
    with pytest.raises(b2.Blah2HipError) as e:
        amb.process_dev(b2.FMT_C32, x.data_ptr(), x.data_ptr(), 3, n)
    assert "holds taps for 2" in str(e.value)
    amb.process_dev(b2.FMT_C32, x.data_ptr(), x.data_ptr(), 2, n)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        amb.set_fir(wt.cpu(), g.delay_min)
    with pytest.raises(ValueError):
        amb.set_fir(wt.to(torch.complex128), g.delay_min)
    amb.close()
