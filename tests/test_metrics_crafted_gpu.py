"""GPU: the Map::set_metrics epilogue of every Doppler kernel form on maps whose peak moves (tests/metrics_crafted.py).

Every case goes through Ambiguity.process_dev (case 6: process_multi_dev) on batches of 7 .. 12 CPIs, one planted target per
CPI, no direct path, the form forced and asserted with last_doppler_kernel(), every persistent form on a grid of 3 or 5
workgroups (doppler_tilew2_kernel: its 32) so that each walks three tiles or more and crosses CPI boundaries, map and metrics
in guarded allocations.  Gates on every CPI: assert_cpi of tests/test_timed_kernels_gpu.py against the fp64 oracle (1e-5 of
the peak, 1e-4 cell-wise, 1e-3 dB), and ``WRITTEN_DB_GATE`` on |noisePower - n'| and |maxPower - m'| against
(n', m') = oracle.map_metrics of the map the device returned.  tests/test_metrics_crafted_model.py shows what the second
gate is worth: a planted cell lost or counted twice, a padding column let in, a max carried over or started elsewhere, a
stale partial each miss it ten times over.

Cases: 1. the descending batch on every form at every Doppler length of its class and three windows (25 columns: ragged
tiles 16 + 9 / 3 x 8 + 1 / 6 x 4 + 1 and 8-byte stores; 26: 16-byte stores; 3: fewer columns than any tile); 2. the mirrored
batch; 3. samples scaled by 1e-6, every cell below 0 dB, maxPower == -noisePower bit for bit; 4. one CPI in the middle with
an all-zero surveillance channel (noisePower -inf, maxPower +inf, its neighbours untouched), then the handle again on the
ordinary batch; 5. one handle through tile8, a lone CPI on sub4, tile16 on one CPI fewer, column; 6. two surveillance
channels; 7. hot columns and leak compensation forced (oracle gates only: both rewrite cells after the partials are taken).

Measured on the MI355X (metrics_crafted.FIGURES, per form): noisePower within 4.1e-6 dB and maxPower within 1.22e-5 dB of the
written map's, in every form alike; no epilogue was wrong.  The map gate found one thing: doppler_dft_kernel (`direct`) at
nD = 2049 left the rows next to a planted peak 1.0e-4 of their own value off, its one running fp32 sum; it now sums in
blocks of 32 pulses.

Every case prints its worst figures."""
import numpy as np
import pytest

import metrics_crafted as MC
from test_timed_kernels_gpu import CELL_TOL, DB_TOL, PEAK_TOL, assert_cpi

pytestmark = pytest.mark.gpu

assert (PEAK_TOL, CELL_TOL, DB_TOL) == (1e-5, 1e-4, 1e-3)
assert MC.WRITTEN_DB_GATE <= MC.WRITTEN_DB_CAP
GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces


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


def handle(b2, g, max_batch, features="off"):
    amb = b2.Ambiguity(*MC.args_of(g), True, max_batch=max_batch, n_doppler_bins=g.nD if g.explicit else 0)
    assert amb.get_n_doppler_bins() == g.nD and amb.get_n_delay_bins() == MC.dims_of(g).n_delay_bins
    amb.set_hot_columns(features)
    amb.set_leak_compensation(features)
    return amb


def launch(b2, amb, form, grid, xs, ys, extra_ys=None):
    """One process_dev (process_multi_dev with ``extra_ys``: a second channel) of fp32 planes on ``amb``.  Returns
    (maps [CPIs, nD, nDelay] complex64, metrics [CPIs, 2]); channel-major with two channels."""
    import torch
    from blah2_amd import _lib
    B, n = len(xs), xs[0].shape[0]
    amb.set_doppler_kernel(form)
    amb.set_doppler_grid(grid)
    x = torch.from_numpy(np.stack(xs).astype(np.complex64)).cuda()
    planes = [torch.from_numpy(np.stack(v).astype(np.complex64)).cuda() for v in ([ys] if extra_ys is None else [ys, extra_ys])]
    V = B * len(planes)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    wo, out = guarded(torch, (V, nD, nC), torch.complex64)
    wm, met = guarded(torch, (V, 2), torch.float64)
    st = torch.cuda.current_stream().cuda_stream
    if extra_ys is None:
        amb.process_dev(b2.FMT_C32, x.data_ptr(), planes[0].data_ptr(), B, n, out.data_ptr(), met.data_ptr(), st)
    else:
        amb.process_multi_dev(b2.FMT_C32, x.data_ptr(), [p.data_ptr() for p in planes], B, n, out.data_ptr(), met.data_ptr(), st)
    torch.cuda.synchronize()
    assert guard_intact(wo) and guard_intact(wm)
    assert amb.last_doppler_kernel() == form, f"Doppler kernel that ran: {amb.last_doppler_kernel()}"
    if form in MC.PERSISTENT and grid:
        used = amb.info(_lib.INFO_DOPPLER_GRID)
        assert used == (max(32, (grid + 31) & ~31) if form == "tilew2" else min(grid, amb.info(_lib.INFO_DOPPLER_TILES))), used
    return out.cpu().numpy(), met.cpu().numpy()


def gate(got, met, refs, tag, form, written=True, zero_cpi=None):
    """Both gates on every CPI; prints the worst figures before it asserts.  Returns (worst |dn|, worst |dm|) against
    written_metrics."""
    figs = []
    for c, ref in enumerate(refs):
        if c == zero_cpi:
            continue
        wn, wm = MC.written_metrics(got[c])
        figs.append((abs(met[c, 0] - wn), abs(met[c, 1] - wm)))
    worst = (max(f[0] for f in figs), max(f[1] for f in figs))
    print(f"\n[{tag}] against written_metrics: noisePower {worst[0]:.2e} dB, maxPower {worst[1]:.2e} dB (gate {MC.WRITTEN_DB_GATE:.1e})  #fig {form} {worst[0]:.3e} {worst[1]:.3e}")
    for c, ref in enumerate(refs):
        if c == zero_cpi:
            assert not got[c].any(), f"{tag} cpi {c}: the map of an all-zero channel is not zero"
            assert met[c, 0] == -np.inf and met[c, 1] == np.inf, f"{tag} cpi {c}: metrics {met[c]} of an all-zero map"
            continue
        assert np.isfinite(met[c]).all(), f"{tag} cpi {c}: metrics {met[c]}"
        assert_cpi(got[c], met[c], ref, f"{tag} cpi {c}")
    if written:
        k = 0
        for c in range(len(refs)):
            if c == zero_cpi:
                continue
            dn, dm = figs[k]
            k += 1
            assert dn <= MC.WRITTEN_DB_GATE and dm <= MC.WRITTEN_DB_GATE, \
                f"{tag} cpi {c}: metrics {met[c]} against those of the written map: noisePower off by {dn:.3e} dB, maxPower by {dm:.3e} dB"
    return worst


def steady(amb, form):
    from blah2_amd import _lib
    tiles, grid = amb.info(_lib.INFO_DOPPLER_TILES), amb.info(_lib.INFO_DOPPLER_GRID)
    assert tiles >= 3 * grid > 0, f"{form}: {tiles} tiles on {grid} workgroups"


def run_case(b2, case, features="off"):
    g = MC.geom(case.nD, case.window)
    b = MC.batch_of(case)
    amb = handle(b2, g, len(b["refs"]), features)
    got, met = launch(b2, amb, case.form, case.grid, b["xs"], b["ys"])
    return amb, b, got, met


# ---- 1. / 2. the ladders ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MC.DESCENDING + MC.ASCENDING, ids=[MC.case_id(c) for c in MC.DESCENDING + MC.ASCENDING])
def test_planted_peak_walks_the_batch(b2, case):
    amb, b, got, met = run_case(b2, case)
    if case.form in MC.PERSISTENT and case.window != "w3" and case.grid != 8:
        steady(amb, case.form)  # (tests/test_metrics_crafted_model.py: the tables hold such a case for every persistent form)
    amb.close()
    gate(got, met, b["refs"], MC.case_id(case), case.form)


# ---- 3. every cell below 0 dB -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MC.SMALL_CASES, ids=[MC.case_id(c) for c in MC.SMALL_CASES])
def test_small_samples_leave_the_max_at_its_start(b2, case):
    amb, b, got, met = run_case(b2, case)
    amb.close()
    gate(got, met, b["refs"], MC.case_id(case), case.form)
    assert (10 * np.log10(np.abs(got.astype(np.complex128)).max())) < 0
    assert np.array_equal(met[:, 1].view(np.uint64), (-met[:, 0]).view(np.uint64)), met.tolist()


# ---- 4. an all-zero CPI in the middle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MC.ZERO_CASES, ids=[MC.case_id(c) for c in MC.ZERO_CASES])
def test_all_zero_cpi_in_the_middle_of_a_batch(b2, case):
    g = MC.geom(case.nD, case.window)
    z = MC.zero_cpi_of(g)
    amb, b, got, met = run_case(b2, case)
    gate(got, met, b["refs"], MC.case_id(case), case.form, zero_cpi=z)
    plain = MC.batch(g)  # the same handle again: nothing of the -inf is left in a partial, a ticket or a slot of LDS
    got, met = launch(b2, amb, case.form, case.grid, plain["xs"], plain["ys"])
    amb.close()
    gate(got, met, plain["refs"], MC.case_id(case) + " again, ordinary CPIs", case.form)


# ---- 5. one handle, four forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nD", [65, 513])
def test_handle_reuse_across_forms(b2, nD):
    """The partial slots of one handle under forms whose part counts differ (4 half tiles, 7 pieces, 2 tiles, 32 columns
    per CPI): tile8 on B CPIs, a lone CPI on sub4, tile16 on B - 1, column on B."""
    g = MC.geom(nD)
    b = MC.batch(g)
    B = len(b["refs"])
    amb = handle(b2, g, B)
    for form, grid, lo, hi in (("tile8", 3, 0, B), ("sub4", 0, B - 1, B), ("tile16", 5, 1, B), ("column", 0, 0, B)):
        got, met = launch(b2, amb, form, grid, b["xs"][lo:hi], b["ys"][lo:hi])
        gate(got, met, b["refs"][lo:hi], f"reuse-{nD} {form} CPIs {lo}..{hi - 1}", form)
    amb.close()


# ---- 6. two surveillance channels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nD,form", [(513, "tile16"), (1027, "tilew4")])
def test_two_surveillance_channels(b2, nD, form):
    g = MC.geom(nD)
    a, b = MC.batch(g), MC.batch(g, channel=1)
    B = len(a["refs"])
    amb = handle(b2, g, 2 * B)
    got, met = launch(b2, amb, form, 5, a["xs"], a["ys"], extra_ys=b["ys"])
    steady(amb, form)
    amb.close()
    gate(got[:B], met[:B], a["refs"], f"multi-{nD} {form} channel 0", form)
    gate(got[B:], met[B:], b["refs"], f"multi-{nD} {form} channel 1", form)


# ---- 7. hot columns and leak compensation forced --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MC.FEATURE_CASES, ids=[MC.case_id(c) for c in MC.FEATURE_CASES])
def test_hot_columns_and_leak_compensation_always(b2, case):
    amb, b, got, met = run_case(b2, case, features="always")
    amb.close()
    gate(got, met, b["refs"], MC.case_id(case), case.form, written=False)
