"""GPU: integration along tracks (blah2hip_nci_set_tracks / blah2hip_nci_process_tracks_dev: track_power_kernel and
track_sum_kernel).  No reference counterpart; the check is the fp64 NumPy restatement ``integrate_tracks``, cell by cell with
none exempt, against THE HYPOTHESIS THE DEVICE NAMES.  Inputs are integrate_crafted.maps (every cell differs) on the handles
of tests/test_integrate_gpu.py: 21 x 111 cells (an odd count: every other plane, in or out, sits 8 bytes off a 16-byte
boundary, and every other ring plane 4 bytes off an 8-byte one), 21 x 112, one case at 513 x 411 (hundreds of workgroups), and
two on handles with 48 explicit Doppler bins: 48 x 64, where every 64 x 8 tile of track_sum_kernel is whole, and 48 x 65, whose
second strip has one live lane.
The CPU proof of what these cases reach and catch is tests/test_tracks_model.py; tables and scene: tests/track_scenes.py.

Bounds
  * cells: ``|out - sqrt(scale S_k)| <= (n_surv W + 8) 2^-24 sqrt(scale S_k)`` for the k the device names, derived, not
    measured (include/blah2hip.h); the imaginary parts are exactly zero.
  * the choice: the named hypothesis's fp64 sum is at least ``1 - 2 (n_surv W + 8) 2^-24`` of the strongest -- twice the
    relative bound of a sum, which is what two fp32 sums that compare the other way round can be apart.  On the shared
    input, where no two hypotheses are that close, the index is the fp64 restatement's in every cell.
  * metrics: 1e-3 dB (the project's DB_TOL) against fp64 Map::set_metrics of the device's OWN output cells.

Measured on the MI355X (printed by the tests).  Largest cell error over the bound: 0.090 .. 0.196 on the cases at 21 and 513 rows;
0.177 at 48 x 64 (W = 5, ``seams``, the ring wrapping) and 0.145 at 48 x 65 (two channels, ``jagged``); the named hypothesis is
the strongest in every cell of every case.  No defect was found.
"""
import ctypes as C
import types

import numpy as np
import pytest

import integrate_crafted as IC
import track_scenes as TS

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces
PAD = 64
MAX_BATCH = 24
SMALL = (-10, 100, -100, 100, 1_000_000, 100_000)    # 21 x 111
EVEN = (-10, 101, -100, 100, 1_000_000, 100_000)     # 21 x 112
CFG2 = (-10, 400, -256, 256, 2_000_000, 2_000_000)   # configs[1]: 513 x 411
WHOLE = (0, 63, -160, 160, 200_000, 40_000)          # 48 x 64 with 48 explicit bins: every 64 x 8 tile of track_sum_kernel whole
LONE = (0, 64, -160, 160, 200_000, 40_000)           # 48 x 65 with 48 explicit bins: the second strip has one live lane
BINS = {WHOLE: 48, LONE: 48}                         # explicit Doppler bin counts; the other geometries take the limits' own
DB_TOL = 1e-3
BANKS = {
    1: (0.0,),
    2: (0.0, 1.0),
    3: TS.SHARED["q"],
    5: (-2.0, -1.0, 0.0, 1.0, 2.0),
    # fractions (ties of rint at 0.5 a), a duplicate pair (the lower index must win), no order
    16: (0.0, 0.37, -0.81, 1.0, -2.5, 1.25, 2.0, -1.75, 0.11, -0.043, 0.62, 1.0, 0.5, -0.5, -1.0, 1.0 / 3.0),
}
# (geometry, n_surv, W, H, CPIs per call, max_cpi, table, bank, weights): the calls follow each other on one integrator
CASES = [
    (SMALL, 1, 4, 1, (6,), 6, "alternating", 3, None),       # the shared input
    (SMALL, 1, 8, 1, (10,), 10, "zero", 1, None),
    (SMALL, 1, 8, 1, (10,), 10, "physical", 5, None),
    (SMALL, 1, 8, 3, (5, 5, 5), 5, "seams", 2, None),           # shifts of 65 cells: past the wave and the strip
    (SMALL, 1, 8, 1, (9,), 9, "beyond", 5, None),              # every older term leaves the map
    (SMALL, 1, 8, 1, (9,), 12, "jagged", 16, None),            # fractional and duplicate rates
    (SMALL, 1, 1, 1, (3, 3, 3), 3, "jagged", 5, None),         # W = 1: the ring is max_cpi planes and wraps at once
    (SMALL, 1, 2, 5, (4, 4, 4), 4, "jagged", 5, None),         # H > W
    (SMALL, 1, 16, 1, (3, 3, 3, 3, 3, 3, 3), 3, "seams", 2, None),  # a ring of 18 planes under 21 CPIs
    (SMALL, 3, 2, 1, (2, 3, 3), 4, "physical", 5, (1.0, 0.25, 4.0)),
    (EVEN, 2, 3, 2, (7,), 8, "jagged", 5, None),
    (CFG2, 1, 4, 1, (5,), 5, "physical", 2, None),
    (WHOLE, 1, 5, 1, (4, 4, 4), 4, "seams", 2, None),          # no partial tile anywhere; W mod 4 = 1; the ring wraps
    (LONE, 2, 3, 2, (7,), 8, "jagged", 5, None),               # a strip of one live lane
]
IDS = [f"{g[1] - g[0] + 1}cols-K{k}-W{w}-H{h}-{'_'.join(map(str, c))}of{mc}-{t}-bank{b}" + ("-w" if wt else "")
       for g, k, w, h, c, mc, t, b, wt in CASES]


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


def handle(b2, geom, bins=None):
    """The handle of a geometry's limits; ``bins`` is the explicit Doppler bin count (BINS' where not given, else 0)."""
    bins = BINS.get(geom, 0) if bins is None else bins
    if (geom, bins) not in _handles:
        _handles[geom, bins] = b2.Ambiguity(*geom, True, max_batch=MAX_BATCH, n_doppler_bins=bins)
    return _handles[geom, bins]


def shape_of(amb):
    return amb.get_n_doppler_bins(), amb.get_n_delay_bins()


def guarded(torch, shape, dtype, off_bytes=0):
    """(whole, view): ``shape`` of ``dtype`` between guard words, the view starting ``off_bytes`` (a multiple of 4) behind
    a 256-byte boundary."""
    item = torch.empty(0, dtype=dtype).element_size()
    nbytes = int(np.prod(shape)) * item
    words = (nbytes + 3) // 4
    lead = PAD + off_bytes // 4
    whole = torch.full((lead + words + PAD,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    view = whole[lead:lead + words].view(torch.uint8)[:nbytes].view(dtype).view(shape)
    return whole, view


def words_outside(whole, first_byte, n_bytes, off_bytes=0):
    """The guard words of ``whole`` that lie wholly outside the bytes [first_byte, first_byte + n_bytes) of its view."""
    w = whole.cpu().numpy().view(np.uint32)
    lead = PAD + off_bytes // 4
    keep = np.ones(w.size, dtype=bool)
    keep[lead + first_byte // 4: lead + (first_byte + n_bytes + 3) // 4] = False
    return w[keep]


def untouched(whole):
    return bool((whole.cpu().numpy().view(np.uint32) == GUARD).all())


def call(torch, amb, integ, maps, w=None, want_index=True, off=0):
    """The next maps.shape[1] CPIs of ``integ`` along its tracks, into guarded outputs with room for one map per CPI, the
    maps ``off`` bytes behind a 256-byte boundary -> (out complex64 [n_out, nD, nC], index uint8 or None, metrics [n_out, 2],
    first_end).  Nothing may be written outside the n_out maps."""
    nD, nC = shape_of(amb)
    n_cpi = maps.shape[1]
    wo, out = guarded(torch, (n_cpi, nD, nC), torch.complex64, off)
    wi, idx = guarded(torch, (n_cpi, nD, nC), torch.uint8)
    wm, met = guarded(torch, (n_cpi, 2), torch.float64)
    win, d_in = guarded(torch, maps.shape, torch.complex64, off)
    d_in.copy_(torch.from_numpy(np.ascontiguousarray(maps)))
    want_n, want_first = integ.count(n_cpi)
    n_out, first = integ.process_tracks_dev(d_in.data_ptr(), n_cpi, out.data_ptr(), idx.data_ptr() if want_index else None,
                                            met.data_ptr(), n_cpi, w, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (n_out, first) == (want_n, want_first)  # count() announces what the call reports
    cells = nD * nC
    assert (words_outside(wo, 0, n_out * cells * 8, off) == GUARD).all()
    assert (words_outside(wi, 0, n_out * cells if want_index else 0) == GUARD).all()
    assert (words_outside(wm, 0, n_out * 16) == GUARD).all()
    assert (words_outside(win, 0, maps.size * 8, off) == GUARD).all()
    return (out[:n_out].cpu().numpy(), idx[:n_out].cpu().numpy() if want_index else None, met[:n_out].cpu().numpy(), first)


def stream(torch, amb, integ, maps, cuts, w=None, want_index=True, off=0):
    """``maps`` through ``integ`` in calls of ``cuts`` CPIs -> (out, index, metrics) of all windows."""
    outs, idxs, mets, at = [], [], [], 0
    for cnt in cuts:
        o, i, m, _ = call(torch, amb, integ, maps[:, at:at + cnt], w, want_index, off)
        outs.append(o)
        idxs.append(i)
        mets.append(m)
        at += cnt
    assert at == maps.shape[1]
    return np.concatenate(outs), (np.concatenate(idxs) if want_index else None), np.concatenate(mets)


def set_metrics64(z):
    """Map::set_metrics (Map.cpp:187-206) in fp64."""
    db = 10.0 * np.log10(np.abs(z.astype(np.complex128)))
    noise = db.mean()
    return noise, max(0.0, db.max()) - noise


def check_against_named(b2, out, idx, met, maps, walk, q, w, K, W, H, tag):
    """Every cell against the fp64 restatement of the hypothesis the device names, the choice against the strongest, the
    metrics against the device's own cells.  Returns the restatement."""
    levels, index, sums = b2.integrate_tracks(maps, walk, q, w, W, H)
    wk = np.ones(K, dtype=np.float32) if w is None else np.asarray(w, dtype=np.float32)
    scale = float(np.float32(1.0 / (W * wk.astype(np.float64).sum())))
    assert out.shape == levels.shape and idx.shape == index.shape and out.shape[0] > 0, (tag, out.shape, levels.shape)
    assert (out.imag == 0).all() and np.isfinite(out.real).all(), tag
    assert (idx < len(q)).all(), tag
    bound = TS.bound(K, W)
    rel, _ = TS.named_error(out.real, idx, sums, scale)
    named = np.take_along_axis(sums, idx[None].astype(np.int64), axis=0)[0]
    print(f"{tag}: largest error / bound {float(rel.max() / bound):.3f}, "
          f"smallest named / strongest - 1 = {float((named / sums.max(axis=0)).min() - 1.0):.2e}")
    assert (rel <= bound).all(), (tag, float(rel.max() / bound))
    assert (named >= (1.0 - 2.0 * bound) * sums.max(axis=0)).all(), tag
    for i in range(out.shape[0]):
        noise, peak = set_metrics64(out[i])
        assert abs(met[i, 0] - noise) <= DB_TOL and abs(met[i, 1] - peak) <= DB_TOL, (tag, i, met[i], noise, peak)
    return levels, index, sums


_results = {}


def case_result(b2, torch, case):
    """Inputs and the device's outputs of a case: computed once, shared by the tests, left unchanged."""
    if case not in _results:
        geom, K, W, H, cuts, max_cpi, table, bank, w = case
        amb = handle(b2, geom)
        nD, nC = shape_of(amb)
        if geom in BINS:
            assert (nD, nC) == (BINS[geom], geom[1] - geom[0] + 1)
        if case == CASES[0]:
            maps, walk, q = TS.shared_input()
        else:
            maps = IC.maps(K, sum(cuts), nD, nC, seed=2000 + 100 * K + 10 * W + sum(cuts))
            walk, q = TS.tables(nD, nC)[table], np.array(BANKS[bank])
        integ = b2.MapIntegrator(amb, K, W, H)
        try:
            integ.set_tracks(walk, q, max_cpi)
            assert integ.n_rates == len(q)
            _, s = b2.track_tables(walk, q, W)
            assert amb.info(b2._lib.INFO_TRACK_MAX_SHIFT) == int(np.abs(s).max())
            out, idx, met = stream(torch, amb, integ, maps, cuts, w)
            assert amb.info(b2._lib.INFO_TRACK_GRID) == -(-nC // 64) * -(-nD // 8)
        finally:
            integ.close()
        _results[case] = (maps, walk, q, out, idx, met)
    return _results[case]


# ---- 1. cells, choice and metrics ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cells_choice_and_metrics(b2, torch, case):
    geom, K, W, H, cuts, max_cpi, table, bank, w = case
    maps, walk, q, out, idx, met = case_result(b2, torch, case)
    if geom is SMALL:
        assert maps[0, 0].size % 2 == 1  # the odd cell count the alignment cases rest on
    if len(cuts) > 1:
        assert sum(cuts) > W - 1 + max_cpi  # the ring wraps inside the test
    levels, index, sums = check_against_named(b2, out, idx, met, maps, walk, q, w, K, W, H, IDS[CASES.index(case)])
    if case == CASES[0]:  # no two hypotheses alike (tests/test_tracks_model.py): the index is the restatement's everywhere
        assert TS.closest_pair(sums) > 2 * TS.bound(K, W)
        assert np.array_equal(idx, index) and len(np.unique(idx)) == 3
    if table == "zero" and bank == 1:
        assert not idx.any()
    if table == "beyond":  # only the cell's own CPI is left of every window, under every hypothesis
        ends = b2.integrate_ends(sum(cuts), W, H)
        own = np.abs(maps[0, ends].astype(np.complex128)) * np.sqrt(float(np.float32(1.0 / W)))
        assert (np.abs(out.real - own) <= TS.bound(K, W) * own).all() and not idx.any()
    if bank == 16:  # rates 3 and 11 are equal: the lower index wins the tie
        assert not (idx == 11).any()


def test_top_and_bottom_rows_lose_the_terms_whose_rows_leave_the_map(b2, torch):
    maps, walk, q, out, idx, met = case_result(b2, torch, CASES[2])  # bank -2 .. 2, W = 8
    jr, _ = b2.track_tables(walk, q, 8)
    assert (jr[4, 1:, 0] < 0).all() and (jr[0, 1:, 20] < 0).all()  # rate +2 in row 0, rate -2 in row 20: the cell alone
    assert (jr[2] >= 0).all()
    _, _, sums = b2.integrate_tracks(maps, walk, q, None, 8, 1)
    p_new = np.abs(maps[0, 7].astype(np.complex128)) ** 2
    assert np.allclose(sums[4, 0, 0], p_new[0]) and np.allclose(sums[0, 0, 20], p_new[20])


# ---- 2. cuts, index plane, short calls, reset -----------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [SMALL, EVEN], ids=["odd-cells", "even-cells"])
def test_the_bits_do_not_depend_on_how_the_cpis_are_cut_into_calls(b2, torch, geom):
    K, W, H, n_cpi = 2, 3, 2, 7
    amb = handle(b2, geom)
    nD, nC = shape_of(amb)
    maps = IC.maps(K, n_cpi, nD, nC, seed=23)
    walk, q = TS.tables(nD, nC)["jagged"], np.array(BANKS[5])
    integ = b2.MapIntegrator(amb, K, W, H)
    try:
        integ.set_tracks(walk, q, 7)
        whole, widx, wmet = stream(torch, amb, integ, maps, (7,))
        assert whole.shape[0] == 3  # windows end at 2, 4, 6
        integ.reset()
        parts, pidx, pmet = stream(torch, amb, integ, maps, (1, 2, 1, 3))
        assert np.array_equal(parts.view(np.uint32), whole.view(np.uint32))
        assert np.array_equal(pidx, widx) and np.array_equal(pmet.view(np.uint64), wmet.view(np.uint64))
        # without an index plane, and with every map 8 bytes off a 16-byte boundary: the same bits
        integ.reset()
        again, none, amet = stream(torch, amb, integ, maps, (3, 4), want_index=False, off=8)
        assert none is None
        assert np.array_equal(again.view(np.uint32), whole.view(np.uint32)) and np.array_equal(amet.view(np.uint64), wmet.view(np.uint64))
        check_against_named(b2, whole, widx, wmet, maps, walk, q, None, K, W, H, f"cuts {nC} cols")
    finally:
        integ.close()


def test_short_calls_fill_the_window_and_reset_forgets(b2, torch):
    amb = handle(b2, SMALL)
    nD, nC = shape_of(amb)
    W = 8
    maps = IC.maps(1, 12, nD, nC, seed=31)
    walk, q = TS.tables(nD, nC)["physical"], np.array(BANKS[5])
    integ = b2.MapIntegrator(amb, 1, W, 1)
    try:
        integ.set_tracks(walk, q, 6)
        # n_cpi < W - 1, twice: nothing is due, nothing is written (call() checks every word), the CPIs count
        for at in (0, 3):
            out, idx, met, first = call(torch, amb, integ, maps[:, at:at + 3])
            assert out.shape[0] == 0 and first == W - 1
        out, idx, met, first = call(torch, amb, integ, maps[:, 6:12])
        assert out.shape[0] == 5 and first == 7
        levels, index, sums = check_against_named(b2, out, idx, met, maps, walk, q, None, 1, W, 1, "short calls")
        # reset: the next window needs W new CPIs and holds nothing of the old ones
        integ.reset()
        assert integ.count(6) == (0, 7)
        o1, _, _, _ = call(torch, amb, integ, maps[:, 4:10])
        o2, i2, m2, first = call(torch, amb, integ, maps[:, 10:12])
        assert o1.shape[0] == 0 and o2.shape[0] == 1 and first == 7
        check_against_named(b2, o2, i2, m2, maps[:, 4:12], walk, q, None, 1, W, 1, "after reset")
    finally:
        integ.close()


# ---- 3. NaN ---------------------------------------------------------------------------------------------------------------
def test_a_nan_cell_reaches_exactly_the_outputs_whose_tracks_pass_through_it(b2, torch):
    amb = handle(b2, SMALL)
    nD, nC = shape_of(amb)
    W, n_cpi = 4, 8
    maps = IC.maps(1, n_cpi, nD, nC, seed=41).copy()
    maps[0, 3, 9, 50] = complex(np.nan, 1.0)
    walk, q = TS.tables(nD, nC)["jagged"], np.array(BANKS[5])
    integ = b2.MapIntegrator(amb, 1, W, 1)
    try:
        integ.set_tracks(walk, q, n_cpi)
        out, idx, met, _ = call(torch, amb, integ, maps)
    finally:
        integ.close()
    levels, index, sums = b2.integrate_tracks(maps, walk, q, None, W, 1)
    # a NaN S_0 stays with index 0; a NaN S_k, k > 0, never wins: the NaN cells are those of hypothesis 0's tracks through the cell
    want = np.isnan(sums[0])
    assert np.array_equal(np.isnan(levels), want) and 1 <= want.sum() <= W
    assert np.array_equal(np.isnan(out.real), want) and (out.imag == 0).all()
    assert (idx[want] == 0).all()
    ok = ~want
    clean = np.where(np.isnan(sums), -1.0, sums)  # a NaN sum never wins: it is no candidate
    scale = float(np.float32(1.0 / W))
    named = np.take_along_axis(clean, idx[None].astype(np.int64), axis=0)[0]
    assert (named[ok] >= 0).all()  # no NaN hypothesis is named where S_0 is finite
    ref = np.sqrt(scale * named[ok])
    assert (np.abs(out.real[ok] - ref) <= TS.bound(1, W) * ref).all()
    assert (named[ok] >= (1.0 - 2.0 * TS.bound(1, W)) * clean.max(axis=0)[ok]).all()
    assert np.isnan(sums[1:]).any(axis=0)[ok].any()  # there ARE cells whose other hypotheses pass through the NaN


# ---- 4. against the plain integrator ----------------------------------------------------------------------------------------
def test_zero_walk_and_the_bank_of_zero_is_the_plain_integrator_bit_for_bit(b2, torch):
    for geom, K, W, H, w in ((SMALL, 3, 4, 1, (1.0, 0.25, 4.0)), (EVEN, 1, 16, 2, None), (SMALL, 1, 1, 1, None)):
        amb = handle(b2, geom)
        nD, nC = shape_of(amb)
        n_cpi = 24 // K
        maps = IC.maps(K, n_cpi, nD, nC, seed=51 + W)
        plain, tracks = b2.MapIntegrator(amb, K, W, H), b2.MapIntegrator(amb, K, W, H)
        try:
            tracks.set_tracks(None, None, 5)
            out, idx, met = stream(torch, amb, tracks, maps, [5] * (n_cpi // 5) + ([n_cpi % 5] if n_cpi % 5 else []), w)
            d_in = torch.from_numpy(np.ascontiguousarray(maps)).cuda()
            ref = torch.zeros((n_cpi, nD, nC), dtype=torch.complex64, device="cuda")
            rmet = torch.zeros((n_cpi, 2), dtype=torch.float64, device="cuda")
            n_out, _ = plain.process_dev(d_in.data_ptr(), n_cpi, ref.data_ptr(), rmet.data_ptr(), n_cpi, w,
                                         torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert n_out == out.shape[0] > 0 and not idx.any()
            assert np.array_equal(out.view(np.uint32), ref[:n_out].cpu().numpy().view(np.uint32))
            assert np.abs(met - rmet[:n_out].cpu().numpy()).max() <= DB_TOL
        finally:
            plain.close()
            tracks.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_counter_tables_and_buffers_as_they_were(b2, torch):
    amb = handle(b2, SMALL)
    nD, nC = shape_of(amb)
    L, lib = amb._L, b2._lib
    W = 3
    maps = IC.maps(2, 6, nD, nC, seed=61)
    walk, q = TS.tables(nD, nC)["jagged"], np.array(BANKS[5])
    d_in = torch.from_numpy(np.ascontiguousarray(maps)).cuda()
    wo, out = guarded(torch, (6, nD, nC), torch.complex64)
    wi, idx = guarded(torch, (6, nD, nC), torch.uint8)
    wm, met = guarded(torch, (6, 2), torch.float64)
    integ = b2.MapIntegrator(amb, 2, W, 1)
    n_out, fe = C.c_uint32(77), C.c_uint64(77)

    def tracks_dev(n=integ, d=None, n_cpi=4, w=None, o=None, i=None, m=None, cap=6):
        wp = None if w is None else np.asarray(w, dtype=np.float32).ctypes.data_as(C.c_void_p)
        return L.blah2hip_nci_process_tracks_dev(n._h if n else None, d_in.data_ptr() if d is None else d, n_cpi, wp,
                                                 out.data_ptr() if o is None else o, idx.data_ptr() if i is None else i,
                                                 met.data_ptr() if m is None else m, cap, C.byref(n_out), C.byref(fe), None)

    def set_tracks(wk, qs, n_rates, max_cpi):
        wp = None if wk is None else np.ascontiguousarray(wk, dtype=np.float64).ctypes.data_as(C.c_void_p)
        qp = None if qs is None else np.ascontiguousarray(qs, dtype=np.float64).ctypes.data_as(C.c_void_p)
        return L.blah2hip_nci_set_tracks(integ._h, wp, qp, n_rates, max_cpi)

    try:
        assert tracks_dev() == lib.ERR_INVALID  # no tracks set
        assert b"none set" in L.blah2hip_last_error()
        integ.set_tracks(walk, q, 4)
        o0, i0, m0, _ = call(torch, amb, integ, maps[:, :4])
        integ.reset()
        # set_tracks: what was set stays
        bad_walk, bad_q = walk.copy(), q.copy()
        bad_walk[7], bad_q[1] = np.inf, np.nan
        for args in ((bad_walk, q, 5, 4), (walk, bad_q, 5, 4), (walk, np.zeros(17), 17, 4), (walk, [nD / 2.0], 1, 4),
                     (walk, q, 5, 0), (walk, q, 5, 13), (np.full(nD, 1e7), q, 5, 4)):
            assert set_tracks(*args) == lib.ERR_INVALID, args[2:]
        assert L.blah2hip_nci_set_tracks(None, None, None, 0, 1) == lib.ERR_INVALID
        o_, i_, m_, _ = call(torch, amb, integ, maps[:, :4])  # (the counter was not reset by a refusal either)
        assert np.array_equal(o_.view(np.uint32), o0.view(np.uint32)) and np.array_equal(i_, i0)
        assert set_tracks(walk, [(nD - 1) / 2.0], 1, 4) == lib.OK  # |q| (W - 1) = nD - 1: allowed
        integ.set_tracks(walk, q, 4)
        # process: nothing enqueued, the counter unchanged
        integ_plain = b2.MapIntegrator(amb, 2, W, 1)
        before = integ.count(4)
        nan_w, neg_w = (1.0, np.nan), (1.0, -1.0)
        refused = [dict(n=None), dict(n_cpi=0), dict(n_cpi=5), dict(cap=1), dict(w=nan_w), dict(w=neg_w), dict(w=(0.0, 0.0)),
                   dict(o=0), dict(m=0), dict(d=d_in.data_ptr() + 4), dict(o=out.data_ptr() + 4),
                   dict(o=d_in.data_ptr()), dict(m=d_in.data_ptr()), dict(i=d_in.data_ptr()), dict(i=out.data_ptr() + 8),
                   dict(i=met.data_ptr()), dict(n=integ_plain)]
        for kw in refused:
            assert tracks_dev(**kw) == lib.ERR_INVALID, kw
            assert (n_out.value, fe.value) == (77, 77), kw
        with pytest.raises(b2.Blah2HipError):  # the history lives in the ring
            integ.process_dev(d_in.data_ptr(), 4, out.data_ptr(), met.data_ptr(), 6)
        integ_plain.close()
        torch.cuda.synchronize()
        assert integ.count(4) == before and untouched(wo) and untouched(wi) and untouched(wm)
        o1, i1, m1, _ = call(torch, amb, integ, maps[:, :4])
        assert np.array_equal(o1.view(np.uint32), o0.view(np.uint32)) and np.array_equal(i1, i0)
        assert np.array_equal(m1.view(np.uint64), m0.view(np.uint64))
    finally:
        integ.close()


def test_walk_table_and_timing_slots(b2, torch):
    amb = handle(b2, SMALL)
    nD, nC = shape_of(amb)
    L, lib = amb._L, b2._lib
    dims = types.SimpleNamespace(doppler=amb.doppler, n_corr=amb.dims.n_corr, n_doppler_bins=nD)
    for fc, sp in ((204.64e6, 1.0), (98.1e6, 0.5)):
        got = b2.nci_walk_table(amb, fc, sp)
        assert np.array_equal(got.view(np.uint64), b2.nci_walk_table(dims, fc, sp).view(np.uint64))
        assert got[0] > 0 > got[-1] and got[nD // 2] == 0  # rows ascend in Doppler; an approaching target moves earlier
    buf = np.zeros(nD)
    p = buf.ctypes.data_as(C.c_void_p)
    for args in ((None, 1e8, 1.0, p), (amb._h, 1e8, 1.0, None), (amb._h, 0.0, 1.0, p), (amb._h, np.nan, 1.0, p),
                 (amb._h, 1e8, 0.0, p), (amb._h, 1e8, np.inf, p), (amb._h, -1e8, 1.0, p)):
        assert L.blah2hip_nci_walk_table(*args) == lib.ERR_INVALID
    for bad in ((0.0, 1.0), (1e8, -1.0)):
        with pytest.raises(ValueError):
            b2.nci_walk_table(dims, *bad)
    maps = IC.maps(1, 5, nD, nC, seed=71)
    integ = b2.MapIntegrator(amb, 1, 2, 1)
    try:
        integ.set_tracks(b2.nci_walk_table(amb, 204.64e6), None, 5)
        integ.set_timing(True)
        integ.get_timing()
        call(torch, amb, integ, maps)
        t = integ.get_timing()
        assert t["track_power"][1] == 1 and t["track_sum"][1] == 1 and t["nci"][1] == 0
        assert t["track_power"][0] > 0 and t["track_sum"][0] > 0
    finally:
        integ.close()


# ---- 6. the scene -----------------------------------------------------------------------------------------------------------
def test_the_scene_on_the_device(b2, torch):
    maps, walk, q, (row, col), true_k = TS.scene()
    W = TS.SCENE["W"]
    amb = handle(b2, SMALL)
    aligned, plain = b2.MapIntegrator(amb, 1, W, 1), b2.MapIntegrator(amb, 1, W, 1)
    try:
        aligned.set_tracks(walk, q, W)
        out, idx, met, _ = call(torch, amb, aligned, maps)
        check_against_named(b2, out, idx, met, maps, walk, q, None, 1, W, 1, "scene")
        aligned.reset()
        host = aligned.process(maps)  # the host-array form goes along the tracks too
        assert len(host) == 1 and host[0]._cpi_index == W - 1 and np.array_equal(host[0].data.view(np.uint32), out[0].view(np.uint32))
        assert host[0].noisePower == met[0, 0] and host[0].maxPower == met[0, 1]
        sum_map = plain.process(maps)[0].data
    finally:
        aligned.close()
        plain.close()
    level = out[0].real
    assert np.unravel_index(np.argmax(level), level.shape) == (row, col) and int(idx[0, row, col]) == true_k
    assert np.unravel_index(np.argmax(sum_map.real), sum_map.shape) != (row, col)
    print(f"scene on the device: aligned {20 * np.log10(level[row, col] / np.median(level)):.2f} dB over the median, "
          f"plain {20 * np.log10(sum_map.real[row, col] / np.median(sum_map.real)):.2f} dB")
