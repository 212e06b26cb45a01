"""GPU: non-coherent integration of the maps over surveillance channels and consecutive CPIs (blah2hip_nci_process_dev,
nci_kernel), the detectors' thresholds for the looks of the sum (BLAH2HIP_OPT_CFAR_LOOKS) and the replay chain behind it.

No reference counterpart; the check is the fp64 NumPy restatement ``integrate_maps``.  The kernel reads any buffer with the
map layout, so most cases feed crafted maps (tests/integrate_crafted.py ``maps``): cell (k, c, i) of channel k and CPI c is
``level(k, c) u exp(i phi)`` with ``level = 1 + 0.25 ((3 k + 5 c) mod 7)``, ``u`` uniform in [0.7, 1.4] per (k, c, cell) and
a random phase -- every term of a sum is of the size of the sum, so a dropped or doubled channel or CPI moves every cell by
far more than the bound; a swapped one does so only where the two differ, which is what ``u`` is for (``level`` alone is the
same in every cell of a plane and has period 7 in c, and the kernel never sees the phase).  The handle is only there for its
dimensions.  The same kernel at every window and ring length, under every cut into calls, on maps 8 bytes off a 16-byte
boundary and with its metrics on a moving peak: tests/test_integrate_crafted_gpu.py, with the CPU proof of what those cases
reach and catch in tests/test_integrate_crafted_model.py.

Bounds
  * cells: ``|out - ref| <= (K W + 8) 2^-24 ref``, derived, not measured: all terms are non-negative, so a relative
    rounding never amplifies; a term passes at most K W + 3 roundings on its way into the sum whatever the order (two in
    |M|^2, up to K in p, up to W - 1 in the window, one with the scale), and the square root halves the total and adds
    one of its own.  The imaginary parts are exactly zero.
  * metrics: 1e-3 dB (the project's DB_TOL) against fp64 Map::set_metrics of the device's OWN output cells.
  * detectors: the hit set of a fp64 restatement of CfarDetector1D.cpp:23-100 (and of its 2-D extension) with
    ``cfar_alpha``'s table on the device's own output map, except cells whose |z|^2 / threshold lies within 1e-12 of 1 --
    of which the seeded map has none.
Geometries: 21 x 111 cells (an odd count: every other map, in or out, starts 8 bytes off a 16-byte boundary and goes through
8-byte accesses, and the last unit of a map is a single cell), 21 x 112 (every map aligned) and one case at the configs[1]
size 513 x 411 (hundreds of workgroups).
"""
import ctypes as C

import numpy as np
import pytest

import integrate_crafted as IC

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces
PAD = 64
MAX_BATCH = 24
SMALL = (-10, 100, -100, 100, 1_000_000, 100_000)    # 21 x 111
EVEN = (-10, 101, -100, 100, 1_000_000, 100_000)     # 21 x 112
CFG2 = (-10, 400, -256, 256, 2_000_000, 2_000_000)   # configs[1]: 513 x 411
DB_TOL = 1e-3
# (geometry, K, W, H, n_cpi, CPIs of history from an earlier call, weights)
CASES = [(SMALL, 1, 1, 1, 1, 0, None), (SMALL, 1, 3, 1, 5, 0, None), (SMALL, 3, 1, 1, 2, 0, None), (SMALL, 4, 4, 2, 6, 0, None),
         (SMALL, 8, 2, 1, 3, 0, None), (SMALL, 2, 16, 1, 12, 5, None), (SMALL, 2, 3, 5, 11, 0, None),
         (SMALL, 3, 2, 1, 3, 0, (1.0, 0.25, 4.0)), (SMALL, 3, 1, 1, 2, 0, (0.0, 1.0, 0.0)),
         (EVEN, 4, 4, 2, 6, 0, None), (EVEN, 2, 3, 1, 5, 2, None), (CFG2, 4, 4, 1, 6, 0, None)]
IDS = [f"{g[1] - g[0] + 1}cols-K{k}-W{w}-H{h}-cpi{c}" + (f"-hist{p}" if p else "") + ("-w" + "_".join(str(v) for v in wt) if wt else "")
       for g, k, w, h, c, p, wt in CASES]


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


def handle(b2, geom, tag=""):
    if (geom, tag) not in _handles:
        _handles[(geom, tag)] = b2.Ambiguity(*geom, True, max_batch=MAX_BATCH)
    return _handles[(geom, tag)]


def guarded(torch, shape, dtype):
    words = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size() // 4
    whole = torch.full((words + PAD,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    return whole, whole[:words].view(dtype).view(shape)


def guard_intact(whole):
    return bool((whole[-PAD:].cpu().numpy().view(np.uint32) == GUARD).all())


def untouched(whole):
    return bool((whole.cpu().numpy().view(np.uint32) == GUARD).all())


def crafted(K, n_cpi, nD, nC, seed):
    """integrate_crafted.maps: the levels under a factor drawn per (k, c, cell), so that no two cells are alike."""
    return IC.maps(K, n_cpi, nD, nC, seed)


def shape_of(amb):
    return amb.get_n_doppler_bins(), amb.get_n_delay_bins()


def call(torch, amb, integ, maps, w=None):
    """The next maps.shape[1] CPIs of ``integ`` into guarded outputs with room for one map per CPI ->
    (out complex64 [n_out, nD, nC], metrics [n_out, 2], first_end, the two guarded buffers)."""
    nD, nC = shape_of(amb)
    n_cpi = maps.shape[1]
    wo, out = guarded(torch, (n_cpi, nD, nC), torch.complex64)
    wm, met = guarded(torch, (n_cpi, 2), torch.float64)
    d_in = torch.from_numpy(np.ascontiguousarray(maps)).cuda()
    want_n, want_first = integ.count(n_cpi)
    n_out, first = integ.process_dev(d_in.data_ptr(), n_cpi, out.data_ptr(), met.data_ptr(), n_cpi, w,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (n_out, first) == (want_n, want_first)  # count() announces what the call reports
    assert guard_intact(wo) and guard_intact(wm)
    assert untouched(wo[n_out * nD * nC * 2:]) and untouched(wm[n_out * 4:])  # nothing behind the n_out maps
    return out[:n_out].cpu().numpy(), met[:n_out].cpu().numpy(), first, (wo, wm)


def cell_bound_check(out, ref, K, W, tag):
    """out complex64 [n_out, ...] against the fp64 levels ref under the derived bound; the worst ratio is printed."""
    assert out.shape == ref.shape, (tag, out.shape, ref.shape)
    assert (out.imag == 0).all(), tag
    bound = (K * W + 8) * 2.0 ** -24 * ref
    err = np.abs(out.real.astype(np.float64) - ref)
    print(f"{tag}: largest error / bound {float((err / bound).max()):.3f}")
    assert np.isfinite(out.real).all(), tag
    assert (err <= bound).all(), (tag, float((err / bound).max()))


def set_metrics64(z):
    """Map::set_metrics (Map.cpp:187-206) in fp64."""
    db = 10.0 * np.log10(np.abs(z.astype(np.complex128)))
    noise = db.mean()
    return noise, max(0.0, db.max()) - noise


_results = {}


def case_result(b2, torch, case):
    """Input maps (history included), the device's outputs and what the counts must be: computed once per case, shared by
    the tests, left unchanged."""
    if case not in _results:
        geom, K, W, H, n_cpi, hist, w = case
        amb = handle(b2, geom)
        nD, nC = shape_of(amb)
        maps = crafted(K, hist + n_cpi, nD, nC, seed=1000 + 100 * K + 10 * W + n_cpi)
        integ = b2.MapIntegrator(amb, K, W, H)
        try:
            if hist:
                out0, _, _, _ = call(torch, amb, integ, maps[:, :hist], w)
                assert hist < W and out0.shape[0] == 0  # the window is still filling
            out, met, first, _ = call(torch, amb, integ, maps[:, hist:], w)
        finally:
            integ.close()
        _results[case] = (maps, out, met, first)
    return _results[case]


# ---- 1. cells ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cells_within_the_fp32_bound(b2, torch, case):
    geom, K, W, H, n_cpi, hist, w = case
    maps, out, _, _ = case_result(b2, torch, case)
    if geom is SMALL:
        assert maps[0, 0].size % 2 == 1  # the odd cell count the alignment cases rest on
    ref = b2.integrate_maps(maps, w, W, H)
    ends = b2.integrate_ends(hist + n_cpi, W, H)
    ref = ref[[i for i, g in enumerate(ends) if g >= hist]]
    cell_bound_check(out, ref, K, W, f"integrate K={K} W={W} H={H} n_cpi={n_cpi} hist={hist} {out.shape[1]}x{out.shape[2]}")
    if w == (0.0, 1.0, 0.0):  # a selector: |M_1|, CPI by CPI
        mag = np.abs(maps[1].astype(np.complex128))
        assert (np.abs(out.real - mag) <= (K * W + 8) * 2.0 ** -24 * mag).all()


# ---- 2. counts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_counts_follow_the_formula(b2, torch, case):
    geom, K, W, H, n_cpi, hist, w = case
    _, out, met, first = case_result(b2, torch, case)
    ends = [g for g in range(hist, hist + n_cpi) if g >= W - 1 and (g - (W - 1)) % H == 0]
    assert out.shape[0] == met.shape[0] == len(ends) and len(ends) > 0
    assert first == ends[0]


def test_nothing_is_written_while_the_window_fills(b2, torch):
    amb = handle(b2, SMALL)
    nD, nC = shape_of(amb)
    maps = crafted(1, 4, nD, nC, seed=11)
    integ = b2.MapIntegrator(amb, 1, 3, 1)
    try:
        assert integ.looks == 3 and integ.count(2) == (0, 2) and integ.count(3) == (1, 2)
        out, met, first, (wo, wm) = call(torch, amb, integ, maps[:, :2])
        assert out.shape[0] == 0 and first == 2 and untouched(wo) and untouched(wm)
        # NULL outputs are accepted while nothing is due, and the CPI still counts: the window ends at the next one
        L = amb._L
        d_in = torch.from_numpy(np.ascontiguousarray(maps[:, 2:3])).cuda()
        assert integ.count(1) == (1, 2)
        integ.reset()
        assert integ.count(1) == (0, 2)
        n_out, fe = C.c_uint32(9), C.c_uint64(9)
        assert L.blah2hip_nci_process_dev(integ._h, d_in.data_ptr(), 1, None, None, None, 0, C.byref(n_out), C.byref(fe), None) == 0
        torch.cuda.synchronize()
        assert (n_out.value, fe.value) == (0, 2) and integ.count(2) == (1, 2)
    finally:
        integ.close()


# ---- 3. split invariance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [SMALL, EVEN], ids=["odd-cells", "even-cells"])
def test_the_bits_do_not_depend_on_how_the_cpis_are_cut_into_calls(b2, torch, geom):
    K, W, H, n_cpi = 2, 3, 2, 7
    amb = handle(b2, geom)
    nD, nC = shape_of(amb)
    maps = crafted(K, n_cpi, nD, nC, seed=23)
    integ = b2.MapIntegrator(amb, K, W, H)
    try:
        whole, wmet, first, _ = call(torch, amb, integ, maps)
        assert whole.shape[0] == 3 and first == 2  # windows end at 2, 4, 6
        integ.reset()
        parts, pmets, at = [], [], 0
        for cnt in (1, 2, 1, 3):
            o, m, _, _ = call(torch, amb, integ, maps[:, at:at + cnt])
            parts.append(o)
            pmets.append(m)
            at += cnt
        assert [p.shape[0] for p in parts] == [0, 1, 0, 2]
        assert np.array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32))
        assert np.array_equal(np.concatenate(pmets).view(np.uint64), wmet.view(np.uint64))
        integ.reset()
        again, amet, _, _ = call(torch, amb, integ, maps)
        assert np.array_equal(again.view(np.uint32), whole.view(np.uint32)) and np.array_equal(amet.view(np.uint64), wmet.view(np.uint64))
    finally:
        integ.close()


# ---- 4. cells that are not finite ---------------------------------------------------------------------------------------
def test_a_nan_or_inf_cell_touches_only_the_windows_that_hold_it(b2, torch):
    K, W, H, n_cpi = 2, 3, 1, 7
    amb = handle(b2, SMALL)
    nD, nC = shape_of(amb)
    maps = crafted(K, n_cpi, nD, nC, seed=29)
    clean = maps.copy()
    nan_at, inf_at = (5, 17), (nD - 1, nC - 1)  # the last cell of the map: the single-cell unit
    maps[1, 2][nan_at] = np.complex64(complex(np.nan, 1.0))
    maps[0, 2][inf_at] = np.complex64(complex(0.5, np.inf))
    integ = b2.MapIntegrator(amb, K, W, H)
    try:
        with np.errstate(all="ignore"):
            out, _, first, _ = call(torch, amb, integ, maps)
    finally:
        integ.close()
    assert first == 2 and out.shape[0] == 5  # windows end at 2 .. 6
    ref = b2.integrate_maps(clean, None, W, H)
    bad = np.zeros(out.shape, dtype=bool)
    for i, g in enumerate(range(2, 7)):
        if g - W + 1 <= 2 <= g:
            bad[i][nan_at] = bad[i][inf_at] = True
            assert np.isnan(out[i].real[nan_at]) and out[i].real[inf_at] == np.inf, g
    assert bad.sum() == 6 and (out.imag == 0).all()
    assert np.isfinite(out.real[~bad]).all()
    err = np.abs(out.real.astype(np.float64) - ref)[~bad]
    assert (err <= (K * W + 8) * 2.0 ** -24 * ref[~bad]).all()


# ---- 5. metrics ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_metrics_are_set_metrics_of_the_cells_as_written(b2, torch, case):
    _, out, met, _ = case_result(b2, torch, case)
    worst = 0.0
    for i in range(out.shape[0]):
        noise, peak = set_metrics64(out[i])
        worst = max(worst, abs(met[i, 0] - noise), abs(met[i, 1] - peak))
        assert abs(met[i, 0] - noise) <= DB_TOL, (i, met[i, 0], noise)
        assert abs(met[i, 1] - peak) <= DB_TOL, (i, met[i, 1], peak)
    print(f"integrated metrics {IDS[CASES.index(case)]}: largest difference {worst:.3e} dB")


@pytest.mark.parametrize("case", [CASES[3], CASES[5], CASES[11]], ids=[IDS[3], IDS[5], IDS[11]])
def test_two_calls_give_the_same_bits(b2, torch, case):
    geom, K, W, H, n_cpi, hist, w = case
    maps, out, met, _ = case_result(b2, torch, case)
    amb = handle(b2, geom)
    integ = b2.MapIntegrator(amb, K, W, H)
    try:
        if hist:
            call(torch, amb, integ, maps[:, :hist], w)
        out2, met2, _, _ = call(torch, amb, integ, maps[:, hist:], w)
    finally:
        integ.close()
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32))
    assert np.array_equal(met.view(np.uint64), met2.view(np.uint64))


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_integrator_as_it_was(b2, torch):
    from blah2_amd import _lib
    amb = handle(b2, SMALL)
    L, h = amb._L, amb._h
    nD, nC = shape_of(amb)
    cells = nD * nC
    K, W = 2, 3
    maps = crafted(K, 6, nD, nC, seed=41)
    # create
    n = C.c_void_p()
    for name, (k, w_, hop) in {"n_surv 0": (0, 3, 1), "n_surv 9": (9, 3, 1), "window 0": (2, 0, 1), "window 17": (2, 17, 1),
                               "hop 0": (2, 3, 0)}.items():
        assert L.blah2hip_nci_create(h, k, w_, hop, C.byref(n)) == _lib.ERR_INVALID, name
    assert L.blah2hip_nci_create(None, 2, 3, 1, C.byref(n)) == _lib.ERR_INVALID and not n.value

    seen, fresh = b2.MapIntegrator(amb, K, W, 1), b2.MapIntegrator(amb, K, W, 1)
    try:
        first2 = np.ascontiguousarray(maps[:, :2])
        for integ in (seen, fresh):
            assert call(torch, amb, integ, first2)[0].shape[0] == 0
        d_in = torch.from_numpy(np.ascontiguousarray(maps[:, 2:6])).cuda()  # 4 CPIs: windows end at 2, 3, 4, 5
        big = torch.zeros((K, 13, nD, nC), dtype=torch.complex64, device="cuda")
        wo, out = guarded(torch, (4, nD, nC), torch.complex64)
        wm, met = guarded(torch, (4, 2), torch.float64)
        int_map, int_met = C.c_void_p(), C.c_void_p()
        assert L.blah2hip_amb_result_ptrs(h, C.byref(int_map), C.byref(int_met)) == _lib.OK

        def wts(*v):
            a = np.array(v, dtype=np.float32)
            return a, C.c_void_p(a.ctypes.data)
        keep = [wts(1, -0.5), wts(1, np.nan), wts(np.inf, 1), wts(0, 0)]
        # (d_map, n_cpi, w, d_out_map, d_out_metrics, out_cap)
        good = [d_in.data_ptr(), 4, None, out.data_ptr(), met.data_ptr(), 4]
        bad = {
            "n_cpi 0": {1: 0}, "n_surv * n_cpi above max_batch": {0: big.data_ptr(), 1: 13, 5: 13}, "n_out above out_cap": {5: 3},
            "a negative weight": {2: keep[0][1]}, "a NaN weight": {2: keep[1][1]}, "an infinite weight": {2: keep[2][1]},
            "a zero weight sum": {2: keep[3][1]}, "NULL map": {3: None}, "NULL metrics": {4: None},
            "map inside the input": {3: d_in.data_ptr() + 8 * (K * 4 * cells - 1)},
            "map around the input's start": {0: out.data_ptr() + 8 * cells},
            "metrics inside the input": {4: d_in.data_ptr() + 16},
            "map in the handle's own map": {0: None, 3: int_map.value + 8 * cells},
        }
        n_out, fe = C.c_uint32(77), C.c_uint64(77)
        for name, change in bad.items():
            args = list(good)
            for k, v in change.items():
                args[k] = v
            assert L.blah2hip_nci_process_dev(seen._h, *args, C.byref(n_out), C.byref(fe), None) == _lib.ERR_INVALID, name
            assert seen.count(4) == (4, 2), name  # the counter has not moved
        assert L.blah2hip_nci_process_dev(None, *good, C.byref(n_out), C.byref(fe), None) == _lib.ERR_INVALID
        torch.cuda.synchronize()
        assert untouched(wo) and untouched(wm) and (n_out.value, fe.value) == (77, 77)
        # the call they were derived from is accepted, and gives the bits of the integrator that never saw them
        assert L.blah2hip_nci_process_dev(seen._h, *good, C.byref(n_out), C.byref(fe), None) == _lib.OK
        torch.cuda.synchronize()
        assert (n_out.value, fe.value) == (4, 2) and guard_intact(wo) and guard_intact(wm) and not untouched(wo)
        want, wmet, _, _ = call(torch, amb, fresh, maps[:, 2:6])
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(met.cpu().numpy().view(np.uint64), wmet.view(np.uint64))
    finally:
        seen.close()
        fresh.close()
    # the option
    assert L.blah2hip_amb_set_option(h, _lib.OPT_CFAR_LOOKS, 0) == _lib.ERR_INVALID
    assert L.blah2hip_amb_set_option(h, _lib.OPT_CFAR_LOOKS, _lib.MAX_CFAR_LOOKS + 1) == _lib.ERR_INVALID


# ---- 7. the detectors on the sum ------------------------------------------------------------------------------------------
def cfar_restated(z, alpha, ng_d, nt_d, ng_f, nt_f):
    """CfarDetector1D.cpp:23-100 (ng_f = nt_f = 0) and its 2-D extension in fp64 with the threshold factors ``alpha``:
    |z|^2 > alpha[n] (tot / n) over the in-bounds training cells, delay column 0 never training (:61), every cell tested.
    Returns (|z|^2 / threshold [nD, nC], n [nD, nC])."""
    z = z.astype(np.complex128)
    sq = z.real * z.real + z.imag * z.imag
    nD, nC = sq.shape
    hR, hC = ng_f + nt_f, ng_d + nt_d
    pad = np.zeros((nD + 2 * hR, nC + 2 * hC))
    one = np.zeros_like(pad)
    pad[hR:hR + nD, hC:hC + nC] = sq
    one[hR:hR + nD, hC:hC + nC] = 1.0
    pad[:, hC] = one[:, hC] = 0.0
    tot, n = np.zeros((nD, nC)), np.zeros((nD, nC))
    for di in range(-hR, hR + 1):
        for dj in range(-hC, hC + 1):
            if abs(di) <= ng_f and abs(dj) <= ng_d:
                continue
            tot += pad[hR + di:hR + di + nD, hC + dj:hC + dj + nC]
            n += one[hR + di:hR + di + nD, hC + dj:hC + dj + nC]
    n = n.astype(np.int64)
    with np.errstate(all="ignore"):
        return sq / (alpha[n] * (tot / n)), n


def device_hits(torch, amb, det, d_map, d_met, cells):
    d_hits = torch.zeros((1, cells, 2), dtype=torch.float64, device="cuda")
    d_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    det.process_dev(amb, 1, d_hits.data_ptr(), cells, d_cnt.data_ptr(), d_map.data_ptr(), d_met.data_ptr(),
                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    k = int(d_cnt[0])
    return d_hits[0, :k].cpu().numpy()


def hit_cells(b2, recs):
    h = recs.view(b2.HIT_DTYPE).reshape(-1)
    return set(zip(h["row"].tolist(), h["col"].tolist()))


def test_detectors_hold_their_pfa_on_the_sum_with_the_looks_option(b2, torch):
    from blah2_amd import _lib
    K, W, PFA = 4, 2, 1e-3
    amb = handle(b2, SMALL, "detector")  # a handle of its own: it has never seen the option
    L, h = amb._L, amb._h
    nD, nC = shape_of(amb)
    cells = nD * nC
    rng = np.random.default_rng(8)
    maps = ((rng.standard_normal((K, W, nD, nC)) + 1j * rng.standard_normal((K, W, nD, nC))) * np.sqrt(0.5)).astype(np.complex64)
    planted = (13, 60)
    maps[:, :, planted[0], planted[1]] = np.complex64(np.sqrt(10.0 ** 0.9))  # every look 9 dB above the mean p of 1
    d_in = torch.from_numpy(maps).cuda()
    d_map = torch.zeros((1, nD, nC), dtype=torch.complex64, device="cuda")
    d_met = torch.zeros((1, 2), dtype=torch.float64, device="cuda")
    integ = b2.MapIntegrator(amb, K, W, 1)
    try:
        assert integ.looks == 8
        assert integ.process_dev(d_in.data_ptr(), W, d_map.data_ptr(), d_met.data_ptr(), 1, None,
                                 torch.cuda.current_stream().cuda_stream) == (1, 1)
    finally:
        torch.cuda.synchronize()
        integ.close()
    z = d_map[0].cpu().numpy()

    # before the option was ever set: raw calls
    def raw_1d():
        d_hits = torch.zeros((1, cells, 2), dtype=torch.float64, device="cuda")
        d_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert L.blah2hip_cfar1d_dev(h, d_map.data_ptr(), d_met.data_ptr(), 1, PFA, 2, 6, -128, 0.0, d_hits.data_ptr(), cells,
                                     d_cnt.data_ptr(), None) == _lib.OK
        torch.cuda.synchronize()
        recs = d_hits[0, :int(d_cnt[0])].cpu().numpy().view(b2.HIT_DTYPE).reshape(-1)
        return recs[np.lexsort((recs["col"], recs["row"]))]
    before = raw_1d()

    for name, win, make in (("1-D", (2, 6, 0, 0), lambda looks: b2.CfarDetector1D(PFA, 2, 6, -128, 0.0, looks=looks)),
                            ("2-D", (2, 6, 1, 3), lambda looks: b2.CfarDetector2D(PFA, 2, 6, 1, 3, -128, 0.0, looks=looks))):
        got = {}
        for looks in (8, 1):
            max_n = (2 * (win[0] + win[1]) + 1) * (2 * (win[2] + win[3]) + 1)
            alpha = b2.cfar_alpha(PFA, looks, max_n)
            margin, n = cfar_restated(z, alpha, *win)
            assert n.max() <= max_n and n.min() >= 1
            assert not (np.abs(margin - 1.0) < 1e-12).any(), (name, looks)  # the seed leaves no cell on its threshold
            want = set(zip(*np.nonzero(margin > 1.0)))
            got[looks] = hit_cells(b2, device_hits(torch, amb, make(looks), d_map, d_met, cells))
            print(f"{name} detector, looks={looks}: {len(got[looks])} hits of {cells} cells")
            assert got[looks] == {(int(r), int(c)) for r, c in want}, (name, looks)
        assert planted in got[8], name
        assert got[1] <= got[8], name
    # the option back at 1: the list from before it was ever set, bit for bit
    amb.set_cfar_looks(8)
    with8 = raw_1d()
    assert planted in set(zip(with8["row"].tolist(), with8["col"].tolist()))
    amb.set_cfar_looks(1)
    after = raw_1d()
    assert np.array_equal(after.view(np.uint8), before.view(np.uint8))


# ---- 7b. the timing slot -------------------------------------------------------------------------------------------------
def test_the_integrators_timing_slot_counts_one_launch(b2, torch):
    from blah2_amd import _lib
    amb = handle(b2, SMALL)
    nD, nC = shape_of(amb)
    maps = crafted(2, 3, nD, nC, seed=61)
    integ = b2.MapIntegrator(amb, 2, 2, 1)
    integ.set_timing(True)
    amb.set_timing(True)
    try:
        integ.get_timing()
        amb.get_timing()  # clears whatever earlier calls left
        out, _, _, _ = call(torch, amb, integ, maps)
        t, ta = integ.get_timing(), amb.get_timing()
    finally:
        amb.set_timing(False)
        integ.close()
    assert out.shape[0] == 2
    assert set(t) == {"nci"} and t["nci"][1] == 1 and t["nci"][0] > 0.0
    # the ambiguity handle's slots are the ones it had: the metrics kernel behind the integrator counts there, nothing else
    assert _lib.K_COUNT == len(_lib.KERNEL_NAMES) and "nci" not in ta
    assert ta["metrics"][1] == 1 and all(n == 0 for name, (ms, n) in ta.items() if name != "metrics")


# ---- 8. the host-array helper ---------------------------------------------------------------------------------------------
def test_process_on_host_arrays_returns_maps_with_metrics(b2, torch):
    amb = handle(b2, SMALL)
    nD, nC = shape_of(amb)
    maps = crafted(2, 4, nD, nC, seed=91)
    integ = b2.MapIntegrator(amb, 2, 3)
    try:
        res = integ.process(maps[:, :1]) + integ.process(maps[:, 1:])
    finally:
        integ.close()
    assert [m._cpi_index for m in res] == [2, 3]
    ref = b2.integrate_maps(maps, None, 3)
    cell_bound_check(np.stack([m.data for m in res]), ref, 2, 3, "process(host arrays)")
    for m in res:
        noise, peak = set_metrics64(m.data)
        assert abs(m.noisePower - noise) <= DB_TOL and abs(m.maxPower - peak) <= DB_TOL
        assert np.array_equal(m.delay, amb.delay) and np.array_equal(m.doppler, amb.doppler)
    with pytest.raises(ValueError):
        b2.CfarDetector1D(1e-3, 2, 6, -128, 0.0, looks=6).process(res[0])  # a host map is one-look only


# ---- 9. through the replay chain ------------------------------------------------------------------------------------------
def capture_cpis(n, fs, n_cpi, seed):
    """int16 [n_cpi * n, 4] (I1 Q1 I2 Q2): a noise-like reference, the surveillance channel 0.8 of it plus an echo at
    37 bins and -60 Hz and noise of its own."""
    rng = np.random.default_rng(seed)
    N = n_cpi * n
    x = 300.0 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    xd = np.roll(x, 37)
    xd[:37] = 0
    y = 0.8 * x + 0.05 * xd * np.exp(-2j * np.pi * 60.0 * np.arange(N) / fs) + 30.0 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    iq = np.stack([x.real, x.imag, y.real, y.imag], axis=1)
    return np.clip(np.rint(iq), -32768, 32767).astype(np.int16)


def test_replay_chain_integrates_behind_the_ambiguity_stage(b2, torch, tmp_path):
    from blah2_amd import replay as R
    n, fs = SMALL[5], SMALL[4]
    W, B, N = 3, 2, 6
    path = str(tmp_path / "cap.rspduo")
    capture_cpis(n, fs, N, 3).tofile(path)
    cfg = {"fs": fs, "n_samples": n,
           "ambiguity": {"delayMin": SMALL[0], "delayMax": SMALL[1], "dopplerMin": SMALL[2], "dopplerMax": SMALL[3]},
           "detection": {"enable": True, "pfa": 1e-5, "nGuard": 2, "nTrain": 6, "minDelay": 5, "minDoppler": 15.0, "nCentroid": 6},
           "clutter": {"enable": False}}

    def run(c, **kw):
        chain = R.GpuChain(c, 0, batch=B, want_map=True, **kw)
        cap = R.RspduoFile(path, n)
        try:
            return R.replay(cap, chain, batch=B)
        finally:
            chain.close()
            cap.close()
    plain = run(cfg)
    assert [r["cpi"] for r in plain] == list(range(N)) and not any("window" in r or "integrating" in r for r in plain)
    # a chain whose config carries the key without a value is the chain without it
    same = run(dict(cfg, integrate=None))
    assert len(same) == N
    for a, b in zip(plain, same):
        assert a.keys() == b.keys() and np.array_equal(a["map"].view(np.uint32), b["map"].view(np.uint32))
        assert all(a[k] == b[k] for k in a if k != "map")

    res = run(dict(cfg, integrate={"window": W, "hop": 1}))
    assert [r["cpi"] for r in res] == list(range(N))
    assert all(r == {"integrating": True, "cpi": g} for g, r in enumerate(res[:W - 1]))
    # ... against MapIntegrator on the chain's own per-CPI maps
    amb = handle(b2, SMALL)
    integ = b2.MapIntegrator(amb, 1, W, 1)
    try:
        want = integ.process(np.stack([r["map"] for r in plain])[None])
    finally:
        integ.close()
    assert [m._cpi_index for m in want] == [2, 3, 4, 5]
    step = float(amb.doppler[1] - amb.doppler[0])
    det = b2.CfarDetector1D(1e-5, 2, 6, 5, 15.0, looks=W)
    fin = b2.DetectionFinisher(6, 6, 1 / (n / fs), True, True)
    cells = amb.get_n_doppler_bins() * amb.get_n_delay_bins()
    st = torch.cuda.current_stream().cuda_stream
    for m, r in zip(want, res[W - 1:]):
        assert r["cpi"] == m._cpi_index and r["window"] == W
        assert np.array_equal(r["map"].view(np.uint32), m.data.view(np.uint32))
        assert r["noisePower"] == m.noisePower and r["maxPower"] == m.maxPower
        # the detections: the detector made for W looks and the finisher on that map
        d_map = torch.from_numpy(m.data[None].copy()).cuda()
        d_met = torch.tensor([[m.noisePower, m.maxPower]], dtype=torch.float64, device="cuda")
        d_hits = torch.zeros((1, cells, 2), dtype=torch.float64, device="cuda")
        d_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        d_out = torch.zeros((1, cells, 4), dtype=torch.float64, device="cuda")
        d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
        det.process_dev(amb, 1, d_hits.data_ptr(), cells, d_cnt.data_ptr(), d_map.data_ptr(), d_met.data_ptr(), st)
        fin.process_dev(amb, 1, d_hits.data_ptr(), cells, d_cnt.data_ptr(), d_out.data_ptr(), cells, d_n.data_ptr(),
                        d_map.data_ptr(), d_met.data_ptr(), st)
        torch.cuda.synchronize()
        host = b2.dets_to_detection(d_out[0].cpu().numpy().view(b2.DET_DTYPE).reshape(-1), int(d_n[0]), cells)
        assert r["delay"] == host.delay.tolist() and r["doppler"] == host.doppler.tolist() and r["snr"] == host.snr.tolist()
        hit = (np.abs(np.array(r["delay"]) - 37) < 1.0) & (np.abs(np.array(r["doppler"]) + 60.0) < step)
        assert hit.any(), ("the echo is missing", r["cpi"])
    amb.set_cfar_looks(1)  # (the module's shared handle as the other tests found it)

    # several ranks deal the batches round-robin: windows must stay inside a batch
    chain = R.GpuChain(dict(cfg, integrate={"window": W, "hop": 1}), 0, batch=B)
    try:
        with pytest.raises(ValueError, match="hop == window"):
            chain.shard_check(2)
        chain.shard_check(1)
    finally:
        chain.close()
    chain = R.GpuChain(dict(cfg, integrate={"window": 2, "hop": 2}), 0, batch=B, want_map=True)
    cap = R.RspduoFile(path, n)
    try:
        chain.shard_check(2)
        per_batch = list(chain.run_batches(cap, [(2, 2), (0, 2)]))  # any order: every batch starts at count 0
    finally:
        chain.close()
        cap.close()
    assert [[("integrating" in r, r["cpi"]) for r in b] for b in per_batch] == [[(True, 2), (False, 3)], [(True, 0), (False, 1)]]
    integ = b2.MapIntegrator(amb, 1, 2, 2)
    try:
        for b, k0 in zip(per_batch, (2, 0)):
            integ.reset()
            m = integ.process(np.stack([plain[k0]["map"], plain[k0 + 1]["map"]])[None])[0]
            assert np.array_equal(b[1]["map"].view(np.uint32), m.data.view(np.uint32))
    finally:
        integ.close()
