"""GPU: the clutter-map detector and its gate (blah2hip_cmap_process_dev / _gate_dev: cmap_kernel, hits_gate_kernel).

No reference counterpart; the check is the fp64 restatement ``clutter_map`` of process.py, fed the device's own levels
(``d_out_level``).  The kernel reads any buffer with the map layout, so the maps are crafted (tests/clutter_map_scenes.py) and
the handle is only there for its dimensions and axes.

Bounds
  * b: ``|b - b_fp64| <= (k + 4) 2^-24 U``, ``k = min(age, T)``, ``U`` the largest u the cell has absorbed -- derived in
    include/blah2hip.h, not measured; every cell is checked.
  * exceed plane: cell for cell, except cells whose u lies within ``2 (k + 4) 2^-24 alpha U`` of ``alpha b`` in the
    restatement, which may go either way; at most 1e-4 of the tested cells may do so (tests/test_clutter_map_model.py
    shows that the inputs hold none, or one in 632 529 at 513 x 411).
  * levels: one fp32 rounding of the fp64 value: 2^-23 relative.
  * snr: ``5 log10 p - noisePower`` with p the kernel's fp32 value, which an fp64 p meets within two fp32 roundings:
    5 log10(1 + 2^-22) = 5.2e-7 dB.
Equal bits are asked wherever the same cells go through the same arithmetic: cuts into calls, a map 8 bytes off, a reset.
"""
import numpy as np
import pytest

import clutter_map_scenes as S

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)
PAD = 64
MAX_BATCH = 40


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


def handle(b2, nD, nC):
    if (nD, nC) not in _handles:
        g = S.geom(nD, nC)
        _handles[(nD, nC)] = b2.Ambiguity(g[0], g[1], g[2], g[3], g[4], g[5], False, max_batch=4 if nD > 100 else MAX_BATCH,
                                          n_doppler_bins=g[6])
        assert (_handles[(nD, nC)].get_n_doppler_bins(), _handles[(nD, nC)].get_n_delay_bins()) == (nD, nC)
    return _handles[(nD, nC)]


def guarded(torch, shape, dtype):
    """A device array with PAD words of a NaN payload behind it (whole, view)."""
    nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    words = (nbytes + 3) // 4
    whole = torch.full((words + PAD,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    return whole, whole.view(torch.uint8)[:nbytes].view(dtype).view(shape)


def guard_intact(whole):
    return bool((whole[-PAD:].cpu().numpy().view(np.uint32) == GUARD).all())


def run(b2, torch, det, maps, mets=None, lists=True, planes=True, cap=None, offset=False):
    """One call on the next maps.shape[0] CPIs -> dict(exceed, level, hits (a list of record arrays per CPI), count)."""
    n_cpi, nD, nC = maps.shape
    cells = nD * nC
    cap = cells if cap is None else cap
    mets = S.metrics(maps) if mets is None else mets
    flat = torch.from_numpy(np.ascontiguousarray(maps).reshape(-1))
    if offset:  # the first map 8 bytes off a 16-byte boundary
        buf = torch.zeros(flat.numel() + 1, dtype=torch.complex64, device="cuda")
        buf[1:] = flat.cuda()
        d_map = buf[1:]
        assert d_map.data_ptr() % 16 == 8
    else:
        d_map = flat.cuda()
        assert d_map.data_ptr() % 16 == 0
    d_met = torch.from_numpy(np.ascontiguousarray(mets)).cuda()
    we, d_ex = guarded(torch, (n_cpi, nD, nC), torch.uint8)
    wl, d_lev = guarded(torch, (n_cpi,), torch.float32)
    wh, d_hits = guarded(torch, (n_cpi, cap, 2), torch.float64)
    wc, d_cnt = guarded(torch, (n_cpi,), torch.int32)
    det.process_dev(n_cpi, d_hits.data_ptr() if lists else None, cap if lists else 0, d_cnt.data_ptr() if lists else None,
                    d_map.data_ptr(), d_met.data_ptr(), d_ex.data_ptr() if planes else None, d_lev.data_ptr() if planes else None,
                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert guard_intact(we) and guard_intact(wl) and guard_intact(wh) and guard_intact(wc)
    out = {}
    if planes:
        out["exceed"] = d_ex.cpu().numpy()
        out["level"] = d_lev.cpu().numpy()
    if lists:
        cnt = d_cnt.cpu().numpy().astype(np.int64)
        recs = d_hits.cpu().numpy().view(b2.HIT_DTYPE).reshape(n_cpi, cap)
        out["count"] = cnt
        out["hits"] = [recs[c, :min(cnt[c], cap)].copy() for c in range(n_cpi)]
    return out


def hit_cells(recs):
    return sorted(zip(recs["row"].tolist(), recs["col"].tolist()))


def detector(b2, amb, T, pfa=1e-2, normalise=True, min_delay=-128, min_doppler=0.0):
    return b2.ClutterMapDetector(amb, pfa, T, min_delay, min_doppler, normalise)


@pytest.mark.parametrize("case", S.CASES, ids=[c.tag for c in S.CASES])
def test_against_the_restatement(b2, torch, case):
    amb = handle(b2, case.nD, case.nC)
    maps = S.case_maps(case)
    mets = S.metrics(maps)
    det = detector(b2, amb, case.T, case.pfa, case.normalise)
    try:
        got = run(b2, torch, det, maps, mets)
        b = det.background().astype(np.float64)
        assert det.age() == case.n_cpi
    finally:
        det.close()
    lev64 = S.levels(maps) if case.normalise else np.ones(case.n_cpi)
    assert (np.abs(got["level"] - lev64) <= 2.0 ** -23 * lev64).all()
    alpha = b2.clutter_map_alpha_table(case.pfa, case.T, 16 * case.T)
    state = {}
    exceed, b64, detail = b2.clutter_map(maps, got["level"].astype(np.float64) if case.normalise else None, alpha, case.T, state,
                                         detail=True)
    err, bound = np.abs(b - b64), S.b_bound(case.n_cpi, case.T, state["umax"])
    print(f"{case.tag}: b reaches {float((err / bound).max()):.2f} of the bound")
    assert (err <= bound).all()  # every cell
    margin = S.margin_cells(detail, alpha, case.T)
    differ = got["exceed"] != exceed
    print(f"{case.tag}: {int(exceed.sum())} cells exceed, {int(margin.sum())} inside the margin, {int(differ.sum())} differ")
    assert set(np.unique(got["exceed"])) <= {0, 1} and not got["exceed"][0].any()
    assert margin.sum() <= 1e-4 * exceed[1:].size
    assert not (differ & ~margin).any()
    assert exceed.sum() > 0.002 * exceed.size  # the comparison is about something
    # the list: the plane's cells (no skips here), with their snr
    for c in range(case.n_cpi):
        want = sorted(zip(*[v.tolist() for v in np.nonzero(got["exceed"][c])]))
        assert got["count"][c] == len(want) and hit_cells(got["hits"][c]) == want, c
        h = got["hits"][c]
        if len(h):
            p = np.abs(maps[c][h["row"], h["col"]].astype(np.complex128)) ** 2
            assert np.abs(h["snr"] - (5.0 * np.log10(p) - mets[c, 0])).max() <= 5.2e-7, c


def test_cuts_into_calls_change_no_bit(b2, torch):
    """21 x 111, T = 3, 7 CPIs: cuts 1, 2, 1, 3 and 3, 4 against one call; and T = 2 over 40 CPIs cut 3, 30, 7: the second
    call crosses the table's last entry (age 32) in mid-walk, the first one the memory."""
    for case, cut_sets in ((S.Case("cuts", 21, 111, 7, 3, 1e-2, True, 21), ((1, 2, 1, 3), (3, 4))), (S.CASES[4], ((3, 30, 7),))):
        amb = handle(b2, case.nD, case.nC)
        maps = S.case_maps(case)
        mets = S.metrics(maps)
        det = detector(b2, amb, case.T)
        try:
            whole = run(b2, torch, det, maps, mets)
            b_whole = det.background()
            for cuts in cut_sets:
                det.reset()
                at, parts = 0, []
                for n in cuts:
                    parts.append(run(b2, torch, det, maps[at:at + n], mets[at:at + n]))
                    at += n
                    assert det.age() == at
                assert at == case.n_cpi
                assert np.array_equal(det.background().view(np.uint32), b_whole.view(np.uint32)), cuts
                assert np.array_equal(np.concatenate([p["exceed"] for p in parts]), whole["exceed"]), cuts
                assert np.array_equal(np.concatenate([p["level"] for p in parts]).view(np.uint32), whole["level"].view(np.uint32))
                hits = [h for p in parts for h in p["hits"]]
                for c in range(case.n_cpi):
                    a, b = np.sort(hits[c], order=["row", "col"]), np.sort(whole["hits"][c], order=["row", "col"])
                    assert a.tobytes() == b.tobytes(), (cuts, c)
        finally:
            det.close()


def test_table_cache_keeps_eight(b2, torch):
    """21 x 111, T = 3, one detector: thirteen pfa values and then the first again, one CPI per call, so the ninth to the
    thirteenth table evict the first five and the last call builds the first one anew.  Every call's plane and list against
    the restatement carried over the same sequence with the same tables, under the bounds of test_against_the_restatement.
    The comparison is about something: N times the pfa values of the calls from age 1 on is 532 expected hits, at least half
    are asked; and a stale table would show: with the table of the call before, N (pfa[0] - pfa[12]) = 233 decisions are
    expected to change over the twelve falling steps and as many at the last call, at least 100 are asked."""
    case = S.Case("cache", 21, 111, 14, 3, None, True, 41)
    amb = handle(b2, case.nD, case.nC)
    maps = S.case_maps(case)
    mets = S.metrics(maps)
    pfas = [10.0 ** -(1.0 + 0.25 * k) for k in range(13)]
    det = detector(b2, amb, case.T, pfas[0])
    state, in_margin, tested, hits, stale, before = {}, 0, 0, 0, 0, None
    try:
        for c, pfa in enumerate(pfas + pfas[:1]):
            det.pfa = pfa
            got = run(b2, torch, det, maps[c:c + 1], mets[c:c + 1])
            assert det.age() == c + 1
            alpha = b2.clutter_map_alpha_table(pfa, case.T, 16 * case.T)
            umax0 = state.get("umax")
            exceed, _, detail = b2.clutter_map(maps[c:c + 1], got["level"].astype(np.float64), alpha, case.T, state, detail=True)
            margin = S.margin_cells(detail, alpha, case.T, age0=c, umax0=umax0)
            assert not ((got["exceed"] != exceed) & ~margin).any(), (c, pfa)
            want = sorted(zip(*[v.tolist() for v in np.nonzero(got["exceed"][0])]))
            assert got["count"][0] == len(want) and hit_cells(got["hits"][0]) == want, (c, pfa)
            if c >= 1:
                in_margin += int(margin.sum())
                tested += exceed.size
                hits += int(exceed.sum())
                idx = min(c, 16 * case.T)
                stale += int(np.count_nonzero((detail["u"] > before[idx] * (detail["thr"] / alpha[idx])) != (exceed != 0)))
            before = alpha
    finally:
        det.close()
    print(f"cache: {hits} hits, {in_margin} of {tested} decisions inside the margin; {stale} would change under the table of the call before")
    assert in_margin <= 1e-4 * tested
    assert hits >= 266 and stale >= 100


def test_map_pointer_8_bytes_off_and_reset(b2, torch):
    case = S.CASES[0]
    amb = handle(b2, case.nD, case.nC)
    maps = S.case_maps(case)
    det = detector(b2, amb, case.T)
    try:
        ref = run(b2, torch, det, maps)
        b_ref = det.background()
        det.reset()
        assert det.age() == 0
        off = run(b2, torch, det, maps, offset=True)  # (the plane's old content is not read: the reset cleared nothing)
        assert np.array_equal(off["exceed"], ref["exceed"]) and np.array_equal(det.background().view(np.uint32), b_ref.view(np.uint32))
        assert [hit_cells(h) for h in off["hits"]] == [hit_cells(h) for h in ref["hits"]]
        # without the reset the same maps meet an older average: other decisions
        again = run(b2, torch, det, maps)
        assert det.age() == 2 * case.n_cpi and again["exceed"][0].any() and not np.array_equal(again["exceed"], ref["exceed"])
    finally:
        det.close()


def test_lists_planes_and_capacity(b2, torch):
    case = S.CASES[0]
    amb = handle(b2, case.nD, case.nC)
    maps = S.case_maps(case)
    det = detector(b2, amb, case.T)
    try:
        both = run(b2, torch, det, maps)
        b_ref = det.background()
        det.reset()
        only_list = run(b2, torch, det, maps, planes=False)
        assert [hit_cells(h) for h in only_list["hits"]] == [hit_cells(h) for h in both["hits"]]
        det.reset()
        only_plane = run(b2, torch, det, maps, lists=False)
        assert np.array_equal(only_plane["exceed"], both["exceed"])
        assert np.array_equal(det.background().view(np.uint32), b_ref.view(np.uint32))
        det.reset()
        cap = 7
        assert both["count"].max() > cap
        small = run(b2, torch, det, maps, cap=cap)
        assert np.array_equal(small["count"], both["count"])  # the count exceeds cap; cap records were stored
        for c in range(case.n_cpi):
            assert len(small["hits"][c]) == min(cap, both["count"][c])
            assert set(hit_cells(small["hits"][c])) <= set(hit_cells(both["hits"][c]))
    finally:
        det.close()


def test_skips_touch_the_list_not_the_plane(b2, torch):
    case = S.CASES[0]
    amb = handle(b2, case.nD, case.nC)
    maps = S.case_maps(case)
    min_delay, min_doppler = 20, float(np.sort(np.abs(amb.doppler))[5]) + 1e-9
    rows_ok = np.abs(amb.doppler) >= min_doppler
    cols_ok = amb.delay >= min_delay
    assert 0 < rows_ok.sum() < case.nD and 0 < cols_ok.sum() < case.nC
    plain = detector(b2, amb, case.T)
    skip = detector(b2, amb, case.T, min_delay=min_delay, min_doppler=min_doppler)
    try:
        ref = run(b2, torch, plain, maps)
        got = run(b2, torch, skip, maps)
        assert np.array_equal(got["exceed"], ref["exceed"])
        for c in range(case.n_cpi):
            want = [rc for rc in hit_cells(ref["hits"][c]) if rows_ok[rc[0]] and cols_ok[rc[1]]]
            assert hit_cells(got["hits"][c]) == want and got["count"][c] == len(want), c
        assert sum(len(h) for h in got["hits"]) < sum(len(h) for h in ref["hits"])
    finally:
        plain.close()
        skip.close()


@pytest.mark.parametrize("normalise", [True, False], ids=["normalised", "raw"])
def test_special_cells(b2, torch, normalise):
    """A NaN cell and an Inf cell (CPIs 0, 3 and 5), and an all-zero map (CPI 6; its noisePower is -inf, so its level is
    +inf and every u of it NaN when normalised): no hit, b untouched, the other cells as without them."""
    case = S.Case("special", 21, 111, 9, 3, 1e-2, normalise, 31)
    amb = handle(b2, case.nD, case.nC)
    clean = S.case_maps(case)
    clean[6] = 0
    mets = S.metrics(clean)  # the metrics of the clean maps: the special cells must not move the level
    maps = clean.copy()
    nan, inf = np.float32("nan"), np.float32("inf")
    spots = {(0, 2, 5): complex(nan, 1), (3, 2, 5): complex(1, nan), (5, 7, 110): complex(inf, 0), (3, 20, 0): complex(0, -inf),
             (0, 11, 3): complex(inf, inf)}
    for (c, r, k), v in spots.items():
        maps[c, r, k] = v
    touched = np.zeros(maps.shape[1:], dtype=bool)
    for (_, r, k) in spots:
        touched[r, k] = True
    det = detector(b2, amb, case.T, normalise=normalise)
    try:
        ref = run(b2, torch, det, clean, mets)
        b_ref = det.background()
        det.reset()
        got = run(b2, torch, det, maps, mets)
        b = det.background()
    finally:
        det.close()
    assert np.array_equal(got["exceed"][:, ~touched], ref["exceed"][:, ~touched])
    assert np.array_equal(b[~touched].view(np.uint32), b_ref[~touched].view(np.uint32))
    assert np.isfinite(b).all()
    for (c, r, k) in spots:
        assert got["exceed"][c, r, k] == 0 and (r, k) not in hit_cells(got["hits"][c])
    assert not got["exceed"][6].any() and got["count"][6] == 0
    alpha = b2.clutter_map_alpha_table(case.pfa, case.T, 16 * case.T)
    state = {}
    exceed, b64, detail = b2.clutter_map(maps, got["level"].astype(np.float64) if normalise else None, alpha, case.T, state, detail=True)
    margin = S.margin_cells(detail, alpha, case.T)
    assert margin.sum() == 0 and np.array_equal(got["exceed"], exceed)
    assert (np.abs(b - b64) <= S.b_bound(case.n_cpi, case.T, state["umax"])).all()
    if normalise:
        assert np.isinf(got["level"][6])


def test_gate(b2, torch):
    """Stable order, a count beyond cap, records outside the map, against gate_hits."""
    nD, nC = 21, 111
    amb = handle(b2, nD, nC)
    rng = np.random.default_rng(5)
    n_cpi, cap = 3, 700  # three chunks of 256, the last one partial
    counts = np.array([cap + 50, 300, 0], dtype=np.int32)
    hits = np.zeros((n_cpi, cap), dtype=b2.HIT_DTYPE)
    hits["row"] = rng.integers(-2, nD + 2, (n_cpi, cap))
    hits["col"] = rng.integers(-3, nC + 3, (n_cpi, cap))
    hits["snr"] = rng.uniform(0, 40, (n_cpi, cap))
    exceed = (rng.uniform(size=(n_cpi, nD, nC)) < 0.4).astype(np.uint8) * rng.integers(1, 255, (n_cpi, nD, nC)).astype(np.uint8)
    det = detector(b2, amb, 8)
    try:
        d_ex = torch.from_numpy(exceed).cuda()
        d_hits = torch.from_numpy(hits.view(np.float64).reshape(n_cpi, cap, 2)).cuda()
        d_cnt = torch.from_numpy(counts).cuda()
        wo, d_out = guarded(torch, (n_cpi, cap, 2), torch.float64)
        wc, d_ocnt = guarded(torch, (n_cpi,), torch.int32)
        det.gate_dev(d_ex.data_ptr(), n_cpi, d_hits.data_ptr(), cap, d_cnt.data_ptr(), d_out.data_ptr(), d_ocnt.data_ptr(),
                     torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert guard_intact(wo) and guard_intact(wc)
        out = d_out.cpu().numpy().view(b2.HIT_DTYPE).reshape(n_cpi, cap)
        ocnt = d_ocnt.cpu().numpy()
        for c in range(n_cpi):
            want = b2.gate_hits(hits[c], counts[c], exceed[c])
            assert ocnt[c] == len(want), c
            assert out[c, :len(want)].tobytes() == want.tobytes(), c  # the same records in the same order
        assert 100 < ocnt[0] < cap and ocnt[2] == 0
        assert det.age() == 0
    finally:
        det.close()


def test_refusals_leave_age_and_plane(b2, torch):
    nD, nC = 21, 111
    amb = handle(b2, nD, nC)
    case = S.CASES[0]
    maps = S.case_maps(case)[:3]
    L = b2.load()
    import ctypes as C
    h = C.c_void_p()
    for memory, flags in ((0, 0), (65, 0), (8, 2), (8, 0x80000001)):
        assert L.blah2hip_cmap_create(amb._h, memory, flags, C.byref(h)) == -1
    assert L.blah2hip_cmap_create(amb._h, 8, 1, None) == -1
    for f in (L.blah2hip_cmap_reset, L.blah2hip_cmap_destroy):
        assert f(None) in (-1, 0)  # (destroy of NULL is a no-op)
    assert L.blah2hip_cmap_prepare(None, 1e-3) == -1 and L.blah2hip_cmap_read_background(None, None) == -1
    det = detector(b2, amb, 8)
    try:
        run(b2, torch, det, maps)
        b0 = det.background()
        st = torch.cuda.current_stream().cuda_stream
        d_map = torch.from_numpy(maps).cuda()
        d_met = torch.from_numpy(S.metrics(maps)).cuda()
        d_hits = torch.zeros((3, 16, 2), dtype=torch.float64, device="cuda")
        d_cnt = torch.full((3,), 77, dtype=torch.int32, device="cuda")
        d_out = torch.zeros((3, 16, 2), dtype=torch.float64, device="cuda")
        d_ocnt = torch.zeros(3, dtype=torch.int32, device="cuda")
        d_ex = torch.zeros((3, nD, nC), dtype=torch.uint8, device="cuda")
        P = lambda t: t.data_ptr()  # noqa: E731
        good = dict(n_cpi=3, d_hits=P(d_hits), cap=16, d_count=P(d_cnt), d_map=P(d_map), d_metrics=P(d_met))
        bad = [dict(good, n_cpi=0), dict(good, n_cpi=MAX_BATCH + 1), dict(good, d_hits=None), dict(good, d_count=None),
               dict(good, cap=0), dict(good, d_map=P(d_map) + 4)]
        for kw in bad:
            with pytest.raises(b2.Blah2HipError) as e:
                det.process_dev(stream=st, **kw)
            assert e.value.code == -1, kw
        for pfa in (0.0, 1.0, float("nan")):
            det.pfa, keep = pfa, det.pfa
            with pytest.raises(b2.Blah2HipError) as e:
                det.process_dev(stream=st, **good)
            assert e.value.code == -1
            with pytest.raises(b2.Blah2HipError):
                det.prepare()
            det.pfa = keep
        assert L.blah2hip_cmap_process_dev(None, P(d_map), P(d_met), 3, 1e-2, 0, 0.0, None, 0, None, None, None, None) == -1
        amb.set_cfar_looks(4)  # integrated maps are not built
        try:
            with pytest.raises(b2.Blah2HipError) as e:
                det.process_dev(stream=st, **good)
            assert e.value.code == -3
        finally:
            amb.set_cfar_looks(1)
        gate_good = (P(d_ex), 3, P(d_hits), 16, P(d_cnt), P(d_out), P(d_ocnt))
        for i, v in ((0, None), (2, None), (4, None), (5, None), (6, None), (1, 0), (1, MAX_BATCH + 1), (3, 0),
                     (5, P(d_hits)), (5, P(d_hits) + 16), (6, P(d_cnt))):
            args = list(gate_good)
            args[i] = v
            with pytest.raises(b2.Blah2HipError) as e:
                det.gate_dev(*args, stream=st)
            assert e.value.code == -1, (i, v)
        torch.cuda.synchronize()
        assert det.age() == 3 and np.array_equal(det.background().view(np.uint32), b0.view(np.uint32))
        assert (d_cnt.cpu().numpy() == 77).all()  # nothing was enqueued: not even the zeroing of the counts
    finally:
        det.close()


def test_scene_behind_a_ca_cfar(b2, torch):
    """The scene of tests/clutter_map_scenes.py on the device: a CA-CFAR list in front, the gated list behind -- the CA hits
    in the cells the model's plane marks (test_clutter_map_model.py: no cell of the scene is inside the margin): the fixed
    discrete is in the detector's list and never in the gated one, the moving target stays."""
    T, pfa = 8, 1e-3
    maps, discrete, target = S.scene(3)
    n_cpi, nD, nC = maps.shape
    cells = nD * nC
    amb = handle(b2, nD, nC)
    mets = S.metrics(maps)
    ca = b2.CfarDetector1D(pfa, 2, 6, -128, 0.0)
    det = detector(b2, amb, T, pfa)
    try:
        st = torch.cuda.current_stream().cuda_stream
        d_map = torch.from_numpy(maps).cuda()
        d_met = torch.from_numpy(mets).cuda()
        d_hits = torch.zeros((n_cpi, cells, 2), dtype=torch.float64, device="cuda")
        d_cnt = torch.zeros(n_cpi, dtype=torch.int32, device="cuda")
        d_out = torch.zeros((n_cpi, cells, 2), dtype=torch.float64, device="cuda")
        d_ocnt = torch.zeros(n_cpi, dtype=torch.int32, device="cuda")
        d_ex = torch.zeros((n_cpi, nD, nC), dtype=torch.uint8, device="cuda")
        d_lev = torch.zeros(n_cpi, dtype=torch.float32, device="cuda")
        ca.process_dev(amb, n_cpi, d_hits.data_ptr(), cells, d_cnt.data_ptr(), d_map.data_ptr(), d_met.data_ptr(), st)
        det.process_dev(n_cpi, None, 0, None, d_map.data_ptr(), d_met.data_ptr(), d_ex.data_ptr(), d_lev.data_ptr(), st)
        det.gate_dev(d_ex.data_ptr(), n_cpi, d_hits.data_ptr(), cells, d_cnt.data_ptr(), d_out.data_ptr(), d_ocnt.data_ptr(), st)
        torch.cuda.synchronize()
        cnt, ocnt = d_cnt.cpu().numpy(), d_ocnt.cpu().numpy()
        hits = d_hits.cpu().numpy().view(b2.HIT_DTYPE).reshape(n_cpi, cells)
        out = d_out.cpu().numpy().view(b2.HIT_DTYPE).reshape(n_cpi, cells)
        lev = d_lev.cpu().numpy().astype(np.float64)
    finally:
        det.close()
    exceed, _ = b2.clutter_map(maps, lev, b2.clutter_map_alpha_table(pfa, T, 16 * T), T)
    in_ca = in_gated = tgt_ca = tgt_gated = 0
    for c in range(n_cpi):
        front = hits[c, :cnt[c]]
        want = front[exceed[c][front["row"], front["col"]] != 0]
        assert out[c, :ocnt[c]].tobytes() == want.tobytes(), c  # the same cells as the model, in the detector's order
        in_ca += discrete in hit_cells(front)
        in_gated += discrete in hit_cells(out[c, :ocnt[c]])
        if c >= 4:
            tgt_ca += target[c] in hit_cells(front)
            tgt_gated += target[c] in hit_cells(out[c, :ocnt[c]])
    print(f"discrete: {in_ca} of {n_cpi} CPIs in the CA list, {in_gated} in the gated one; target from age 4: {tgt_ca} / {tgt_gated} of {n_cpi - 4}")
    assert in_ca >= n_cpi - 2 and in_gated == 0
    assert tgt_gated == tgt_ca >= n_cpi - 6
