"""The greatest-of / smallest-of detector kernels (csrc/gocfar_kernels.hpp) on the crafted maps of tests/gocfar_crafted.py.

Every case hands the same complex64 maps to ``GoCfarDetector1D`` / ``GoCfarDetector2D.process_dev`` and to the fp64 NumPy
restatement ``gocfar_hits`` fed with blah2hip_gocfar_alpha's own factors for the pairs the map's geometry gives.  The rule
is two fp64 divide-multiply-compares on sums with a defined order of additions (include/blah2hip.h), so there is no margin
band: the hit sets (row, col) per CPI are EQUAL, the counts with them, and snr agrees within 1e-9.  With cap below the count
the count is still the true one and the stored records are cap members of the expected set.

  gocfar1d_kernel<true>    test_one_d (all but 19 201 bins), test_one_d_long_windows, test_one_d_nonfinite, test_one_d_skips,
                           test_one_d_batch_and_cap, test_prepare_then_a_graph, test_process_host_map
  gocfar1d_kernel<false>   test_one_d (19 201 delay bins)
  gocfar2d_kernel          test_two_d_seams, test_two_d_small_map, test_two_d_halo_limits, test_two_d_batch,
                           test_two_d_without_rows_is_one_d
"""
import numpy as np
import pytest

import gocfar_crafted as G

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)
PAD = 64
SNR_TOL = 1e-9
KINDS = ["go", "so"]
PFA = 0.02


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


def handle(b2, geom, B):
    key = (geom, B)
    if key not in _handles:
        d = G.dims_of(geom)
        amb = b2.Ambiguity(geom[0], geom[1], geom[2], geom[3], geom[4], geom[5], False, max_batch=B, n_doppler_bins=geom[6])
        assert (amb.get_n_doppler_bins(), amb.get_n_delay_bins()) == (d.n_doppler_bins, d.n_delay_bins)
        _handles[key] = amb
    return _handles[key]


@pytest.fixture(scope="module", autouse=True)
def release_handles():
    yield
    _handles.clear()


def expected(b2, geom, maps, metrics, kind, window, pfa=PFA, min_delay=-128, min_doppler=0.0):
    """Per CPI {(row, col): snr} of the restatement with the library's own factors."""
    d = G.dims_of(geom)
    table = b2.gocfar_table_for(pfa, kind, d.n_doppler_bins, d.n_delay_bins, window)
    return [G.hits_dict(b2.gocfar_hits(maps[c], d.delay, d.doppler, metrics[c, 0], table, kind, window, min_delay, min_doppler))
            for c in range(maps.shape[0])]


def arena(torch, words, fill):
    whole = torch.full((words + PAD,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    whole[:words] = int(np.uint32(fill).view(np.int32))
    return whole


def detector(b2, kind, window, pfa=PFA, min_delay=-128, min_doppler=0.0):
    w = tuple(window)
    return (b2.GoCfarDetector1D if len(w) == 2 else b2.GoCfarDetector2D)(pfa, *w, min_delay, min_doppler, kind=kind)


def launch(b2, torch, amb, det, B, d_map, d_met, cap, name=""):
    """One detector call into guarded arenas -> (counts [B], records per CPI as HIT_DTYPE arrays of the stored length)."""
    hits = arena(torch, B * cap * 4, GUARD)
    cnt = arena(torch, B, 0xDEADBEEF)  # the call zeroes the counts itself
    st = torch.cuda.current_stream().cuda_stream
    det.process_dev(amb, B, hits.data_ptr(), cap, cnt.data_ptr(), d_map.data_ptr(), d_met.data_ptr(), st)
    torch.cuda.synchronize()
    return read_arenas(b2, hits, cnt, B, cap, name)


def read_arenas(b2, hits, cnt, B, cap, name=""):
    hw, cw = hits.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)
    assert (hw[-PAD:] == GUARD).all(), (name, "words behind the hit arena were written")
    assert (cw[-PAD:] == GUARD).all(), (name, "words behind the counts were written")
    counts = cw[:B].copy()
    raw = hw[:B * cap * 4].reshape(B, cap, 4)
    recs = []
    for c in range(B):
        stored = min(int(counts[c]), cap)
        assert (raw[c, stored:] == GUARD).all(), (name, c, "a slot beyond the count was written")
        recs.append(np.ascontiguousarray(raw[c, :stored]).view(b2.HIT_DTYPE).reshape(-1))
    return counts, recs


def compare(name, ref, counts, recs, cap):
    for c in range(len(ref)):
        t = (name, f"cap {cap}", f"cpi {c}")
        assert int(counts[c]) == len(ref[c]), (*t, "count", int(counts[c]), len(ref[c]))
        cells = list(zip(recs[c]["row"].tolist(), recs[c]["col"].tolist()))
        got = set(cells)
        assert len(got) == len(cells), (*t, "a cell was reported twice")
        if len(ref[c]) <= cap:
            assert got == set(ref[c]), (*t, "missing", sorted(set(ref[c]) - got)[:8], "extra", sorted(got - set(ref[c]))[:8])
        else:
            assert len(cells) == cap and got <= set(ref[c]), (*t, "stored hits the restatement lacks", sorted(got - set(ref[c]))[:8])
        for cell, s in zip(cells, recs[c]["snr"].tolist()):
            want = ref[c][cell]
            assert s == want or abs(s - want) <= SNR_TOL or (np.isinf(s) and s == want), (*t, cell, s, want)


def run_case(b2, torch, name, geom, window, kind, B=1, caps=None, maps=None, **kw):
    d = G.dims_of(geom)
    if maps is None:
        maps = G.noise_map(name, d.n_doppler_bins, d.n_delay_bins, B)
    metrics = G.metrics_for(B)
    ref = expected(b2, geom, maps, metrics, kind, window, **kw)
    amb = handle(b2, geom, B)
    d_map, d_met = torch.from_numpy(maps).cuda(), torch.from_numpy(metrics).cuda()
    det = detector(b2, kind, window, **kw)
    for cap in caps or [maps.shape[1] * maps.shape[2]]:
        counts, recs = launch(b2, torch, amb, det, B, d_map, d_met, cap, name)
        compare(name, ref, counts, recs, cap)
    return ref


# ------------------------------------------------------------------------------------------------------- 1-D --
@pytest.mark.parametrize("kind", KINDS)
def test_one_d(b2, torch, kind):
    """Rows of 5 ... 257 delay bins in LDS and 19 201 bins (3 rows) straight from the map; a huge cell in delay column 0."""
    for nD, nC in ((6, 5), (6, 17), (6, 64), (6, 65), (6, 257), (3, 19201)):
        geom = G.geom(nD, nC) if nC < 19201 else G.geom(nD, nC, -10, n_corr=16384)  # (|delay| stays below the transform's length)
        ref = run_case(b2, torch, f"go-1d-{nC}", geom, (2, 8), kind)
        assert nC == 5 or len(ref[0]) > 0, nC


@pytest.mark.parametrize("kind", KINDS)
def test_one_d_long_windows(b2, torch, kind):
    """Windows longer than the row: every (a, b) with an empty half occurs, and both-empty cells."""
    total = 0
    for nC, w in ((5, (0, 127)), (17, (1, 20)), (17, (16, 3)), (17, (20, 5)), (64, (2, 70)), (9, (0, 1)), (9, (3, 0))):
        d = G.dims_of(G.geom(6, nC))
        a, b = b2.gocfar_counts(d.n_doppler_bins, nC, w)
        if w in ((1, 20), (0, 127), (2, 70)):
            assert ((a == 0) & (b > 0)).any() and ((b == 0) & (a > 0)).any()
        total += len(run_case(b2, torch, f"go-1d-long-{nC}-{w[0]}-{w[1]}", G.geom(6, nC), w, kind)[0])
    assert total > 0


@pytest.mark.parametrize("kind", KINDS)
def test_one_d_nonfinite(b2, torch, kind):
    """NaN and +Inf inside the row: each is a training cell of its neighbours and a cell under test."""
    geom = G.geom(9, 65)
    maps = G.noise_map("go-1d-nonfinite", 9, 65, 1, nonfinite=True)
    ref = run_case(b2, torch, "go-1d-nonfinite", geom, (2, 8), kind, maps=maps)
    assert (3, 21) not in ref[0]  # the NaN cell never hits
    zero = run_case(b2, torch, "go-1d-zero", geom, (2, 8), kind, maps=np.zeros_like(maps))
    assert len(zero[0]) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_one_d_skips(b2, torch, kind):
    geom = G.geom(21, 71, -10)
    full = run_case(b2, torch, "go-1d-skips", geom, (2, 8), kind)
    cut = run_case(b2, torch, "go-1d-skips", geom, (2, 8), kind, min_delay=-4, min_doppler=3.0)
    d = G.dims_of(geom)
    assert 0 < len(cut[0]) < len(full[0])
    assert all(d.delay[j] >= -4 and abs(d.doppler[i]) >= 3.0 for i, j in cut[0])


@pytest.mark.parametrize("kind", KINDS)
def test_one_d_batch_and_cap(b2, torch, kind):
    """Three CPIs a call; cap below the count of one of them, of all of them, and at the largest count."""
    geom = G.geom(12, 130)
    d = G.dims_of(geom)
    maps = G.noise_map("go-1d-batch", 12, 130, 3)
    n = [len(h) for h in expected(b2, geom, maps, G.metrics_for(3), kind, (2, 8))]
    assert min(n) > 2 and len(set(n)) > 1
    run_case(b2, torch, "go-1d-batch", geom, (2, 8), kind, B=3, maps=maps, caps=sorted({1, min(n) - 1, max(n) - 1, max(n), d.n_delay_bins * 12}))


# ------------------------------------------------------------------------------------------------------- 2-D --
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w", [(2, 6, 4), (1, 3, 1), (0, 1, 7)], ids=["w2_6_4", "w1_3_1", "w0_1_7"])
def test_two_d_seams(b2, torch, kind, w):
    """Tile seams (16 rows, 64 columns) and ragged last tiles on both axes: 33 x 130 has two whole tiles and a rest of one row
    and of two columns; 16 x 64 is exactly one tile; 17 x 65 one row and one column more."""
    total = 0
    for nD, nC in ((33, 130), (16, 64), (17, 65)):
        assert (nD % G.G2_ROWS, nC % G.G2_COLS) in ((1, 2), (0, 0), (1, 1))
        total += len(run_case(b2, torch, f"go-2d-seams-{nD}x{nC}", G.geom(nD, nC), w, kind)[0])
    assert total > 0


@pytest.mark.parametrize("kind", KINDS)
def test_two_d_small_map(b2, torch, kind):
    """3 x 7 cells under a window larger than the map: every half is clipped on every side."""
    for w in ((2, 8, 5), (0, 3, 2)):
        run_case(b2, torch, "go-2d-small", G.geom(3, 7), w, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_two_d_halo_limits(b2, torch, kind):
    ref = run_case(b2, torch, "go-2d-halo", G.geom(50, 90), (6, 34, G.MAX_HR), kind)
    assert G.MAX_HC == 6 + 34 and len(ref[0]) > 0


@pytest.mark.parametrize("kind", KINDS)
def test_two_d_batch(b2, torch, kind):
    """Two CPIs, with NaN and +Inf cells, the skips, and caps below the counts."""
    geom = G.geom(35, 70, -10)
    maps = G.noise_map("go-2d-batch", 35, 70, 2, nonfinite=True)
    ref = run_case(b2, torch, "go-2d-batch", geom, (2, 6, 3), kind, B=2, maps=maps)
    n = [len(h) for h in ref]
    assert min(n) > 2 and frozenset(ref[0]) != frozenset(ref[1])
    run_case(b2, torch, "go-2d-batch", geom, (2, 6, 3), kind, B=2, maps=maps, caps=[1, min(n) - 1])
    cut = run_case(b2, torch, "go-2d-batch", geom, (2, 6, 3), kind, B=2, maps=maps, min_delay=-4, min_doppler=3.0)
    assert 0 < len(cut[0]) < n[0]


@pytest.mark.parametrize("kind", KINDS)
def test_two_d_without_rows_is_one_d(b2, torch, kind):
    """hR = 0: the 1-D detector's hits and snr, bit for bit."""
    for name, geom, w, B, kw in (("go-1d-as-2d", G.geom(33, 257), (2, 8), 3, {}), ("go-1d-as-2d-quirk", G.geom(9, 40), (0, 1), 1, {}),
                                ("go-1d-as-2d-min", G.geom(21, 71, -10), (2, 6), 1, {"min_delay": -4, "min_doppler": 3.0})):
        d = G.dims_of(geom)
        maps = G.noise_map(name, d.n_doppler_bins, d.n_delay_bins, B, nonfinite=True)
        amb = handle(b2, geom, B)
        d_map, d_met = torch.from_numpy(maps).cuda(), torch.from_numpy(G.metrics_for(B)).cuda()
        cap = maps[0].size
        out = []
        for window in (w, (w[0], w[1], 0)):
            counts, recs = launch(b2, torch, amb, detector(b2, kind, window, **kw), B, d_map, d_met, cap, name)
            out.append([sorted(zip(r["row"].tolist(), r["col"].tolist(), r["snr"].view(np.uint64).tolist())) for r in recs])
        assert out[0] == out[1] and sum(len(x) for x in out[0]) > 0
        run_case(b2, torch, name, geom, (w[0], w[1], 0), kind, B=B, maps=maps, **kw)


# ------------------------------------------------------------------------------------------ other properties --
def test_go_and_so_differ_from_each_other_and_from_averaging(b2, torch):
    geom = G.geom(12, 130)
    maps = G.noise_map("go-kinds", 12, 130, 1)
    go = run_case(b2, torch, "go-kinds", geom, (2, 8), "go", maps=maps)[0]
    so = run_case(b2, torch, "go-kinds", geom, (2, 8), "so", maps=maps)[0]
    assert set(go) != set(so) and len(go) > 0 and len(so) > 0


def test_prepare_then_a_graph(b2, torch):
    """_prepare pins the table; a graph captured afterwards replays the detector; a pfa that was not prepared is refused
    while the stream is being captured, with a message that names _prepare, and writes nothing."""
    from blah2_amd import _lib
    geom, B, w = G.geom(12, 130), 1, (2, 8)
    maps = G.noise_map("go-graph", 12, 130, B)
    metrics = G.metrics_for(B)
    amb = handle(b2, geom, B)
    d_map, d_met = torch.from_numpy(maps).cuda(), torch.from_numpy(metrics).cuda()
    cap = maps[0].size
    for kind, det2 in (("go", (2, 6, 2)), ("so", None)):
        window = det2 or w
        ref = expected(b2, geom, maps, metrics, kind, window, pfa=0.0125)
        det = detector(b2, kind, window, pfa=0.0125)
        det.prepare(amb)
        missing = detector(b2, kind, window, pfa=0.0126)
        hits, cnt = arena(torch, B * cap * 4, GUARD), arena(torch, B, 0xDEADBEEF)
        other, other_cnt = arena(torch, B * cap * 4, GUARD), arena(torch, B, 0xDEADBEEF)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):  # one stream, a memset and a kernel in a chain: no parallel branches
            st = torch.cuda.current_stream().cuda_stream
            det.process_dev(amb, B, hits.data_ptr(), cap, cnt.data_ptr(), d_map.data_ptr(), d_met.data_ptr(), st)
            with pytest.raises(b2.Blah2HipError) as e:
                missing.process_dev(amb, B, other.data_ptr(), cap, other_cnt.data_ptr(), d_map.data_ptr(), d_met.data_ptr(), st)
        assert e.value.code == _lib.ERR_INVALID and "_prepare" in str(e.value)
        torch.cuda.synchronize()
        assert (hits.cpu().numpy().view(np.uint32) == GUARD).all()  # captured, not run
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            counts, recs = read_arenas(b2, hits, cnt, B, cap, "graph")
            compare("go-graph", ref, counts, recs, cap)
        assert (other.cpu().numpy().view(np.uint32) == GUARD).all()
        assert (other_cnt.cpu().numpy().view(np.uint32)[:B] == 0xDEADBEEF).all()


def test_refusals_write_nothing(b2, torch):
    """Every refusal of the _dev and _prepare calls: the error code, and d_hits / d_count untouched."""
    from blah2_amd import _lib
    geom, B = G.geom(12, 130), 1
    amb = handle(b2, geom, B)
    L, h = amb._L, amb._h
    maps = G.noise_map("go-refusals", 12, 130, B)
    d_map, d_met = torch.from_numpy(maps).cuda(), torch.from_numpy(G.metrics_for(B)).cuda()
    cap = 16
    hits, cnt = arena(torch, B * cap * 4, GUARD), arena(torch, B, 0xDEADBEEF)
    # (h, d_map, d_metrics, n_cpi, pfa, kind, nGuard, nTrain, minDelay, minDoppler, d_hits, cap, d_count, stream)
    good1 = [h, d_map.data_ptr(), d_met.data_ptr(), 1, 1e-3, 1, 2, 8, -128, 0.0, hits.data_ptr(), cap, cnt.data_ptr(), None]
    bad1 = {"NULL handle": ({0: None}, _lib.ERR_INVALID), "NULL hits": ({10: None}, _lib.ERR_INVALID),
            "NULL count": ({12: None}, _lib.ERR_INVALID), "n_cpi 0": ({3: 0}, _lib.ERR_INVALID), "n_cpi 2": ({3: 2}, _lib.ERR_INVALID),
            "kind 0": ({5: 0}, _lib.ERR_INVALID), "kind 3": ({5: 3}, _lib.ERR_INVALID), "pfa 0": ({4: 0.0}, _lib.ERR_INVALID),
            "pfa 1": ({4: 1.0}, _lib.ERR_INVALID), "pfa nan": ({4: float("nan")}, _lib.ERR_INVALID),
            "nGuard 128": ({6: 128}, _lib.ERR_INVALID), "nTrain -1": ({7: -1}, _lib.ERR_INVALID), "minDelay 128": ({8: 128}, _lib.ERR_INVALID)}
    # (..., kind, nGd, nTd, hR, minDelay, ...)
    good2 = good1[:6] + [2, 6, 4, -128] + good1[9:]
    bad2 = {"NULL hits": ({11: None}, _lib.ERR_INVALID), "NULL count": ({13: None}, _lib.ERR_INVALID), "kind 7": ({5: 7}, _lib.ERR_INVALID), "pfa 2": ({4: 2.0}, _lib.ERR_INVALID),
            "hR 25": ({8: 25}, _lib.ERR_UNSUPPORTED), "nGd + nTd 41": ({6: 7, 7: 34}, _lib.ERR_UNSUPPORTED),
            "hR -1": ({8: -1}, _lib.ERR_INVALID), "nTd 128": ({7: 128}, _lib.ERR_INVALID), "minDelay -129": ({9: -129}, _lib.ERR_INVALID)}
    for f, good, bad in ((L.blah2hip_gocfar1d_dev, good1, bad1), (L.blah2hip_gocfar2d_dev, good2, bad2)):
        for name, (change, code) in bad.items():
            args = list(good)
            for k, v in change.items():
                args[k] = v
            assert f(*args) == code, name
    amb.set_cfar_looks(2)
    try:
        assert L.blah2hip_gocfar1d_dev(*good1) == _lib.ERR_UNSUPPORTED
        assert L.blah2hip_gocfar2d_dev(*good2) == _lib.ERR_UNSUPPORTED
        assert L.blah2hip_gocfar1d_prepare(h, 1e-3, 1, 2, 8) == _lib.ERR_UNSUPPORTED
        assert L.blah2hip_gocfar2d_prepare(h, 1e-3, 2, 2, 6, 4) == _lib.ERR_UNSUPPORTED
    finally:
        amb.set_cfar_looks(1)
    assert L.blah2hip_gocfar1d_prepare(h, 1e-3, 0, 2, 8) == _lib.ERR_INVALID
    assert L.blah2hip_gocfar1d_prepare(h, 1.5, 1, 2, 8) == _lib.ERR_INVALID
    assert L.blah2hip_gocfar1d_prepare(None, 1e-3, 1, 2, 8) == _lib.ERR_INVALID
    assert L.blah2hip_gocfar2d_prepare(h, 1e-3, 1, 2, 6, 25) == _lib.ERR_UNSUPPORTED
    assert L.blah2hip_gocfar2d_prepare(h, 1e-3, 1, 1, 40, 0) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (hits.cpu().numpy().view(np.uint32) == GUARD).all(), "a refusal wrote to d_hits"
    assert (cnt.cpu().numpy().view(np.uint32)[:B] == 0xDEADBEEF).all(), "a refusal wrote to d_count"
    with pytest.raises(ValueError):
        b2.GoCfarDetector1D(1e-3, 2, 8, -128, 0.0, kind="go", looks=2)
    with pytest.raises(ValueError):
        b2.GoCfarDetector2D(1e-3, 2, 8, 1, -128, 0.0, kind="xo")
    assert L.blah2hip_gocfar1d_dev(*good1) == _lib.OK and L.blah2hip_gocfar2d_dev(*good2) == _lib.OK
    torch.cuda.synchronize()


def test_table_cache_keeps_eight(b2, torch):
    """Thirteen pfas on one handle, then the first again: the lists are right behind the evictions, and the timing counts
    under the detectors' slot."""
    geom, B = G.geom(12, 130), 1
    maps = G.noise_map("go-cache", 12, 130, B)
    metrics = G.metrics_for(B)
    amb = handle(b2, geom, B)
    amb.set_timing(True)
    d_map, d_met = torch.from_numpy(maps).cuda(), torch.from_numpy(metrics).cuda()
    cap = maps[0].size
    pfas = [10.0 ** -(1.0 + 0.25 * k) for k in range(13)]
    for k, pfa in enumerate(pfas + pfas[:1]):
        kind, window = KINDS[k % 2], (2, 8) if k % 3 else (2, 6, 2)
        counts, recs = launch(b2, torch, amb, detector(b2, kind, window, pfa=pfa), B, d_map, d_met, cap)
        compare("go-cache", expected(b2, geom, maps, metrics, kind, window, pfa=pfa), counts, recs, cap)
    assert amb.get_timing()["cfar"][1] > 0
    amb.set_timing(False)


@pytest.mark.parametrize("kind", KINDS)
def test_process_host_map(b2, torch, kind):
    """``process`` on a map held by the host, in the reference's emission order."""
    geom = G.geom(12, 130)
    d = G.dims_of(geom)
    maps = G.noise_map("go-host", 12, 130, 1)
    amb = handle(b2, geom, 1)
    for window in ((2, 8), (2, 6, 2)):
        ref = expected(b2, geom, maps, np.array([[4.5, 0.0]]), kind, window)[0]
        m = b2.Map(None, maps[0], d.delay, d.doppler, 4.5, 0.0)
        det = detector(b2, kind, window).process(m, amb)
        cells = sorted(ref)
        assert det.get_nDetections() == len(cells) > 0
        assert np.array_equal(det.get_delay(), [j + float(d.delay[0]) for _, j in cells])
        assert np.array_equal(det.get_doppler(), [d.doppler[i] for i, _ in cells])
        assert np.allclose(det.get_snr(), [ref[c] for c in cells], rtol=0, atol=SNR_TOL)
