"""The ordered-statistic detector kernels (csrc/oscfar_kernels.hpp) on the crafted maps of tests/cfar_crafted.py.

Every case hands the same complex64 maps to ``OsCfarDetector1D`` / ``OsCfarDetector2D.process_dev`` and to the fp64 NumPy
restatement ``oscfar_hits`` fed with blah2hip_oscfar_alpha's own tables.  The rule is a count of fp64 multiply-compares
on values that round once (include/blah2hip.h), so there is no margin band: the hit sets (row, col) per CPI are EQUAL, the
counts with them, and snr agrees within 1e-9.  With cap below the count the count is still the true one and the stored
records are cap members of the expected set.

  oscfar1d_kernel<true>    test_one_d (all but 19 201 bins), test_one_d_groups, test_ranks, test_flat_map_with_ties, test_looks,
                           test_masking_scene, test_detect_dev_on_an_os_list, test_cell_averaging_detectors_are_undisturbed
  oscfar1d_kernel<false>   test_one_d (19 201 delay bins)
  oscfar2d_kernel          test_two_d_shapes, test_two_d_windows, test_two_d_values, test_two_d_batch,
                           test_two_d_without_doppler_cells_is_one_d, test_ranks, test_flat_map_with_ties
"""
from dataclasses import replace
from functools import lru_cache

import numpy as np
import pytest

import cfar_crafted as X

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)
PAD = 64
SNR_TOL = 1e-9


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


def handle(b2, case):
    key = (case.geom, case.B)
    if key not in _handles:
        g, d = case.geom, X.dims_of(case.geom)
        amb = b2.Ambiguity(g[0], g[1], g[2], g[3], g[4], g[5], False, max_batch=case.B, n_doppler_bins=g[6])
        assert (amb.get_n_doppler_bins(), amb.get_n_delay_bins()) == (d.n_doppler_bins, d.n_delay_bins)
        assert np.array_equal(amb.delay, d.delay) and np.array_equal(amb.doppler, d.doppler)
        _handles[key] = amb
    return _handles[key]


@pytest.fixture(scope="module", autouse=True)
def release_handles():
    yield
    _handles.clear()


@lru_cache(maxsize=None)
def tables(pfa, looks, pm, max_n):
    import blah2_amd
    return blah2_amd.oscfar_alpha_table(pfa, looks, pm, max_n)


def table_size(w4):
    return (2 * (w4[0] + w4[1]) + 1) * (2 * (w4[2] + w4[3]) + 1)


def expected(b2, case, maps, metrics, window=None, pm=750, looks=1):
    """Per CPI {(row, col): snr} of the restatement with the library's tables for the size the entry point asks for."""
    w = tuple(window if window is not None else case.window)
    w4 = w if len(w) == 4 else (w[0], w[1], 0, 0)
    alpha, rank = tables(case.pfa, looks, pm, 2 * w[1] if len(w) == 2 else table_size(w4))
    d = X.dims_of(case.geom)
    out = []
    for c in range(maps.shape[0]):
        r, k, s = b2.oscfar_hits(maps[c], d.delay, d.doppler, metrics[c, 0], alpha, rank, w, case.min_delay, case.min_doppler)
        out.append({(int(i), int(j)): float(v) for i, j, v in zip(r, k, s)})
    return out


def arena(torch, words, fill):
    whole = torch.full((words + PAD,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    whole[:words] = int(np.uint32(fill).view(np.int32))
    return whole


def launch(b2, torch, amb, case, d_map, d_met, cap, window=None, rank=0.75, looks=1):
    """One detector call into guarded arenas -> (counts [B], records per CPI as HIT_DTYPE arrays of the stored length)."""
    w = tuple(window if window is not None else case.window)
    B = case.B
    hits = arena(torch, B * cap * 4, GUARD)
    cnt = arena(torch, B, 0xDEADBEEF)  # the call zeroes the counts itself
    st = torch.cuda.current_stream().cuda_stream
    if len(w) == 2:
        det = b2.OsCfarDetector1D(case.pfa, w[0], w[1], case.min_delay, case.min_doppler, rank=rank, looks=looks)
    else:
        det = b2.OsCfarDetector2D(case.pfa, *w, case.min_delay, case.min_doppler, rank=rank, looks=looks)
    det.process_dev(amb, B, hits.data_ptr(), cap, cnt.data_ptr(), d_map.data_ptr(), d_met.data_ptr(), st)
    torch.cuda.synchronize()
    amb.set_cfar_looks(1)
    hw, cw = hits.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)
    assert (hw[-PAD:] == GUARD).all(), (case.name, "words behind the hit arena were written")
    assert (cw[-PAD:] == GUARD).all(), (case.name, "words behind the counts were written")
    counts = cw[:B].copy()
    raw = hw[:B * cap * 4].reshape(B, cap, 4)
    recs = []
    for c in range(B):
        stored = min(int(counts[c]), cap)
        assert (raw[c, stored:] == GUARD).all(), (case.name, c, "a slot beyond the count was written")
        recs.append(np.ascontiguousarray(raw[c, :stored]).view(b2.HIT_DTYPE).reshape(-1))
    return counts, recs


def compare(case, ref, counts, recs, cap, tag=""):
    for c in range(len(ref)):
        t = (case.name, tag, f"cpi {c}")
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
            assert s == want or abs(s - want) <= SNR_TOL, (*t, cell, s, want)


def run_case(b2, torch, case, window=None, rank=0.75, looks=1, caps=None):
    maps, metrics = X.make_maps(case)
    ref = expected(b2, case, maps, metrics, window, int(round(rank * 1000)), looks)
    amb = handle(b2, case)
    d_map, d_met = torch.from_numpy(maps).cuda(), torch.from_numpy(metrics).cuda()
    for cap in caps or [maps.shape[1] * maps.shape[2]]:
        counts, recs = launch(b2, torch, amb, case, d_map, d_met, cap, window, rank, looks)
        compare(case, ref, counts, recs, cap, f"cap {cap}")
    return ref


# ------------------------------------------------------------------------------------------------------- 1-D --
def test_one_d(b2, torch):
    """The column-0 quirk, windows wider than the row, one column, a batch of three, 19 200 / 19 201 bins either side of
    the LDS limit."""
    for case in X.one_d_cases():
        ref = run_case(b2, torch, case)
        if X.dims_of(case.geom).n_delay_bins > 2:
            assert len(ref[0]) > 0, case.name


@pytest.mark.parametrize("group", ["values", "dead", "mindelay"])
def test_one_d_groups(b2, torch, group):
    cases = [c for c in {"values": X.value_cases, "dead": X.dead_row_cases, "mindelay": X.min_delay_cases}[group]() if c.one_d]
    assert len(cases) >= 4
    total = 0
    for case in cases:
        ref = run_case(b2, torch, case)
        total += sum(len(h) for h in ref)
        if case.kind == "zero" or case.name.endswith("above"):
            assert all(len(h) == 0 for h in ref), case.name
    assert total > 0


def test_one_d_overflow(b2, torch):
    """cap below the count: the count is the true one and the first cap records are members of the expected set."""
    cases = [c for c in X.overflow_cases() if c.one_d]
    assert cases
    for case in cases:
        maps, metrics = X.make_maps(case)
        n = [len(h) for h in expected(b2, case, maps, metrics)]
        assert min(n) > 2
        run_case(b2, torch, case, caps=sorted({1, min(n) - 1, max(n) - 1, max(n)}))


# ------------------------------------------------------------------------------------------------------- 2-D --
@pytest.mark.parametrize("w", [(2, 6, 1, 3), X.TILE_NL3], ids=["w2_6_1_3", "w6_34_2_4"])
def test_two_d_shapes(b2, torch, w):
    """The map shapes at the tile's column and row seams (64 columns, 16 rows) and below one tile."""
    total = 0
    for case in X.shape_cases(w):
        total += sum(len(h) for h in run_case(b2, torch, case))
    assert total > 0


@pytest.mark.parametrize("w", [(0, 0, 0, 1), (0, 1, 0, 0), X.TILE_NOLDS], ids=["w0_0_0_1", "w0_1_0_0", "w5_27_3_21"])
def test_two_d_windows(b2, torch, w):
    ref = run_case(b2, torch, X.Case("os-window-" + "_".join(map(str, w)), X.geom(60, 140), w))
    assert len(ref[0]) > 0


def test_two_d_values(b2, torch):
    cases = [c for c in X.value_cases() if not c.one_d]
    assert len(cases) == 12
    for case in cases:
        ref = run_case(b2, torch, case)
        assert (len(ref[0]) == 0) == (case.kind == "zero"), case.name


def test_two_d_batch(b2, torch):
    case = X.Case("os-batch", X.geom(70, 130), (2, 6, 1, 3), B=3)
    ref = run_case(b2, torch, case)
    assert len({frozenset(h) for h in ref}) == 3 and min(len(h) for h in ref) > 0
    n = [len(h) for h in ref]
    run_case(b2, torch, case, caps=[1, min(n) - 1])


def test_two_d_window_beyond_the_halo_is_unsupported(b2, torch):
    from blah2_amd import _lib
    case = X.Case("os-unsupported", X.geom(40, 100), X.SAT_ONLY)
    amb = handle(b2, case)
    buf = torch.zeros(64, dtype=torch.int32, device="cuda")
    for w in (X.SAT_ONLY, (1, 40, 0, 0), (0, 0, 5, 20)):
        with pytest.raises(b2.Blah2HipError) as e:
            b2.OsCfarDetector2D(1e-3, *w, -128, 0.0).process_dev(amb, 1, buf.data_ptr(), 1, buf.data_ptr() + 128)
        assert e.value.code == _lib.ERR_UNSUPPORTED
        assert amb._L.blah2hip_oscfar2d_prepare(amb._h, 1e-3, 750, *w) == _lib.ERR_UNSUPPORTED
    assert amb._L.blah2hip_oscfar2d_prepare(amb._h, 1e-3, 750, 2, 6, 1, 3) == _lib.OK
    assert amb._L.blah2hip_oscfar2d_prepare(amb._h, 1e-3, 0, 2, 6, 1, 3) == _lib.ERR_INVALID
    assert amb._L.blah2hip_oscfar1d_prepare(amb._h, 1e-3, 1001, 6) == _lib.ERR_INVALID
    torch.cuda.synchronize()


def test_two_d_without_doppler_cells_is_one_d(b2, torch):
    for base in (X.Case("os-1d-as-2d", X.geom(33, 257), (2, 6), B=3), X.Case("os-1d-as-2d-quirk", X.geom(9, 40), (0, 1)),
                 X.Case("os-1d-as-2d-min", X.geom(21, 71, -10), (2, 6), min_delay=-4, min_doppler=3.0)):
        one = run_case(b2, torch, base)
        two = run_case(b2, torch, base, window=(base.window[0], base.window[1], 0, 0))
        assert one == two and sum(len(h) for h in one) > 0


# ------------------------------------------------------------------------------------------ other properties --
@pytest.mark.parametrize("rank", [0.001, 0.5, 0.75, 1.0])
def test_ranks(b2, torch, rank):
    sizes = []
    for case in (X.Case("os-rank-1d", X.geom(33, 257), (2, 6), pfa=1e-2), X.Case("os-rank-2d", X.geom(40, 100), (2, 6, 1, 3), pfa=1e-2)):
        ref = run_case(b2, torch, case, rank=rank)
        sizes.append(len(ref[0]))
    assert min(sizes) > 0


def test_flat_map_with_ties(b2, torch):
    """Every power equal: ties at every rank.  Nothing hits but the planted cells, and two equal planted cells in each
    other's window survive rank 750 and mask each other at rank 1000."""
    for window in ((2, 6), (2, 6, 1, 3)):
        case = X.Case("os-flat-" + str(len(window)), X.geom(20, 100), window, pfa=1e-3)
        d = X.dims_of(case.geom)
        maps = np.ones((1, d.n_doppler_bins, d.n_delay_bins), dtype=np.complex64)
        for i, j in ((0, 0), (0, 1), (7, 63), (7, 67), (19, 99), (12, 30)):
            maps[0, i, j] = np.float32(40.0)
        metrics = np.array([[2.5, 0.0]])
        amb = handle(b2, case)
        d_map, d_met = torch.from_numpy(maps).cuda(), torch.from_numpy(metrics).cuda()
        cap = maps[0].size
        got = {}
        for rank in (0.75, 1.0):
            ref = expected(b2, case, maps, metrics, pm=int(rank * 1000))
            counts, recs = launch(b2, torch, amb, case, d_map, d_met, cap, rank=rank)
            compare(case, ref, counts, recs, cap, f"rank {rank}")
            got[rank] = set(ref[0])
        assert got[0.75] == {(0, 0), (0, 1), (7, 63), (7, 67), (19, 99), (12, 30)}
        assert (7, 63) not in got[1.0] and (7, 67) not in got[1.0] and (12, 30) in got[1.0]


def test_looks(b2, torch):
    """BLAH2HIP_OPT_CFAR_LOOKS = 4: the sets are those of the L = 4 tables and differ from the L = 1 sets."""
    for case in (X.Case("os-looks-1d", X.geom(33, 257), (2, 6), pfa=1e-3), X.Case("os-looks-2d", X.geom(40, 100), (2, 6, 1, 3), pfa=1e-3)):
        one = run_case(b2, torch, case, looks=1)
        four = run_case(b2, torch, case, looks=4)
        assert set(one[0]) < set(four[0])  # the L = 4 factors are lower at every n


def test_cell_averaging_detectors_are_undisturbed(b2, torch):
    """Thirteen ordered-statistic calls with distinct pfas on one handle (more than either cache holds): the averaging
    detectors give the lists they gave before, and the timing table has the slots it had."""
    from blah2_amd import _lib
    case = X.Case("os-undisturbed", X.geom(40, 100), (2, 6, 1, 3), pfa=X.PFAS[0])
    maps, metrics = X.make_maps(case)
    amb = handle(b2, case)
    amb.set_timing(True)
    d_map, d_met = torch.from_numpy(maps).cuda(), torch.from_numpy(metrics).cuda()
    cap = maps[0].size
    st = torch.cuda.current_stream().cuda_stream

    def ca_lists():
        out = []
        for det in (b2.CfarDetector1D(case.pfa, 2, 6, case.min_delay, case.min_doppler),
                    b2.CfarDetector2D(case.pfa, 2, 6, 1, 3, case.min_delay, case.min_doppler)):
            hits = torch.zeros((cap, 2), dtype=torch.float64, device="cuda")
            cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
            det.process_dev(amb, 1, hits.data_ptr(), cap, cnt.data_ptr(), d_map.data_ptr(), d_met.data_ptr(), st)
            torch.cuda.synchronize()
            r = hits.cpu().numpy().view(b2.HIT_DTYPE).reshape(-1)[:int(cnt.cpu()[0])]
            out.append(sorted(zip(r["row"].tolist(), r["col"].tolist(), r["snr"].tolist())))
        return out

    before = ca_lists()
    slots = amb.get_timing()
    assert min(len(x) for x in before) > 0 and set(slots) == set(_lib.KERNEL_NAMES.values()) and len(slots) == _lib.K_COUNT
    sizes = set()
    for k, pfa in enumerate(X.PFAS):
        c = replace(case, pfa=pfa, window=(2, 6) if k % 2 else (2, 6, 1, 3))
        counts, recs = launch(b2, torch, amb, c, d_map, d_met, cap)
        compare(c, expected(b2, c, maps, metrics), counts, recs, cap)
        sizes.add((k % 2, int(counts[0])))
    assert len(X.PFAS) == 13 and len(sizes) > 6
    # the first tuple again, behind the evictions of its own cache
    counts, recs = launch(b2, torch, amb, case, d_map, d_met, cap)
    compare(case, expected(b2, case, maps, metrics), counts, recs, cap)
    assert ca_lists() == before
    after = amb.get_timing()
    assert list(after) == list(slots) and after["cfar"][1] > 0
    amb.set_timing(False)


def test_detect_dev_on_an_os_list(b2, torch):
    """blah2hip_detect_dev takes the ordered-statistic hit list as it takes the averaging detectors': Centroid and
    Interpolate on the device equal the host functions on the restatement's list."""
    case = X.Case("os-detect", X.geom(33, 257), (2, 6), pfa=1e-3)
    maps, metrics = X.make_maps(case)
    ref = expected(b2, case, maps, metrics)[0]
    d = X.dims_of(case.geom)
    amb = handle(b2, case)
    d_map, d_met = torch.from_numpy(maps).cuda(), torch.from_numpy(metrics).cuda()
    cap = maps[0].size
    st = torch.cuda.current_stream().cuda_stream
    d_hits = torch.zeros((cap, 2), dtype=torch.float64, device="cuda")
    d_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_out = torch.zeros((cap, 4), dtype=torch.float64, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
    res = float(d.doppler[1] - d.doppler[0])
    b2.OsCfarDetector1D(case.pfa, 2, 6, case.min_delay, case.min_doppler).process_dev(
        amb, 1, d_hits.data_ptr(), cap, d_cnt.data_ptr(), d_map.data_ptr(), d_met.data_ptr(), st)
    b2.DetectionFinisher(6, 6, res).process_dev(amb, 1, d_hits.data_ptr(), cap, d_cnt.data_ptr(), d_out.data_ptr(), cap,
                                                d_n.data_ptr(), d_map.data_ptr(), d_met.data_ptr(), st)
    torch.cuda.synchronize()
    got = b2.dets_to_detection(d_out.cpu().numpy().view(b2.DET_DTYPE).reshape(-1), int(d_n.cpu()[0]), cap)
    cells = sorted(ref)
    det = b2.Detection([j + float(d.delay[0]) for _, j in cells], [d.doppler[i] for i, _ in cells], [ref[c] for c in cells])
    m = b2.Map(None, maps[0], d.delay, d.doppler, float(metrics[0, 0]), float(metrics[0, 1]))
    want = b2.Interpolate(True, True).process(b2.Centroid(6, 6, res).process(det), m)
    assert int(d_cnt.cpu()[0]) == len(ref) >= want.get_nDetections() > 0
    assert got.get_nDetections() == want.get_nDetections()
    assert np.allclose(got.get_delay(), want.get_delay(), rtol=0, atol=1e-9)
    assert np.allclose(got.get_doppler() / res, want.get_doppler() / res, rtol=0, atol=1e-9)
    assert np.allclose(got.get_snr(), want.get_snr(), rtol=0, atol=1e-9)


def test_masking_scene(b2, torch):
    """test_oscfar_model.py's scene on the device: CfarDetector1D misses the middle one of three equal echoes four cells
    apart, OsCfarDetector1D reports it."""
    from test_oscfar_model import masking_scene
    case = X.Case("os-masking", X.geom(3, 40), (2, 6), pfa=1e-3)
    maps = masking_scene(3, 40)[None]
    metrics = np.array([[0.0, 0.0]])
    amb = handle(b2, case)
    d_map, d_met = torch.from_numpy(maps).cuda(), torch.from_numpy(metrics).cuda()
    cap = maps[0].size
    st = torch.cuda.current_stream().cuda_stream
    hits = torch.zeros((cap, 2), dtype=torch.float64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    b2.CfarDetector1D(1e-3, 2, 6, -128, 0.0).process_dev(amb, 1, hits.data_ptr(), cap, cnt.data_ptr(), d_map.data_ptr(),
                                                          d_met.data_ptr(), st)
    torch.cuda.synchronize()
    r = hits.cpu().numpy().view(b2.HIT_DTYPE).reshape(-1)[:int(cnt.cpu()[0])]
    ca = set(zip(r["row"].tolist(), r["col"].tolist()))
    counts, recs = launch(b2, torch, amb, case, d_map, d_met, cap)
    compare(case, expected(b2, case, maps, metrics), counts, recs, cap)
    os_ = set(zip(recs[0]["row"].tolist(), recs[0]["col"].tolist()))
    for row in range(3):
        assert (row, 20) not in ca and (row, 20) in os_
    assert os_ == {(i, j) for i in range(3) for j in (16, 20, 24)}
