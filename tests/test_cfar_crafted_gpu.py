"""The detector kernels on maps built to break them (tests/cfar_crafted.py), against the additive fp64 oracle.

Every case hands the same complex64 map to a kernel (``process_dev`` of the detectors only: the ambiguity engine never
runs here; a handle only gives the shape and the axes) and to ``oracle.cfar2d_additive`` / ``cfar1d``.

Comparison rule
  * 1-D, tile and stream kernels sum every window additively in fp64 (error bound for 81 x 49 non-negative terms:
    4e-13).  test_oracle_properties.py asserts that no tested cell of any input lies within 1e-9 of its threshold, so
    their hit sets EQUAL the oracle's, and the counts with them.
  * summed-area kernels: a mismatch is allowed only at a cell whose margin |sq/thr - 1| is inside
    8 x 2^-52 x (table value at the window's far corner) / (window sum), from the oracle's own arrays.  The CPU test
    bounds the share of hits inside that band by 1 % per input; measured: 0 on every input, the map spanning
    1e-20 ... 1e18 included (the levels rise along the map, so the prefix at a window's far corner is dominated by the
    window's own rows).
  * snr against 10 log10|z| - noisePower[cpi] of the same cell in NumPy: largest difference measured over this module
    on an MI355X 2.84e-14 dB (one ulp of a value near 200 dB), asserted at 100 x that.
  * row / col of every stored record in range and unique; d_count (pre-filled with garbage) is the true count also
    when it exceeds cap; then exactly cap records are stored, all members of that CPI's own oracle set; the slots of a
    CPI beyond its count, the words behind the arena and behind the counts keep their guard pattern.
  * NaN / +Inf cells: additive kernels equal the oracle (NumPy's compare semantics); the summed-area kernels carry the
    value into every prefix behind the cell and lose detections: they must report no hit the oracle lacks, and the
    number lost is printed.

Which test launches what
  cfar2d_stream_kernel, each of the nine C2S_SHAPES windows    test_shapes[shape-w<window>] (stream and auto)
    the 17 x 9 window besides: test_segment_seams, test_dead_rows, test_min_delay, test_overflow, test_values, test_table_cache
    (2,8,1,4) test_overflow; (1,4,1,2) test_min_delay; (2,5,2,6) test_segment_seams, test_values; (0,0,0,1) test_dead_rows
  cfar2d_tile_kernel<2, true>    every shape-w* of a stream window, test_persistent_tile_walk, and the groups above
  cfar2d_tile_kernel<3, true>    test_shapes[shape-w6_34_2_4], test_persistent_tile_walk, test_values
  cfar2d_tile_kernel<2, false>   test_shapes[shape-w5_27_3_21]
  sat_rows / sat_cols / cfar2d_kernel   every group ('sat' forced; 'auto' for shape-w9_40_5_20)
  cfar1d_kernel<true>            test_one_d, test_dead_rows, test_min_delay, test_overflow, test_values, test_table_cache
  cfar1d_kernel<false>           test_one_d (19 201 delay bins)

Wall time of the module on an MI355X: 4.3 s (471 cases, up to four kernels each).
"""
import numpy as np
import pytest

import cfar_crafted as X

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces
PAD = 64
SNR_TOL = 100 * 2.9e-14  # 100 x the largest difference measured (module docstring)
GROUPS = X.groups()
worst = {"snr": 0.0, "sat_in_band": 0, "sat_hits": 0}


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print(f"\ncrafted detector inputs: largest snr difference {worst['snr']:.3e} dB; summed-area kernels: "
          f"{worst['sat_in_band']} of {worst['sat_hits']} hits inside their band")


_handles = {}


def handle(b2, case):
    """An engine handle of the case's shape and axes (kept: a handle of 1024-sample pulses is small)."""
    key = (case.geom, case.B)
    if key not in _handles:
        g, d = case.geom, X.dims_of(case.geom)
        amb = b2.Ambiguity(g[0], g[1], g[2], g[3], g[4], g[5], False, max_batch=case.B, n_doppler_bins=g[6])
        assert (amb.get_n_doppler_bins(), amb.get_n_delay_bins()) == (d.n_doppler_bins, d.n_delay_bins)
        assert np.array_equal(amb.delay, d.delay) and np.array_equal(amb.doppler, d.doppler)
        _handles[key] = amb
    return _handles[key]


def fresh_handle(b2, case):
    _handles.pop((case.geom, case.B), None)
    return handle(b2, case)


def arena(torch, words, fill):
    """``words`` 32-bit words of ``fill`` followed by PAD guard words."""
    whole = torch.full((words + PAD,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    whole[:words] = int(np.uint32(fill).view(np.int32))
    return whole


def launch(b2, torch, amb, case, which, d_map, d_met, cap):
    """One detector call into guarded arenas -> (counts [B], records [B, cap])."""
    from blah2_amd import _lib
    B = case.B
    hits = arena(torch, B * cap * 4, GUARD)
    cnt = arena(torch, B, 0xDEADBEEF)  # the call zeroes the counts itself
    st = torch.cuda.current_stream().cuda_stream
    if which == "1d":
        det = b2.CfarDetector1D(case.pfa, case.window[0], case.window[1], case.min_delay, case.min_doppler)
    else:
        amb.set_cfar2d_kernel(which)
        amb.set_cfar2d_seg_rows(case.seg_rows)
        amb.set_cfar2d_grid(case.grid)
        det = b2.CfarDetector2D(case.pfa, *case.window, case.min_delay, case.min_doppler)
    try:
        det.process_dev(amb, B, hits.data_ptr(), cap, cnt.data_ptr(), d_map.data_ptr(), d_met.data_ptr(), st)
        torch.cuda.synchronize()
    finally:
        if which != "1d":
            amb.set_cfar2d_seg_rows(0)
            amb.set_cfar2d_grid(0)
            amb.set_cfar2d_kernel("auto")
    if which != "1d":  # the kernel that ran, and its plan
        seg, grid = amb.info(_lib.INFO_CFAR2D_SEG_ROWS), amb.info(_lib.INFO_CFAR2D_GRID)
        nD = amb.get_n_doppler_bins()
        ran = "stream" if seg else ("tile" if grid else "sat")
        if which != "auto":
            assert ran == which, (case.name, which, ran)
        else:
            w = case.window
            assert ran == ("stream" if tuple(w) in X.STREAM_SHAPES else "tile" if "tile" in X.kernels_for(w) else "sat")
        if ran == "stream" and case.seg_rows:
            assert seg == min(case.seg_rows, nD), (case.name, seg)
        if ran == "stream":
            assert 1 <= seg <= nD
        if ran == "tile":
            assert grid % 8 == 0 and (grid == 8 if case.grid == 8 else grid <= max(8, (amb.info(_lib.INFO_NUM_CU) + 7) & ~7))
    hw, cw = hits.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)
    assert (hw[-PAD:] == GUARD).all(), (case.name, which, "words behind the hit arena were written")
    assert (cw[-PAD:] == GUARD).all(), (case.name, which, "words behind the counts were written")
    return cw[:B].copy(), hw[:B * cap * 4].reshape(B, cap, 4)


def check(case, which, exp, maps, metrics, counts, recs, cap):
    """The comparison rule of the module docstring for one launch."""
    nD, nC = maps.shape[1:]
    sat = which == "sat" or (which == "auto" and "tile" not in X.kernels_for(case.w4) and not case.one_d)
    for c in range(case.B):
        ref = exp.hits[c]
        tag = (case.name, which, f"cpi {c}")
        stored = min(int(counts[c]), cap)
        raw = recs[c]
        assert (raw[stored:] == GUARD).all(), (*tag, "a slot beyond the count was written")
        r = np.ascontiguousarray(raw[:stored]).view(b2_hit_dtype()).reshape(-1)
        cells = list(zip(r["row"].tolist(), r["col"].tolist()))
        assert all(0 <= i < nD and 0 <= j < nC for i, j in cells), (*tag, "record outside the map")
        assert len(set(cells)) == len(cells), (*tag, "a cell was reported twice")
        got = set(cells)
        if sat and case.kind == "nonfinite":
            assert got <= set(ref), (*tag, "hits the oracle lacks", sorted(got - set(ref))[:8])
            print(f"{case.name} {which} cpi {c}: summed-area kernels lose {len(ref) - len(got)} of {len(ref)} detections")
        elif sat:
            assert int(counts[c]) <= cap
            inb = exp.sat_band[c]
            bad = [k for k in got ^ set(ref) if not inb[k]]
            assert not bad, (*tag, "outside the band", bad[:8], [exp.margin[c][k] for k in bad[:8]])
            worst["sat_hits"] += len(ref)
            worst["sat_in_band"] += sum(1 for k in ref if inb[k])
        else:
            assert int(counts[c]) == len(ref), (*tag, "count", int(counts[c]), len(ref))
            if stored == len(ref):
                assert got == set(ref), (*tag, "missing", sorted(set(ref) - got)[:8], "extra", sorted(got - set(ref))[:8])
            else:
                assert stored == cap and got <= set(ref), (*tag, "stored hits the oracle lacks", sorted(got - set(ref))[:8])
        # snr of every stored record, from the same cell in NumPy with this CPI's own noisePower
        z = maps[c].astype(np.complex128)
        for (i, j), s in zip(cells, r["snr"].tolist()):
            with np.errstate(divide="ignore"):
                want = 10.0 * np.log10(np.abs(z[i, j])) - metrics[c, 0]
            if np.isfinite(want):
                worst["snr"] = max(worst["snr"], abs(s - want))
                assert abs(s - want) <= SNR_TOL, (*tag, (i, j), s, want)
            else:
                assert s == want, (*tag, (i, j), s, want)


def b2_hit_dtype():
    from blah2_amd.process import HIT_DTYPE
    return HIT_DTYPE


def run_case(b2, torch, case, kernels=None, exp=None):
    maps, metrics = X.make_maps(case)
    exp = exp or X.expected(case, maps, metrics)
    amb = handle(b2, case)
    d_map = torch.from_numpy(maps).cuda()
    d_met = torch.from_numpy(metrics).cuda()
    cap = maps.shape[1] * maps.shape[2]
    for which in kernels or case.kernels():
        counts, recs = launch(b2, torch, amb, case, which, d_map, d_met, cap)
        check(case, which, exp, maps, metrics, counts, recs, cap)
    return exp


@pytest.mark.parametrize("group", sorted(g for g in GROUPS if g.startswith("shape-")))
def test_shapes(b2, torch, group):
    """One window on the map shapes at the kernels' own boundaries: nDelay of 1, 2, one output strip +- 1, 63 ... 257;
    nD of 1, 2, hR, 2 hR, 2 hR + 1, 7 ... 9 and one tile's output rows +- 1; windows larger than the whole map."""
    n = 0
    for case in GROUPS[group]:
        n += sum(len(h) for h in run_case(b2, torch, case).hits)
    assert n > 0


def test_segment_seams(b2, torch):
    """Forced rows per segment of the stream kernel (1, 2, hR, U - 1, U, U + 1, 8, 33, nD - 1, nD), one map and a batch of
    three distinct ones with distinct noisePower; the launch reports the value it used."""
    for case in GROUPS["seg"]:
        assert len(run_case(b2, torch, case).hits[0]) > 0


def test_persistent_tile_walk(b2, torch):
    """Eight workgroups walk 44 (88) tiles, two and three loads per row: the steady state of the persistent loop."""
    for case in GROUPS["grid"]:
        assert len(run_case(b2, torch, case).hits[0]) > 0


def test_dead_rows(b2, torch):
    """|doppler| < minDoppler on one-sided axes of either sign, odd and even nD: no dead row, a threshold equal to an
    axis value, between two values, an interval that touches the first / last row, and the whole map."""
    for case in GROUPS["dead"]:
        exp = run_case(b2, torch, case)
        assert (len(exp.hits[0]) == 0) == case.name.endswith("above")


def test_min_delay(b2, torch):
    for case in GROUPS["mindelay"]:
        exp = run_case(b2, torch, case)
        d = X.dims_of(case.geom)
        assert (len(exp.hits[0]) == 0) == (case.min_delay > d.delay[-1])


@pytest.mark.parametrize("name", [c.name for c in GROUPS["overflow"]])
def test_overflow(b2, torch, name):
    """cap below the count: the count stays the true one, exactly cap records of the CPI's own set are stored, and
    nothing lands in the next CPI's slots or behind the arena."""
    case = next(c for c in GROUPS["overflow"] if c.name == name)
    maps, metrics = X.make_maps(case)
    exp = X.expected(case, maps, metrics)
    n = [len(h) for h in exp.hits]
    assert min(n) > 2 and len({frozenset(h) for h in exp.hits}) == case.B
    amb = handle(b2, case)
    d_map, d_met = torch.from_numpy(maps).cuda(), torch.from_numpy(metrics).cuda()
    for which in [k for k in case.kernels() if k != "sat"]:
        for cap in sorted({1, min(n) - 1, max(n) - 1, max(n)}):
            counts, recs = launch(b2, torch, amb, case, which, d_map, d_met, cap)
            assert counts.tolist() == n, (name, which, cap)
            check(case, which, exp, maps, metrics, counts, recs, cap)
    if "sat" in case.kernels():  # same contract; its counts are its own (equal here: no hit of this input is in its band)
        for cap in sorted({1, min(n) - 1, max(n) - 1}):
            counts, recs = launch(b2, torch, amb, case, "sat", d_map, d_met, cap)
            assert counts.tolist() == n
            for c in range(case.B):
                r = np.ascontiguousarray(recs[c][:min(cap, n[c])]).view(b2_hit_dtype()).reshape(-1)
                cells = set(zip(r["row"].tolist(), r["col"].tolist()))
                assert len(cells) == min(cap, n[c]) and cells <= set(exp.hits[c])


def test_values(b2, torch):
    """Cells from 1e-20 to 1e18 (|z|^2 is formed in fp64 everywhere), an all-zero map, isolated zero cells, and a NaN and
    a +Inf cell."""
    for case in GROUPS["values"]:
        exp = run_case(b2, torch, case)
        assert (len(exp.hits[0]) == 0) == (case.kind == "zero")


def test_table_cache(b2, torch):
    """Twelve further pfa values through one handle evict the first table of the cache of eight; the first pfa then gives
    what a fresh handle gives.  A table built by *_prepare survives the same traffic."""
    from dataclasses import replace
    for case in GROUPS["cache"]:
        maps, metrics = X.make_maps(case)
        d_map, d_met = torch.from_numpy(maps).cuda(), torch.from_numpy(metrics).cuda()
        cap = maps.shape[1] * maps.shape[2]

        def lists(amb, pfa, which):
            c = replace(case, pfa=pfa)
            counts, recs = launch(b2, torch, amb, c, which, d_map, d_met, cap)
            r = np.ascontiguousarray(recs[0][:counts[0]]).view(b2_hit_dtype()).reshape(-1)
            return sorted(zip(r["row"].tolist(), r["col"].tolist(), r["snr"].tolist()))

        for which in case.kernels():
            amb = fresh_handle(b2, case)
            first = lists(amb, X.PFAS[0], which)
            assert len(first) > 0
            fresh = {p: lists(fresh_handle(b2, case), p, which) for p in X.PFAS[1:4]}
            for prepared in (False, True):
                amb = fresh_handle(b2, case)
                if prepared:
                    from blah2_amd._lib import check
                    if which == "1d":
                        check(amb._L.blah2hip_cfar1d_prepare(amb._h, X.PFAS[0], case.window[1]))
                    else:
                        amb.set_cfar2d_kernel(which)
                        check(amb._L.blah2hip_cfar2d_prepare(amb._h, X.PFAS[0], *case.window))
                else:
                    assert lists(amb, X.PFAS[0], which) == first
                sizes = set()
                for p in X.PFAS[1:]:
                    got = lists(amb, p, which)
                    sizes.add(len(got))
                    if p in fresh:
                        assert got == fresh[p], (case.name, which, p)
                assert len(sizes) > 3  # the thresholds did change with pfa
                assert lists(amb, X.PFAS[0], which) == first, (case.name, which, prepared)
                assert lists(amb, X.PFAS[5], which) == lists(fresh_handle(b2, case), X.PFAS[5], which)
        run_case(b2, torch, case)  # and pfa[0] against the oracle


def test_one_d(b2, torch):
    """The k > 0 quirk at columns 0 and 1, windows wider than the row, a batch, and rows either side of the longest one
    cfar1d_dev stages in LDS."""
    for case in GROUPS["1d"]:
        exp = run_case(b2, torch, case)
        if X.dims_of(case.geom).n_delay_bins > 2:
            assert len(exp.hits[0]) > 0, case.name
    _handles.clear()
