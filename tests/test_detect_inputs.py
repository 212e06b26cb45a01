"""CPU suite for the device detection finish (blah2hip_detect_dev): the ABI is there, and the inputs the GPU module runs
(tests/detect_crafted.py, the golden fixtures) satisfy the condition under which it may demand identical sets.

The kernel evaluates 10 log10(hypot(re, im)) with the device's fp64 log10 / hypot, the host functions with libm's: a
cell value may differ by an ulp or two, 3e-14 dB at 100 dB.  That can only change a result where a peak test
(s1 < s0, s1 < s2) is that close to a tie, or move an offset (s0 - s2) / (2 (s0 - 2 s1 + s2)) by eps / curvature.  So:
no candidate's test within 1e-9 dB of a tie, every kept candidate curved by 1e-3 dB or more (3e-14 / 1e-3 = 3e-11 of a
bin, far below the 1e-9 the GPU module asserts).  Cells holding ONE bit pattern are exempt from the tie rule: whatever
the implementation, it maps equal inputs to equal values, so a comparison between them cannot flip; and three such
cells give 0/0 on both sides (the flat triple the cases plant on purpose).
"""
import ctypes as C

import numpy as np
import pytest

import detect_crafted as D
from conftest import golden_names, load_golden

ALL = D.cases() + [D.batch_case(D.TILE), D.batch_case(4 * D.TILE)]


def test_library_exports_detect_dev(built_lib):
    fn = built_lib.blah2hip_detect_dev
    assert fn.restype is C.c_int and len(fn.argtypes) == 17


def test_det_record_is_32_bytes(built_lib):
    from blah2_amd import _lib
    assert C.sizeof(_lib.Det) == 32
    assert [f[0] for f in _lib.Det._fields_] == ["row", "col", "delay", "doppler", "snr"]
    import blah2_amd
    assert blah2_amd.DET_DTYPE.itemsize == 32
    assert [blah2_amd.DET_DTYPE.fields[k][1] for k in ("row", "col", "delay", "doppler", "snr")] == [0, 4, 8, 16, 24]


def test_package_exposes_the_new_names(built_lib):
    import blah2_amd
    from blah2_amd import _lib
    for name in ("DetectionFinisher", "dets_to_detection", "DET_DTYPE"):
        assert hasattr(blah2_amd, name) and name in blah2_amd.__all__
    assert (_lib.INFO_DETECT_GRID, _lib.INFO_DETECT_TILED) == (14, 15)
    f = blah2_amd.DetectionFinisher(6, 6, 1.0)
    assert (f.doCentroid, f.doDelay, f.doDoppler) == (True, True, True)
    with pytest.raises(ValueError):
        blah2_amd.DetectionFinisher(70000, 6, 1.0)


def test_dets_to_detection_sorts_into_emission_order(built_lib):
    import blah2_amd
    recs = np.zeros(4, dtype=blah2_amd.DET_DTYPE)
    recs["row"], recs["col"] = [3, 1, 3, 0], [2, 9, 1, 0]
    recs["delay"], recs["doppler"], recs["snr"] = [1.5, 2.5, 3.5, 9.0], [10.0, 20.0, 30.0, 9.0], [5.0, 6.0, 7.0, 9.0]
    d = blah2_amd.dets_to_detection(recs, 3, 4)  # the fourth record is not part of the list
    assert d.get_delay().tolist() == [2.5, 3.5, 1.5] and d.get_doppler().tolist() == [20.0, 30.0, 10.0]
    assert d.get_snr().tolist() == [6.0, 7.0, 5.0]
    assert blah2_amd.dets_to_detection(recs, 0, 4).get_nDetections() == 0
    with pytest.raises(blah2_amd.Blah2HipError):
        blah2_amd.dets_to_detection(recs, 5, 4)


def test_gpu_chain_refuses_an_unknown_detect_mode():
    from blah2_amd import replay as R
    with pytest.raises(ValueError):
        R.GpuChain({}, detect="elsewhere")


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_crafted_inputs_are_decidable(built_lib, case):
    maps, metrics, hits, words = D.make(case)
    d = D.dims(case)
    assert maps.shape == (case.B, d.n_doppler_bins, d.n_delay_bins)
    assert len(set(metrics[:, 0].tolist())) == case.B  # distinct noisePower
    slips = kept = 0
    for b, k in enumerate(case.counts):
        assert words[b] == k + (case.over if k == case.cap else 0)
        h = hits[b, :k]
        assert len(set(zip(h["row"].tolist(), h["col"].tolist()))) == k
        if k == 0:
            continue
        # every hit as a candidate (the list without Centroid is one of the GPU module's runs), in both directions
        tie, curv, _ = D.margins(maps[b], metrics[b, 0], h["row"], h["col"])
        assert tie >= D.DECISION, (case.name, b, tie)
        assert curv >= D.CURVATURE, (case.name, b, curv)
        rows, cols, _ = D.candidates(case, maps, metrics, hits, b)
        assert 0 < rows.size <= k
        slips += D.margins(maps[b], metrics[b, 0], rows, cols)[2]
        if b < 3:  # the whole host chain (one call per candidate: the first CPIs are enough here)
            exp = D.expected(case, maps, metrics, hits, b, True, True, True)
            assert len(exp) <= rows.size
            kept += len(exp)
    if case.features and max(case.counts) >= 140:
        assert slips >= 1, "no detection shows the :80 slip"
        assert kept >= 1
        flat = [v for v in D.expected(case, maps, metrics, hits, 0, True, True, False).values() if np.isnan(v[0])]
        assert flat, "no flat triple reached the output"


def test_crafted_cases_cover_what_they_claim(built_lib):
    names = {c.name: c for c in ALL}
    assert {c.counts[0] for c in ALL if c.B == 1} >= {0, 1, 255, 256, 257, D.TILE - 1, D.TILE, D.TILE + 1, 5000}
    assert any(c.cap > D.TILE for c in ALL) and any(c.cap <= D.TILE for c in ALL)
    assert any(c.over and c.cap <= D.TILE for c in ALL) and any(c.over and c.cap > D.TILE for c in ALL)
    assert any(c.cap_out for c in ALL)
    assert min(D.dims(names["features"]).delay) < 0 and min(D.dims(names["features-step"]).doppler) > -7
    assert max(D.dims(names["features-mirror"]).doppler) < 7
    b = names[f"batch-{D.TILE}"]
    assert b.B >= 64 and 0 in b.counts
    # the box edge: with 1 / cpi as the resolution, a hit nDoppler rows away is inside, on or outside the box by one
    # rounding of doppler[i] + (nDoppler * resolution) -- all three happen on these axes
    for name in ("features-step", "features-mirror"):
        c = names[name]
        ax, nf = D.dims(c).doppler, c.n_centroid[1]
        box = nf * D.resolution(c)
        inside = sum(bool(ax[i + nf] < ax[i] + box) for i in range(len(ax) - nf))
        on = sum(bool(ax[i + nf] == ax[i] + box) for i in range(len(ax) - nf))
        print(f"{name}: rows whose nDoppler-th neighbour lies inside the box {inside}, on its edge {on}, of {len(ax) - nf}")
        assert inside > 0 and on > 0 and inside + on < len(ax) - nf


@pytest.mark.parametrize("name", golden_names())
def test_golden_interp_stage_is_decidable(built_lib, name):
    g = load_golden(name)
    m = g["map"].astype(np.complex64)
    delay0 = int(g["delay"][0])
    row = {f: i for i, f in enumerate(g["doppler"].tolist())}
    rows = np.array([row[f] for f in g["centroid"][1].tolist()], dtype=np.int64)
    cols = (g["centroid"][0] - delay0).astype(np.int64)
    if rows.size == 0:
        return
    tie, curv, _ = D.margins(m, float(g["metrics"][0]), rows, cols)
    assert tie >= D.DECISION, (name, tie)
    assert curv >= D.CURVATURE, (name, curv)
