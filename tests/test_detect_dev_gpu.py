"""GPU: Centroid and Interpolate on the device (blah2hip_detect_dev, detect_finish_kernel) against the host functions
blah2hip_centroid / blah2hip_interpolate on the same map and hit list, and against the compiled reference's lists in
tests/golden.

Comparison rule
  * golden fixtures: iq -> Ambiguity -> cfar1d on the device -> detect_dev.  The list after Centroid equals the
    reference's exactly in delay and Doppler (its snr is the detector's, off the device's fp32 map: 1e-3 dB like
    test_cfar_gpu.py); the final list agrees to the tolerances of test_centroid_interpolate.py (1e-4 bins, 1e-3 Hz,
    1e-4 dB: an fp32 map against the reference's fp64 one).
  * crafted inputs (tests/detect_crafted.py): the set of (row, col) EQUALS the host's, nothing excluded;
    delay, doppler / step and snr within 1e-9 (NaN where the host has NaN).  test_detect_inputs.py asserts on the CPU
    that no decision of these inputs is closer than 1e-9 dB to a tie and that every kept candidate is curved by 1e-3 dB,
    so an ulp of the device's log10 / hypot cannot show.
  * count_out (pre-filled with garbage) is the true number also when it exceeds cap_out; then exactly cap_out records
    are stored, all members of the host's set; slots beyond, the words behind the arenas and the hit counts keep their
    pattern.
"""
import numpy as np
import pytest

import detect_crafted as D
from conftest import golden_names, load_golden

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)
PAD = 64
TOL = 1e-9
CASES = {c.name: c for c in D.cases()}
worst = {"delay": 0.0, "doppler": 0.0, "snr": 0.0}


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
    print(f"\ndetect_dev against the host functions: largest difference delay {worst['delay']:.3e} bins, "
          f"doppler {worst['doppler']:.3e} steps, snr {worst['snr']:.3e} dB")


_handles = {}


def handle(b2, case):
    key = (case.geom, case.B)
    if key not in _handles:
        g, d = case.geom, D.dims(case)
        amb = b2.Ambiguity(g[0], g[1], g[2], g[3], g[4], g[5], False, max_batch=case.B, n_doppler_bins=g[6])
        assert np.array_equal(amb.delay, d.delay) and np.array_equal(amb.doppler, d.doppler)
        _handles[key] = amb
    return _handles[key]


def arena(torch, words, fill):
    whole = torch.full((words + PAD,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    whole[:words] = int(np.uint32(fill).view(np.int32))
    return whole


class Inputs:
    def __init__(self, b2, torch, case):
        self.case, self.amb = case, handle(b2, case)
        self.maps, self.metrics, self.hits, self.words = D.make(case)
        self.d_map, self.d_met = torch.from_numpy(self.maps).cuda(), torch.from_numpy(self.metrics).cuda()
        self.d_hits = torch.from_numpy(self.hits.view(np.float64).reshape(case.B, case.cap, 2)).cuda()
        self.d_cnt = torch.from_numpy(self.words.view(np.int32)).cuda()


def launch(b2, torch, inp, flags, do_centroid=True, repeat=1):
    """One call into guarded arenas -> (count_out [B], records [B, cap_out]); repeat > 1: that many calls enqueued back to
    back, each into arenas of its own, before the one synchronisation -> a list of such pairs."""
    from blah2_amd import _lib
    case, amb = inp.case, inp.amb
    cap_out = case.cap_out or case.cap
    fin = b2.DetectionFinisher(case.n_centroid[0], case.n_centroid[1], D.resolution(case), bool(flags[0]), bool(flags[1]),
                               do_centroid)
    sets = [(arena(torch, case.B * cap_out * 8, GUARD), arena(torch, case.B, 0xDEADBEEF)) for _ in range(repeat)]
    torch.cuda.synchronize()
    for out, cnt in sets:
        fin.process_dev(amb, case.B, inp.d_hits.data_ptr(), case.cap, inp.d_cnt.data_ptr(), out.data_ptr(), cap_out, cnt.data_ptr(),
                        inp.d_map.data_ptr(), inp.d_met.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    tiled, grid = amb.info(_lib.INFO_DETECT_TILED), amb.info(_lib.INFO_DETECT_GRID)
    assert tiled == (1 if case.cap > D.TILE else 0), (case.name, tiled)
    assert (grid > 1 and grid <= -(-case.cap // 256)) if tiled else grid == 1, (case.name, grid)
    assert np.array_equal(inp.d_cnt.cpu().numpy().view(np.uint32), inp.words), (case.name, "the hit counts were written")
    res = []
    for out, cnt in sets:
        ow, cw = out.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)
        assert (ow[-PAD:] == GUARD).all() and (cw[-PAD:] == GUARD).all(), (case.name, "words behind an arena were written")
        res.append((cw[:case.B].copy(), ow[:case.B * cap_out * 8].reshape(case.B, cap_out, 8)))
    return res[0] if repeat == 1 else res


def compare(b2, inp, flags, do_centroid, counts, recs, cpis=None):
    case = inp.case
    step = float(inp.amb.doppler[1] - inp.amb.doppler[0])
    cap_out = recs.shape[1]
    for b in (range(case.B) if cpis is None else cpis):
        exp = D.expected(case, inp.maps, inp.metrics, inp.hits, b, do_centroid, *flags)
        tag = (case.name, flags, do_centroid, f"cpi {b}")
        assert int(counts[b]) == len(exp), (*tag, "count", int(counts[b]), len(exp))
        stored = min(len(exp), cap_out)
        assert (recs[b, stored:] == GUARD).all(), (*tag, "a slot beyond the count was written")
        r = np.ascontiguousarray(recs[b, :stored]).view(b2.DET_DTYPE).reshape(-1)
        cells = list(zip(r["row"].tolist(), r["col"].tolist()))
        assert len(set(cells)) == len(cells), (*tag, "a detection was reported twice")
        if stored == len(exp):
            assert set(cells) == set(exp), (*tag, "missing", sorted(set(exp) - set(cells))[:8], "extra", sorted(set(cells) - set(exp))[:8])
        else:
            assert set(cells) <= set(exp), (*tag, "stored detections the host lacks", sorted(set(cells) - set(exp))[:8])
        for cell, dl, dp, sn in zip(cells, r["delay"].tolist(), r["doppler"].tolist(), r["snr"].tolist()):
            for name, got, want, scale in (("delay", dl, exp[cell][0], 1.0), ("doppler", dp, exp[cell][1], step), ("snr", sn, exp[cell][2], 1.0)):
                if np.isnan(want) or np.isinf(want):
                    assert np.isnan(got) if np.isnan(want) else got == want, (*tag, cell, name, got, want)
                else:
                    err = abs(got - want) / scale
                    worst[name] = max(worst[name], err)
                    assert err <= TOL, (*tag, cell, name, got, want)


# ---- 1. golden fixtures ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names())
def test_golden_chain_on_the_device(b2, torch, name):
    g = load_golden(name)
    fs, n, dmin, dmax, fmin, fmax, rh = (int(v) for v in g["params"])
    pfa, ng, nt, md, mdop = g["det_params"][:5]
    nc, res = int(g["det_params"][5]), float(g["det_params"][6])
    amb = b2.Ambiguity(dmin, dmax, fmin, fmax, fs, n, bool(rh))
    amb.process(g["x"], g["y"])  # the map and its metrics stay in the engine's buffers
    cap = amb.get_n_doppler_bins() * amb.get_n_delay_bins()
    st = torch.cuda.current_stream().cuda_stream
    d_hits = torch.zeros((cap, 2), dtype=torch.float64, device="cuda")
    d_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    b2.CfarDetector1D(pfa, int(ng), int(nt), int(md), mdop).process_dev(amb, 1, d_hits.data_ptr(), cap, d_cnt.data_ptr(), stream=st)
    out = {}
    for flags in ((False, False), (True, True)):
        d_out = torch.zeros((cap, 4), dtype=torch.float64, device="cuda")
        d_n = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        b2.DetectionFinisher(nc, nc, res, *flags).process_dev(amb, 1, d_hits.data_ptr(), cap, d_cnt.data_ptr(), d_out.data_ptr(), cap,
                                                              d_n.data_ptr(), stream=st)
        torch.cuda.synchronize()
        k = int(d_n.cpu()[0])
        out[flags] = b2.dets_to_detection(d_out.cpu().numpy().view(b2.DET_DTYPE).reshape(-1), k, cap)
    assert int(d_cnt.cpu()[0]) == g["cfar"].shape[1]
    c, i = out[(False, False)], out[(True, True)]
    assert np.array_equal(c.get_delay(), g["centroid"][0]) and np.array_equal(c.get_doppler(), g["centroid"][1])
    assert np.allclose(c.get_snr(), g["centroid"][2], rtol=0, atol=1e-3)  # the hit's snr, off an fp32 map (test_cfar_gpu.py)
    assert i.get_nDetections() == g["interp"].shape[1]
    assert np.allclose(i.get_delay(), g["interp"][0], rtol=0, atol=1e-4)
    assert np.allclose(i.get_doppler(), g["interp"][1], rtol=0, atol=1e-3)
    assert np.allclose(i.get_snr(), g["interp"][2], rtol=0, atol=1e-4)


# ---- 2. crafted maps and lists ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_crafted(b2, torch, name):
    """Every (do_delay, do_doppler) combination behind Centroid, and the list without Centroid through both."""
    case = CASES[name]
    inp = Inputs(b2, torch, case)
    total = 0
    for do_centroid, flags in [(True, f) for f in D.FLAGS] + [(False, (1, 1))]:
        counts, recs = launch(b2, torch, inp, flags, do_centroid)
        compare(b2, inp, flags, do_centroid, counts, recs)
        total += int(counts.sum())
    assert (total > 0) == (max(case.counts) > 0)
    if case.cap_out:
        assert max(int(c) for c in counts) > case.cap_out  # the truncation did happen
    if case.over:
        assert int(inp.words.max()) > case.cap


def test_invalid_arguments(b2, torch):
    from blah2_amd import _lib
    inp = Inputs(b2, torch, CASES["count-1"])
    out, cnt = arena(torch, 1024 * 8, GUARD), arena(torch, 1, 0)
    L, h = inp.amb._L, inp.amb._h
    good = [h, inp.d_map.data_ptr(), inp.d_met.data_ptr(), 1, inp.d_hits.data_ptr(), 1024, inp.d_cnt.data_ptr(), 6, 6, 1.0, 1, 1, 1,
            out.data_ptr(), 1024, cnt.data_ptr(), None]
    assert L.blah2hip_detect_dev(*good) == _lib.OK
    for k, v in ((0, None), (4, None), (6, None), (13, None), (15, None), (5, 0), (3, 0), (3, 2)):
        bad = list(good)
        bad[k] = v
        assert L.blah2hip_detect_dev(*bad) == _lib.ERR_INVALID, k
    torch.cuda.synchronize()


# ---- 3. a batch, twice in a row: the counters reset themselves ----------------------------------------------------
@pytest.mark.parametrize("cap", [D.TILE, 4 * D.TILE])
def test_batch_twice_on_one_stream(b2, torch, cap):
    case = D.batch_case(cap)
    assert case.B >= 64
    inp = Inputs(b2, torch, case)
    first, second = launch(b2, torch, inp, (1, 1), repeat=2)  # nothing between the two but the stream's order
    assert np.array_equal(first[0], second[0])
    for b in range(case.B):
        k = int(first[0][b])
        a = np.sort(np.ascontiguousarray(first[1][b, :k]).view(b2.DET_DTYPE).reshape(-1), order=["row", "col"])
        c = np.sort(np.ascontiguousarray(second[1][b, :k]).view(b2.DET_DTYPE).reshape(-1), order=["row", "col"])
        assert a.tobytes() == c.tobytes(), (cap, b)
    compare(b2, inp, (1, 1), True, *second)
    assert sum(1 for k in first[0] if k == 0) >= 8 and int(first[0].sum()) > 0
    third = launch(b2, torch, inp, (0, 0))  # and another flag set behind them
    compare(b2, inp, (0, 0), True, *third, cpis=range(0, case.B, 7))


# ---- 4. a 2-D detector's list of an engine-made map ---------------------------------------------------------------
def test_cfar2d_hits_of_an_engine_map(b2, torch):
    g = load_golden("medium")
    fs, n, dmin, dmax, fmin, fmax, rh = (int(v) for v in g["params"])
    amb = b2.Ambiguity(dmin, dmax, fmin, fmax, fs, n, bool(rh))
    m = amb.process(g["x"], g["y"])
    det2 = b2.CfarDetector2D(1e-3, 1, 3, 1, 2, -10, 0.0)
    ref = b2.Interpolate(True, True).process(b2.Centroid(6, 6, 1 / (n / fs)).process(det2.process(m)), m)
    cap = m.data.size
    st = torch.cuda.current_stream().cuda_stream
    d_hits = torch.zeros((cap, 2), dtype=torch.float64, device="cuda")
    d_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_out = torch.zeros((cap, 4), dtype=torch.float64, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
    det2.process_dev(amb, 1, d_hits.data_ptr(), cap, d_cnt.data_ptr(), stream=st)
    b2.DetectionFinisher(6, 6, 1 / (n / fs)).process_dev(amb, 1, d_hits.data_ptr(), cap, d_cnt.data_ptr(), d_out.data_ptr(), cap,
                                                         d_n.data_ptr(), stream=st)
    torch.cuda.synchronize()
    got = b2.dets_to_detection(d_out.cpu().numpy().view(b2.DET_DTYPE).reshape(-1), int(d_n.cpu()[0]), cap)
    assert int(d_cnt.cpu()[0]) > ref.get_nDetections() > 0
    assert got.get_nDetections() == ref.get_nDetections()
    step = float(amb.doppler[1] - amb.doppler[0])
    assert np.allclose(got.get_delay(), ref.get_delay(), rtol=0, atol=TOL)
    assert np.allclose(got.get_doppler() / step, ref.get_doppler() / step, rtol=0, atol=TOL)
    assert np.allclose(got.get_snr(), ref.get_snr(), rtol=0, atol=TOL)


# ---- 5. the replay chain ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clutter", [False, True])
def test_gpu_chain_device_against_host(b2, torch, tmp_path, clutter):
    from blah2_amd import replay as R
    g = load_golden("medium")
    fs, n, dmin, dmax, fmin, fmax, rh = (int(v) for v in g["params"])
    pfa, ng, nt, md, mdop = g["det_params"][:5]
    rng = np.random.default_rng(11)
    cpis = [g["iq"], -g["iq"]] + [np.roll(g["iq"], int(k), axis=0) for k in rng.integers(1, 50, 5)]
    path = str(tmp_path / "cap.rspduo")
    np.concatenate(cpis).tofile(path)
    cfg = {"fs": fs, "n_samples": n,
           "ambiguity": {"delayMin": dmin, "delayMax": dmax, "dopplerMin": fmin, "dopplerMax": fmax},
           "detection": {"enable": True, "pfa": pfa, "nGuard": int(ng), "nTrain": int(nt), "minDelay": int(md), "minDoppler": mdop,
                         "nCentroid": 6},
           "clutter": {"enable": clutter, "delayMin": int(g["clutter_params"][0]), "delayMax": int(g["clutter_params"][1])}}
    step = fs / n
    out = {}
    for detect, want_map in (("host", False), ("device", False), ("device", True), (None, False)):
        cap = R.RspduoFile(path, n)
        chain = R.GpuChain(cfg, 0, batch=4, want_map=want_map, detect=detect)
        assert chain.detect == (detect or "device")
        if chain.detect == "device":
            assert all((s["h_map"] is None) == (not want_map) for s in chain.slots)
            assert all(s["h_hits"] is None for s in chain.slots) and chain.need_map == want_map
        else:
            assert all(s["h_map"] is not None for s in chain.slots)
        out[(detect, want_map)] = R.replay(cap, chain, batch=4)
        chain.close()
        cap.close()
    ref = out[("host", False)]
    assert [r["cpi"] for r in ref] == list(range(7)) and sum(len(r["delay"]) for r in ref) > 0
    for key, res in out.items():
        assert len(res) == len(ref)
        for a, b in zip(res, ref):
            assert a["cpi"] == b["cpi"] and abs(a["noisePower"] - b["noisePower"]) < TOL
            assert len(a["delay"]) == len(b["delay"]), (key, a["cpi"])
            assert np.allclose(a["delay"], b["delay"], rtol=0, atol=TOL)
            assert np.allclose(np.array(a["doppler"]) / step, np.array(b["doppler"]) / step, rtol=0, atol=TOL)
            assert np.allclose(a["snr"], b["snr"], rtol=0, atol=TOL)
            assert ("map" in a) == key[1]
    if not clutter:  # the fixture's own CPI: the compiled reference's final list
        assert len(ref[0]["delay"]) == g["interp"].shape[1]
    _handles.clear()
