"""GPU: several carriers through the replay chain (``cfg["ddc"]["offset"]`` a list, ``replay.py --ddc OFF0,OFF1:DECIM``) on
the synthetic wideband capture of carrier_scenes.py: three CPIs of one second at 65 536 Hz as int16 words, two programmes at
-16 384 and +16 384 Hz, capture.fc = 655 360 Hz (ratio 1.0513), ONE target in both carriers at delay 6 -- 40 Hz in carrier 0,
42.05 Hz in carrier 1, two rows apart -- and a strong echo of carrier 0 alone at 62 Hz, a row carrier 1 does not cover.

  * the fused chain's maps and metrics are the Python mirror's (Channelizer -> Ambiguity over 2 B virtual CPIs ->
    fuse_carriers_dev) bit for bit, and pass the cell-wise gate of oracle/gates.py against the fp64 restatement chain
    (blah2_amd.ddc -> the oracle's ambiguity stage -> blah2_amd.fuse_carriers);
  * the amplitude condition (below); detections outside the covered interval are absent; a one-entry list is the scalar
    configuration byte for byte; batches of 1 + 2 CPIs give the frames of one batch of 3.

The amplitude condition.  The target's amplitude, carrier_scenes.ECHO = 0.0087, was chosen on the CPU from the fp64
restatement chain and the CFAR restatement (carrier_scenes.margins: |z|^2 over the threshold of the cell-averaging detector
made for L looks, pfa 1e-5, 2 guard and 6 training cells a side).  In CPIs 0 and 2 the fused map's detector (2 looks) has the
target's cell at 1.09 and 1.05 of its threshold, while each single carrier's detector (1 look, same pfa) has its own cell
at 0.62 / 0.43 (CPI 0) and 0.96 / 0.36 (CPI 2): every margin is further from 1 than the project's detection-margin rule
asks (MARGIN_K x the measured map error, some 4e-6).  Both facts are asserted, on the CPU figures and on the device's lists.
In CPI 1 carrier 1's programme alone happens to carry the echo to 1.02 of the one-look threshold, so that CPI is asserted for
the fused chain only (1.35).  The strong echo at 62 Hz exceeds the fused map's threshold 4.6 to 5.5 times and the plain
carrier-0 chain reports it: that the fused frames do not hold it is the covered interval's doing.
"""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import carrier_scenes as S
from oracle import gates as G

DET = dict(pfa=1e-5, nGuard=2, nTrain=6, minDelay=0, minDoppler=5.0)
FULL = (0, 2)  # the CPIs on which neither carrier alone detects the target


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    """(path of the .rspduo capture, its int16 words [n, 4], the integers as complex128 [2, n])."""
    words, u = S.quantise(*S.stream())
    path = str(tmp_path_factory.mktemp("carriers") / "cap.rspduo")
    words.tofile(path)
    return path, words, u


@pytest.fixture(scope="module")
def restated(b2, capture):
    """The fp64 restatement chain, once: (dims, the carriers' maps [2, 3, nD, nC], the fused levels [3, nD, nC], the table)."""
    dims, maps = S.carrier_maps(capture[2])
    table = b2.carrier_table(np.asarray(dims.doppler), b2.carrier_ratios(S.FC, S.OFFSETS), "nearest")
    return dims, maps, b2.fuse_carriers(maps, table), table


def config(offset, **ddc):
    a = S.AMB_ARGS
    return {"fs": S.FS, "n_samples": S.N, "fc": S.FC,
            "ambiguity": {"delayMin": a[0], "delayMax": a[1], "dopplerMin": a[2], "dopplerMax": a[3]},
            "detection": dict(DET, enable=True), "clutter": {"enable": False},
            "ddc": dict({"offset": offset, "decimation": S.D, "taps": S.T}, **ddc)}


_runs = {}


def run(capture, offset, batches=((0, 3),), batch=3):
    """The frames of the capture under ``offset``, in batches: computed once per configuration, left unchanged."""
    from blah2_amd import replay as R
    key = (json.dumps(offset), tuple(batches), batch)
    if key not in _runs:
        cap = R.RspduoFile(capture[0], S.N)
        chain = R.GpuChain(config(offset), 0, batch=batch, want_map=True)
        try:
            _runs[key] = [r for part in chain.run_batches(cap, batches) for r in part]
        finally:
            chain.close()
            cap.close()
    return _runs[key]


def cells(r):
    return set(zip(r["delay"], r["doppler"]))


def same_frames(p, q):
    assert len(p) == len(q)
    for a, b in zip(p, q):
        assert a.keys() == b.keys() and np.array_equal(a["map"].view(np.uint32), b["map"].view(np.uint32))
        assert all(a[k] == b[k] for k in a if k != "map"), [k for k in a if k != "map" and a[k] != b[k]]


def test_the_fused_maps_are_the_mirrors_bits(b2, capture):
    import torch
    res = run(capture, list(S.OFFSETS))
    assert [r["cpi"] for r in res] == [0, 1, 2] and all(r["carriers"] == 2 for r in res)
    B, n, st = 3, S.N // S.D, torch.cuda.current_stream().cuda_stream
    ch = b2.Channelizer(S.FS, S.D, b2.ddc_design(S.D, S.T, 0.8, 8.0), list(S.OFFSETS), S.N, max_rows=B)
    amb = b2.Ambiguity(*S.AMB_ARGS, True, max_batch=2 * B)
    try:
        nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
        d_iq = torch.from_numpy(capture[1].reshape(B, S.N, 4)).cuda()
        planes = torch.zeros((2, 2 * B, n), dtype=torch.complex64, device="cuda")
        d_map = torch.zeros((2 * B, nD, nC), dtype=torch.complex64, device="cuda")
        d_met = torch.zeros((2 * B, 2), dtype=torch.float64, device="cuda")
        out = torch.zeros((B, nD, nC), dtype=torch.complex64, device="cuda")
        met = torch.zeros((B, 2), dtype=torch.float64, device="cuda")
        ch.reset(0, st)
        ch.process_dev(b2.FMT_I16, d_iq.data_ptr(), None, S.N, B, S.N, planes[0].data_ptr(), planes[1].data_ptr(), n, B * n, st)
        amb.process_dev(b2.FMT_C32, planes[0].data_ptr(), planes[1].data_ptr(), 2 * B, n, d_map.data_ptr(), d_met.data_ptr(), st)
        amb.set_carriers(b2.carrier_ratios(S.FC, S.OFFSETS), "nearest")
        amb.fuse_carriers_dev(d_map.data_ptr(), B, out.data_ptr(), met.data_ptr(), None, st)
        torch.cuda.synchronize()
        out, met = out.cpu().numpy(), met.cpu().numpy()
    finally:
        amb.close()
        ch.close()
    for c, r in enumerate(res):
        assert np.array_equal(r["map"].view(np.uint32), out[c].view(np.uint32)), c
        assert r["noisePower"] == met[c, 0] and r["maxPower"] == met[c, 1]


def test_the_fused_maps_pass_the_gates_against_the_restatement(b2, capture, restated):
    dims, _, fused, _ = restated
    for c, r in enumerate(run(capture, list(S.OFFSETS))):
        assert (r["map"].imag == 0).all()
        cell = G.map_cell_gate(r["map"], fused[c])
        print(f"[cpi {c}] {cell}")
        assert cell["ok"], cell
        assert abs(r["noisePower"] - float(np.mean(10.0 * np.log10(fused[c])))) <= 1e-3


def test_two_looks_find_what_one_look_misses(b2, capture, restated):
    dims, maps, fused, table = restated
    dop, d0 = np.asarray(dims.doppler), int(dims.delay[0])
    row = {c: int(np.argmin(np.abs(dop - S.ECHO_DOPPLER * ratio))) for c, ratio in enumerate((1.0, S.RATIO))}
    assert row[1] - row[0] == 2 and table["row"][1][row[0]] == row[1]  # two rows apart, and the table knows
    col = S.PEAK[0] - d0
    peaks = {k: (float(S.PEAK[0]), float(dop[row[k]])) for k in (0, 1)}  # (the bins are 16384 / 16383 Hz apart: 40.002 Hz)
    assert abs(peaks[0][1] - S.PEAK[1]) < 0.01
    both = run(capture, list(S.OFFSETS))
    single = {c: run(capture, S.OFFSETS[c]) for c in (0, 1)}
    for c in range(S.CAPTURE_CPIS):
        cell = G.map_cell_gate(both[c]["map"], fused[c])
        tol = G.MARGIN_K * G.margin_eps(cell)
        mf = S.margins(fused[c], DET["pfa"], DET["nGuard"], DET["nTrain"], 2)[row[0], col]
        ms = [S.margins(np.abs(maps[k, c]), DET["pfa"], DET["nGuard"], DET["nTrain"], 1)[row[k], col] for k in (0, 1)]
        print(f"[cpi {c}] margin fused {mf:.3f}, carriers alone {ms[0]:.3f} {ms[1]:.3f}, rule {tol:.1e}")
        assert mf > 1.0 + tol and peaks[0] in cells(both[c]), c
        if c in FULL:
            for k in (0, 1):
                assert ms[k] < 1.0 - tol and peaks[k] not in cells(single[k][c]), (c, k)


def test_detections_outside_the_covered_interval_are_absent(b2, capture, restated):
    dims, _, fused, table = restated
    dop, d0 = np.asarray(dims.doppler), int(dims.delay[0])
    full = np.nonzero(table["covered"] == 2)[0]
    lo, hi = float(dop[full[0]]), float(dop[full[-1]])
    assert abs(lo + 60.0) < 0.01 and abs(hi - 60.0) < 0.01  # rows -60 .. 60: 61 x 1.0513 lies beyond the axis' 64
    j = int(np.argmin(np.abs(dop - S.EDGE_PEAK[1])))
    edge = (float(S.EDGE_PEAK[0]), float(dop[j]))
    assert abs(edge[1] - S.EDGE_PEAK[1]) < 0.01
    for c, r in enumerate(run(capture, list(S.OFFSETS))):
        assert r["covered"] == [lo, hi] and all(lo <= f <= hi for f in r["doppler"])
        assert len(r["delay"]) == len(r["doppler"]) == len(r["snr"])
        assert S.margins(fused[c], DET["pfa"], DET["nGuard"], DET["nTrain"], 2)[j, S.EDGE_PEAK[0] - d0] > 2.0  # the detector had it
        assert edge in cells(run(capture, S.OFFSETS[0])[c])  # ... as carrier 0's own chain reports it
    assert "covered" not in run(capture, S.OFFSETS[0])[0]


def test_a_list_of_one_offset_is_the_scalar(b2, capture):
    same_frames(run(capture, [S.OFFSETS[1]]), run(capture, S.OFFSETS[1]))


def test_batches_of_one_and_two_give_the_frames_of_three(b2, capture):
    same_frames(run(capture, list(S.OFFSETS), batches=((0, 1), (1, 2)), batch=2), run(capture, list(S.OFFSETS)))


def test_refusals_that_need_the_handle_and_the_command_line(b2, capture, tmp_path, capsys):
    from blah2_amd import replay as R
    cfg = config(list(S.OFFSETS))
    cfg["fc"] = 20000.0  # (20000 + 16384) / (20000 - 16384): a ratio the table refuses
    with pytest.raises(ValueError, match="capture.ddc"):
        R.GpuChain(cfg, 0, batch=1)
    for bad in (dict(cfg, fc=None), config([1000.0, 1000.0]), config(list(S.OFFSETS), interp="cubic")):
        with pytest.raises(ValueError, match="capture.ddc"):
            R.GpuChain({k: v for k, v in bad.items() if v is not None}, 0, batch=1)
    yml = tmp_path / "config.yml"
    yml.write_text("capture:\n  fs: 65536\n  fc: 655360\nprocess:\n  data:\n    cpi: 1.0\n  ambiguity:\n"
                   "    delayMin: -4\n    delayMax: 20\n    dopplerMin: -64\n    dopplerMax: 64\n"
                   "  clutter:\n    enable: false\n  detection:\n    enable: true\n    pfa: 0.00001\n    nGuard: 2\n    nTrain: 6\n"
                   "    minDelay: 0\n    minDoppler: 5.0\n")
    strict = tmp_path / "centroid.yml"  # with nCentroid, so that --detect host asks for the host finisher
    strict.write_text(yml.read_text() + "    nCentroid: 3\n")
    for argv in (["--ddc", "-16384,x:4"], ["--ddc", "-16384,16384:4", "--ddc-interp", "cubic"], ["--ddc-interp", "linear"],
                 ["--ddc", "-16384,16384:4", "--migration"], ["--ddc", "-16384,16384:4", "--detect", "host"]):
        with pytest.raises(SystemExit):
            R.main([capture[0], "--config", str(strict)] + argv)
    capsys.readouterr()
    R.main([capture[0], "--config", str(yml), "--batch", "3", "--ddc", "-16384,16384:4:64"])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    want = run(capture, list(S.OFFSETS))
    assert [ln["cpi"] for ln in lines] == [0, 1, 2]
    for ln, w in zip(lines, want):
        assert ln["noisePower"] == w["noisePower"] and ln["delay"] == list(w["delay"]) and ln["doppler"] == list(w["doppler"])
        assert ln["covered"] == w["covered"] and ln["carriers"] == 2
