"""GPU: integration along tracks in the replay chain (``cfg["integrate"]["tracks"] = {"fc": HZ, "rate": QMAX | {max, step}}``,
``replay.py --integrate W[:H] --integrate-tracks [QMAX[:STEP]]``), on the capture of tests/test_migrate_replay_gpu.py.

  * no key, ``None`` and ``False``: the integrating chain's frames byte for byte, track_sum_kernel never launched
    (BLAH2HIP_INFO_TRACK_GRID stays 0), the detector at the configured pfa;
  * with the key the chain's maps and metrics are the bits of ``process_dev`` + ``MapIntegrator.set_tracks`` /
    ``process_tracks_dev`` called by hand on the same batches, and its detections those of ``CfarDetector1D(pfa / K,
    looks=W)`` and the finisher on them;
  * the ValueErrors name the key; the command line refuses its forms of them.
"""
import numpy as np
import pytest

from test_migrate_replay_gpu import DET, FC, SMALL, capture_cpis

pytestmark = pytest.mark.gpu

B, N, W = 2, 6, 3


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def config(tracks="absent"):
    amb = {"delayMin": SMALL[0], "delayMax": SMALL[1], "dopplerMin": SMALL[2], "dopplerMax": SMALL[3]}
    integ = {"window": W, "hop": 1}
    if tracks != "absent":
        integ["tracks"] = tracks
    return {"fs": SMALL[4], "n_samples": SMALL[5], "ambiguity": amb, "detection": dict(DET), "clutter": {"enable": False},
            "integrate": integ}


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tracks") / "cap.rspduo")
    iq = capture_cpis(SMALL[5], SMALL[4], N, 3)
    iq.tofile(path)
    return path, iq


def run(path, cfg):
    """-> (frames, what the chain holds and launched)."""
    from blah2_amd import _lib, replay as R
    chain = R.GpuChain(cfg, 0, batch=B, want_map=True)
    cap = R.RspduoFile(path, SMALL[5])
    try:
        res = R.replay(cap, chain, batch=B)
        return res, {"tracks": chain.nci_tracks, "n_rates": chain.nci.n_rates, "pfa": chain.cfar.pfa,
                     "grid": chain.amb.info(_lib.INFO_TRACK_GRID)}
    finally:
        chain.close()
        cap.close()


def same_frames(a, b):
    if len(a) != len(b):
        return False
    for p, q in zip(a, b):
        if p.keys() != q.keys() or ("map" in p and not np.array_equal(p["map"].view(np.uint32), q["map"].view(np.uint32))):
            return False
        if any(p[k] != q[k] for k in p if k != "map"):
            return False
    return True


_plain = {}


def plain_of(path):
    if "p" not in _plain:
        _plain["p"] = run(path, config())
    return _plain["p"]


def test_no_key_is_the_integrating_chain_without_the_feature(b2, capture):
    path, _ = capture
    plain, held = plain_of(path)
    assert held["tracks"] is False and held["n_rates"] == 0 and held["grid"] == 0 and held["pfa"] == DET["pfa"]
    assert [r["cpi"] for r in plain] == list(range(N)) and [bool(r.get("integrating")) for r in plain] == [True, True] + [False] * 4
    assert sum(len(r["delay"]) for r in plain if "delay" in r) > 0
    for off in (None, False):
        res, held = run(path, config(tracks=off))
        assert held["tracks"] is False and held["grid"] == 0 and held["pfa"] == DET["pfa"] and same_frames(res, plain), off


@pytest.mark.parametrize("rate", [None, 1, {"max": 1.0, "step": 0.5}], ids=["walk-only", "number", "dict"])
def test_chain_is_the_python_objects_called_by_hand(b2, torch, capture, rate):
    path, iq = capture
    plain, _ = plain_of(path)
    bank = None if rate is None else b2.rate_bank(1.0, 1.0 if rate == 1 else 0.5)
    K = 1 if bank is None else bank.size
    res, held = run(path, config({"fc": FC} if rate is None else {"fc": FC, "rate": rate}))
    n, fs = SMALL[5], SMALL[4]
    amb = b2.Ambiguity(*SMALL, True, max_batch=B)
    integ = b2.MapIntegrator(amb, 1, W, 1)
    try:
        nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
        cells = nD * nC
        assert held["tracks"] is True and held["n_rates"] == K and held["grid"] == -(-nC // 64) * -(-nD // 8)
        assert held["pfa"] == DET["pfa"] / K  # the union bound over the K hypotheses
        assert [r["cpi"] for r in res] == list(range(N)) and [bool(r.get("integrating")) for r in res] == [True, True] + [False] * 4
        st = torch.cuda.current_stream().cuda_stream
        walk = b2.nci_walk_table(amb, FC)
        assert np.abs(walk).max() * (W - 1) > 4  # the walk moves cells
        integ.set_tracks(walk, bank, B)
        d_map = torch.zeros((B, nD, nC), dtype=torch.complex64, device="cuda")
        d_met = torch.zeros((B, 2), dtype=torch.float64, device="cuda")
        d_out = torch.zeros((N, nD, nC), dtype=torch.complex64, device="cuda")
        d_omet = torch.zeros((N, 2), dtype=torch.float64, device="cuda")
        at = 0
        for k0 in range(0, N, B):  # the chain's batches
            d_iq = torch.from_numpy(iq[k0 * n:(k0 + B) * n].copy()).cuda()
            amb.process_dev(b2.FMT_I16, d_iq.data_ptr(), None, B, n, d_map.data_ptr(), d_met.data_ptr(), st)
            n_out, _ = integ.process_tracks_dev(d_map.data_ptr(), B, d_out[at].data_ptr(), None, d_omet[at].data_ptr(), B, None, st)
            at += n_out
        torch.cuda.synchronize()
        assert at == N - (W - 1)
        maps, mets = d_out[:at].cpu().numpy(), d_omet[:at].cpu().numpy()
        frames = [r for r in res if not r.get("integrating")]
        assert not any(np.array_equal(maps[i], p["map"]) for i, p in enumerate(q for q in plain if not q.get("integrating")))
        det = b2.CfarDetector1D(DET["pfa"] / K, DET["nGuard"], DET["nTrain"], DET["minDelay"], DET["minDoppler"], looks=W)
        fin = b2.DetectionFinisher(6, 6, 1 / (n / fs), True, True)
        for i, r in enumerate(frames):
            assert r["window"] == W
            assert np.array_equal(r["map"].view(np.uint32), maps[i].view(np.uint32)), r["cpi"]
            assert r["noisePower"] == mets[i, 0] and r["maxPower"] == mets[i, 1]
            d_m = torch.from_numpy(maps[i][None].copy()).cuda()
            d_e = torch.from_numpy(mets[i][None].copy()).cuda()
            d_hits = torch.zeros((1, cells, 2), dtype=torch.float64, device="cuda")
            d_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
            d_dets = torch.zeros((1, cells, 4), dtype=torch.float64, device="cuda")
            d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
            det.process_dev(amb, 1, d_hits.data_ptr(), cells, d_cnt.data_ptr(), d_m.data_ptr(), d_e.data_ptr(), st)
            fin.process_dev(amb, 1, d_hits.data_ptr(), cells, d_cnt.data_ptr(), d_dets.data_ptr(), cells, d_n.data_ptr(),
                            d_m.data_ptr(), d_e.data_ptr(), st)
            torch.cuda.synchronize()
            host = b2.dets_to_detection(d_dets[0].cpu().numpy().view(b2.DET_DTYPE).reshape(-1), int(d_n[0]), cells)
            assert r["delay"] == host.delay.tolist() and r["doppler"] == host.doppler.tolist() and r["snr"] == host.snr.tolist()
    finally:
        integ.close()
        amb.close()


def test_refusals(b2, capture, tmp_path):
    from blah2_amd import replay as R
    for bad in (True, {}, {"rate": 1}, {"fc": -1.0}, {"fc": float("nan")}, {"fc": "carrier"}, {"fc": FC, "rate": 8},
                {"fc": FC, "rate": True}, {"fc": FC, "rate": {"step": 1.0}}, {"fc": FC, "rate": {"max": 2, "step": 0.0}},
                {"fc": FC, "rate": {"max": 10.5, "step": 10.5}},  # the library's |q| (W - 1) < n_doppler
                {"fc": 1.0}):                                     # the library's BLAH2HIP_MAX_TRACK_SHIFT
        with pytest.raises(ValueError, match="integrate.tracks"):
            R.GpuChain(config(tracks=bad), 0, batch=B)
    yml = tmp_path / "config.yml"
    text = ("capture:\n  fs: 1000000\n{fc}  device:\n    type: RspDuo\nprocess:\n  data:\n    cpi: 0.1\n  ambiguity:\n"
            "    delayMin: -10\n    delayMax: 100\n    dopplerMin: -100\n    dopplerMax: 100\n"
            "  clutter:\n    enable: false\n  detection:\n    enable: false\n")
    yml.write_text(text.format(fc="  fc: 204640000\n"))
    path, _ = capture
    for argv in (["--integrate-tracks"], ["--integrate-tracks", "1"], ["--integrate", "3", "--integrate-tracks", "8"],
                 ["--integrate", "3", "--integrate-tracks", "2:0"], ["--integrate", "3", "--integrate-tracks", "-1"],
                 ["--integrate", "3", "--integrate-tracks", "fast"], ["--integrate", "3", "--integrate-tracks", "1:1:1"]):
        with pytest.raises(SystemExit):
            R.main([path, "--config", str(yml)] + argv)
    yml.write_text(text.format(fc=""))
    with pytest.raises(SystemExit):  # no carrier anywhere
        R.main([path, "--config", str(yml), "--integrate", "3", "--integrate-tracks", "1"])
