"""GPU: the Doppler-rate bank in the replay chain (``cfg["ambiguity"]["dopplerRate"] = QMAX | {"max": QMAX, "step": S}``,
``replay.py --doppler-rate QMAX[:STEP]``), on the capture of tests/test_migrate_replay_gpu.py.

  * no key, ``None`` and ``False``: the same frames, byte for byte, nothing set on the handle, no launch
    (BLAH2HIP_INFO_RATE_GRID stays 0) and the detector at the configured pfa;
  * with the key the chain's maps and metrics are the bits of ``process_dev`` + ``rate_bank_dev`` (in place) on the same
    batches, and its detections those of ``CfarDetector1D(pfa / K)`` and the finisher on them;
  * with ``migration`` configured too, the table is set and exactly one second-sum kernel runs, the new one:
    BLAH2HIP_INFO_MIGRATE_GRID stays 0, and the frames are the by-hand chain's with the table set;
  * the ValueErrors name the key; the command line refuses its forms of them.
"""
import numpy as np
import pytest

from test_migrate_replay_gpu import B, DET, FC, N, SMALL, capture_cpis, same_frames

pytestmark = pytest.mark.gpu

QMAX, STEP, K = 3.0, 1.5, 5  # -3, -1.5, 0, 1.5, 3


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def config(rate="absent", migration=None):
    amb = {"delayMin": SMALL[0], "delayMax": SMALL[1], "dopplerMin": SMALL[2], "dopplerMax": SMALL[3]}
    if rate != "absent":
        amb["dopplerRate"] = rate
    if migration:
        amb["migration"] = migration
    return {"fs": SMALL[4], "n_samples": SMALL[5], "ambiguity": amb, "detection": dict(DET), "clutter": {"enable": False}}


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("rate") / "cap.rspduo")
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
        return res, {"rates": chain.rates, "migrate": chain.migrate, "pfa": chain.cfar.pfa,
                     "rate_grid": chain.amb.info(_lib.INFO_RATE_GRID), "migrate_grid": chain.amb.info(_lib.INFO_MIGRATE_GRID)}
    finally:
        chain.close()
        cap.close()


_plain = {}


def plain_of(path):
    if "p" not in _plain:
        _plain["p"] = run(path, config())
    return _plain["p"]


def test_no_key_is_the_chain_without_the_feature(b2, capture):
    path, _ = capture
    plain, held = plain_of(path)
    assert held["rates"] is None and held["rate_grid"] == 0 and held["pfa"] == DET["pfa"]
    assert [r["cpi"] for r in plain] == list(range(N)) and sum(len(r["delay"]) for r in plain) > 0
    for off in (None, False):
        res, held = run(path, config(rate=off))
        assert held["rates"] is None and held["rate_grid"] == 0 and held["pfa"] == DET["pfa"] and same_frames(res, plain), off


@pytest.mark.parametrize("form,migration", [("dict", False), ("number", False), ("dict", True)], ids=["dict", "number", "with-migration"])
def test_chain_is_process_dev_and_rate_bank_dev_on_the_same_batches(b2, torch, capture, form, migration):
    path, iq = capture
    plain, _ = plain_of(path)
    rate, bank = ({"max": QMAX, "step": STEP}, b2.rate_bank(QMAX, STEP)) if form == "dict" else (2, b2.rate_bank(2))
    assert bank.size == K
    res, held = run(path, config(rate, {"fc": FC} if migration else None))
    n, fs = SMALL[5], SMALL[4]
    amb = b2.Ambiguity(*SMALL, True, max_batch=B)
    try:
        nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
        cells = nD * nC
        # what the chain set and launched: the bank, the table only when asked for, one second-sum kernel and never migrate_dev's
        assert np.array_equal(held["rates"], bank) and held["migrate"] is migration
        assert held["rate_grid"] == -(-nC // 64) * -(-nD // 16) and held["migrate_grid"] == 0
        assert held["pfa"] == DET["pfa"] / K  # the union bound over the K hypotheses
        assert [r["cpi"] for r in res] == list(range(N))
        st = torch.cuda.current_stream().cuda_stream
        if migration:
            amb.set_migration(amb.migration_table(FC))
        amb.set_rates(bank)
        d_map = torch.zeros((N, nD, nC), dtype=torch.complex64, device="cuda")
        d_met = torch.zeros((N, 2), dtype=torch.float64, device="cuda")
        for k0 in range(0, N, B):  # the chain's batches
            d_iq = torch.from_numpy(iq[k0 * n:(k0 + B) * n].copy()).cuda()
            amb.process_dev(b2.FMT_I16, d_iq.data_ptr(), None, B, n, d_map[k0].data_ptr(), d_met[k0].data_ptr(), st)
            if k0 == 0:
                torch.cuda.synchronize()
                assert np.array_equal(d_map[0].cpu().numpy().view(np.uint32), plain[0]["map"].view(np.uint32))
            amb.rate_bank_dev(d_map[k0].data_ptr(), B, d_map[k0].data_ptr(), None, d_met[k0].data_ptr(), st)
        torch.cuda.synchronize()
        maps, mets = d_map.cpu().numpy(), d_met.cpu().numpy()
        assert not any(np.array_equal(maps[i], plain[i]["map"]) for i in range(N))
        det = b2.CfarDetector1D(DET["pfa"] / K, DET["nGuard"], DET["nTrain"], DET["minDelay"], DET["minDoppler"])
        fin = b2.DetectionFinisher(6, 6, 1 / (n / fs), True, True)
        for i, r in enumerate(res):
            assert np.array_equal(r["map"].view(np.uint32), maps[i].view(np.uint32)), r["cpi"]
            assert r["noisePower"] == mets[i, 0] and r["maxPower"] == mets[i, 1]
            d_m = torch.from_numpy(maps[i][None].copy()).cuda()
            d_e = torch.from_numpy(mets[i][None].copy()).cuda()
            d_hits = torch.zeros((1, cells, 2), dtype=torch.float64, device="cuda")
            d_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
            d_out = torch.zeros((1, cells, 4), dtype=torch.float64, device="cuda")
            d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
            det.process_dev(amb, 1, d_hits.data_ptr(), cells, d_cnt.data_ptr(), d_m.data_ptr(), d_e.data_ptr(), st)
            fin.process_dev(amb, 1, d_hits.data_ptr(), cells, d_cnt.data_ptr(), d_out.data_ptr(), cells, d_n.data_ptr(),
                            d_m.data_ptr(), d_e.data_ptr(), st)
            torch.cuda.synchronize()
            host = b2.dets_to_detection(d_out[0].cpu().numpy().view(b2.DET_DTYPE).reshape(-1), int(d_n[0]), cells)
            assert r["delay"] == host.delay.tolist() and r["doppler"] == host.doppler.tolist() and r["snr"] == host.snr.tolist()
        assert sum(len(r["delay"]) for r in res) > 0
    finally:
        amb.close()


def test_refusals(b2, capture, tmp_path):
    from blah2_amd import replay as R
    nD = 21
    for bad in (8, {"max": 4, "step": 0.5}, {"step": 1.0}, {}, {"max": 2, "step": 0.0}, {"max": 2, "step": -1.0}, -1.0, float("nan"),
                {"max": float("inf")}, "fast", True, {"max": 10 * nD, "step": 5.0 * nD}):  # the last: the library's |q| <= nD
        with pytest.raises(ValueError, match="dopplerRate"):
            R.GpuChain(config(rate=bad), 0, batch=B)
    yml = tmp_path / "config.yml"
    yml.write_text("capture:\n  fs: 1000000\n  device:\n    type: RspDuo\nprocess:\n  data:\n    cpi: 0.1\n  ambiguity:\n"
                   "    delayMin: -10\n    delayMax: 100\n    dopplerMin: -100\n    dopplerMax: 100\n"
                   "  clutter:\n    enable: false\n  detection:\n    enable: false\n")
    path, _ = capture
    for argv in (["--doppler-rate", "8"], ["--doppler-rate", "2:0"], ["--doppler-rate", "-1"], ["--doppler-rate", "fast"],
                 ["--doppler-rate", "1:1:1"], ["--doppler-rate", "nan"]):
        with pytest.raises(SystemExit):
            R.main([path, "--config", str(yml)] + argv)
