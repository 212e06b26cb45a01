"""GPU: range-migration compensation in the replay chain (``cfg["ambiguity"]["migration"] = {"fc": HZ}``,
``replay.py --migration``).

  * no key, ``None`` and ``False``: the same frames, byte for byte, and nothing set on the handle;
  * with the key the chain's maps and metrics are the bits of ``process_dev`` + ``migrate_dev`` (in place) on the same
    batches, and its detections those of the same detector and finisher on them -- also with ``window: hann`` and
    ``integrate: {window: 2}`` behind it (``taper_dev`` and ``MapIntegrator`` over the migrated maps);
  * no ``fc``, an ``fc`` that is not positive and finite, and a table beyond BLAH2HIP_MAX_MIGRATION are refused; so are
    the command line's forms of them.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL = (-10, 100, -100, 100, 1_000_000, 100_000)  # 21 x 111, nCorr 4761
B, N = 2, 4
DET = {"enable": True, "pfa": 1e-5, "nGuard": 2, "nTrain": 6, "minDelay": 5, "minDoppler": 15.0, "nCentroid": 6}
FC = 0.5 * 100.0 * 4761 * 20 / 3.25  # the outermost rows walk 3 cells from the middle of the CPI to its end


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def capture_cpis(n, fs, n_cpi, seed):
    """int16 [n_cpi * n, 4] (I1 Q1 I2 Q2): a noise-like reference, the surveillance channel 0.8 of it plus an echo at
    37 bins and -60 Hz and noise of its own (tests/test_taper_replay_gpu.py's capture)."""
    rng = np.random.default_rng(seed)
    total = n_cpi * n
    x = 300.0 * (rng.standard_normal(total) + 1j * rng.standard_normal(total))
    xd = np.roll(x, 37)
    xd[:37] = 0
    y = 0.8 * x + 0.05 * xd * np.exp(-2j * np.pi * 60.0 * np.arange(total) / fs) + 30.0 * (rng.standard_normal(total) + 1j * rng.standard_normal(total))
    iq = np.stack([x.real, x.imag, y.real, y.imag], axis=1)
    return np.clip(np.rint(iq), -32768, 32767).astype(np.int16)


def config(migration="absent", window=None, integrate=None):
    amb = {"delayMin": SMALL[0], "delayMax": SMALL[1], "dopplerMin": SMALL[2], "dopplerMax": SMALL[3]}
    if migration != "absent":
        amb["migration"] = migration
    if window:
        amb["window"] = window
    cfg = {"fs": SMALL[4], "n_samples": SMALL[5], "ambiguity": amb, "detection": dict(DET), "clutter": {"enable": False}}
    if integrate:
        cfg["integrate"] = {"window": integrate, "hop": 1}
    return cfg


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("migrate") / "cap.rspduo")
    iq = capture_cpis(SMALL[5], SMALL[4], N, 3)
    iq.tofile(path)
    return path, iq


def run(path, cfg):
    from blah2_amd import replay as R
    chain = R.GpuChain(cfg, 0, batch=B, want_map=True)
    cap = R.RspduoFile(path, SMALL[5])
    try:
        return R.replay(cap, chain, batch=B), chain.migrate
    finally:
        chain.close()
        cap.close()


def same_frames(a, b):
    if len(a) != len(b):
        return False
    for p, q in zip(a, b):
        if p.keys() != q.keys() or not np.array_equal(p["map"].view(np.uint32), q["map"].view(np.uint32)):
            return False
        if any(p[k] != q[k] for k in p if k != "map"):
            return False
    return True


_plain = {}


def plain_of(path):
    if "p" not in _plain:
        _plain["p"] = run(path, config())
    return _plain["p"]


def test_no_key_is_the_chain_without_the_feature(b2, capture):
    path, _ = capture
    plain, on = plain_of(path)
    assert on is False and [r["cpi"] for r in plain] == list(range(N))
    assert sum(len(r["delay"]) for r in plain) > 0
    for off in (None, False):
        res, on = run(path, config(migration=off))
        assert on is False and same_frames(res, plain), off


@pytest.mark.parametrize("window,integrate", [(None, None), ("hann", 2)], ids=["plain", "hann-integrate2"])
def test_chain_is_process_dev_and_migrate_dev_on_the_same_batches(b2, torch, capture, window, integrate):
    path, iq = capture
    plain, _ = plain_of(path)
    res, on = run(path, config({"fc": FC}, window, integrate))
    assert on is True and [r["cpi"] for r in res] == list(range(N))
    n, fs = SMALL[5], SMALL[4]
    amb = b2.Ambiguity(*SMALL, True, max_batch=B)    # the chain's batches
    big = b2.Ambiguity(*SMALL, True, max_batch=N)    # what runs behind them here, over all N maps at once
    try:
        nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
        cells = nD * nC
        st = torch.cuda.current_stream().cuda_stream
        table = amb.migration_table(FC)
        s = b2.migration_shifts(table, nD)
        assert np.abs(s).max() == 3 and np.array_equal(table, b2.migration_table(amb, FC))
        amb.set_migration(table)
        d_map = torch.zeros((N, nD, nC), dtype=torch.complex64, device="cuda")
        d_met = torch.zeros((N, 2), dtype=torch.float64, device="cuda")
        for k0 in range(0, N, B):  # the chain's batches
            d_iq = torch.from_numpy(iq[k0 * n:(k0 + B) * n].copy()).cuda()
            amb.process_dev(b2.FMT_I16, d_iq.data_ptr(), None, B, n, d_map[k0].data_ptr(), d_met[k0].data_ptr(), st)
            if k0 == 0:
                torch.cuda.synchronize()
                assert np.array_equal(d_map[0].cpu().numpy().view(np.uint32), plain[0]["map"].view(np.uint32))
            amb.migrate_dev(d_map[k0].data_ptr(), B, d_map[k0].data_ptr(), d_met[k0].data_ptr(), st)
        if window:
            d_t, d_tmet = torch.zeros_like(d_map), torch.zeros_like(d_met)
            big.taper_dev(d_map.data_ptr(), N, b2.doppler_taper_f32(window), d_t.data_ptr(), d_tmet.data_ptr(), st)
            d_map, d_met = d_t, d_tmet
        torch.cuda.synchronize()
        maps, mets = d_map.cpu().numpy(), d_met.cpu().numpy()
        zero = np.rint(table * (nD - 1)) == 0
        if not window:
            assert all(np.array_equal(maps[i][zero].view(np.uint32), plain[i]["map"][zero].view(np.uint32)) for i in range(N))
            assert not any(np.array_equal(maps[i][~zero], plain[i]["map"][~zero]) for i in range(N))
        W = integrate or 1
        if integrate:
            assert all(r == {"integrating": True, "cpi": g} for g, r in enumerate(res[:W - 1]))
            integ = b2.MapIntegrator(big, 1, W, 1)
            try:
                want = integ.process(maps[None])
            finally:
                integ.close()
            maps = np.stack([m.data for m in want])
            mets = np.array([[m.noisePower, m.maxPower] for m in want])
        det = b2.CfarDetector1D(DET["pfa"], DET["nGuard"], DET["nTrain"], DET["minDelay"], DET["minDoppler"], looks=W)
        fin = b2.DetectionFinisher(6, 6, 1 / (n / fs), True, True)
        for i, r in enumerate(res[W - 1:]):
            assert r["cpi"] == i + W - 1
            assert np.array_equal(r["map"].view(np.uint32), maps[i].view(np.uint32)), r["cpi"]
            assert r["noisePower"] == mets[i, 0] and r["maxPower"] == mets[i, 1]
            d_m = torch.from_numpy(maps[i][None].copy()).cuda()
            d_e = torch.from_numpy(mets[i][None].copy()).cuda()
            d_hits = torch.zeros((1, cells, 2), dtype=torch.float64, device="cuda")
            d_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
            d_out = torch.zeros((1, cells, 4), dtype=torch.float64, device="cuda")
            d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
            det.process_dev(big, 1, d_hits.data_ptr(), cells, d_cnt.data_ptr(), d_m.data_ptr(), d_e.data_ptr(), st)
            fin.process_dev(big, 1, d_hits.data_ptr(), cells, d_cnt.data_ptr(), d_out.data_ptr(), cells, d_n.data_ptr(),
                            d_m.data_ptr(), d_e.data_ptr(), st)
            torch.cuda.synchronize()
            host = b2.dets_to_detection(d_out[0].cpu().numpy().view(b2.DET_DTYPE).reshape(-1), int(d_n[0]), cells)
            assert r["delay"] == host.delay.tolist() and r["doppler"] == host.doppler.tolist() and r["snr"] == host.snr.tolist()
    finally:
        amb.close()
        big.close()


def test_refusals(b2, capture, tmp_path):
    from blah2_amd import replay as R
    for bad in ({}, {"fc": None}, {"fc": 0.0}, {"fc": -1e8}, {"fc": float("nan")}, {"fc": float("inf")}):
        with pytest.raises(ValueError):
            R.GpuChain(config(migration=bad), 0, batch=B)
    with pytest.raises(ValueError, match="MAX_MIGRATION"):
        R.GpuChain(config(migration={"fc": FC * 3.0 / 600.0}), 0, batch=B)  # 600 cells
    # the command line: a config without capture.fc and no value, a value that is no frequency
    yml = tmp_path / "config.yml"
    yml.write_text("capture:\n  fs: 1000000\n  device:\n    type: RspDuo\nprocess:\n  data:\n    cpi: 0.1\n  ambiguity:\n"
                   "    delayMin: -10\n    delayMax: 100\n    dopplerMin: -100\n    dopplerMax: 100\n"
                   "  clutter:\n    enable: false\n  detection:\n    enable: false\n")
    path, _ = capture
    for argv in (["--migration"], ["--migration", "-5"], ["--migration", "nan"], ["--migration", "carrier"]):
        with pytest.raises(SystemExit):
            R.main([path, "--config", str(yml)] + argv)
