"""GPU: the Doppler taper in the replay chain (``cfg["ambiguity"]["window"]``, ``replay.py --doppler-window``).

  * ``window: none`` and no key: the same frames, byte for byte;
  * ``window: blackman``: the chain's maps and metrics are the bits of ``Ambiguity.taper_dev`` on the no-window chain's maps,
    and its detections those of the same detector and finisher on them -- also with the integrator behind the taper
    (``integrate: {window: 2}``: the windows are ``MapIntegrator``'s over the tapered maps, the detector made for 2 looks) and
    with the ordered-statistic detector (``detection.cfar: os``);
  * an unknown name, a malformed one and a stencil wider than the map are refused.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL = (-10, 100, -100, 100, 1_000_000, 100_000)  # 21 x 111
B, N = 2, 4
DET = {"enable": True, "pfa": 1e-5, "nGuard": 2, "nTrain": 6, "minDelay": 5, "minDoppler": 15.0, "nCentroid": 6}


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
    37 bins and -60 Hz and noise of its own."""
    rng = np.random.default_rng(seed)
    total = n_cpi * n
    x = 300.0 * (rng.standard_normal(total) + 1j * rng.standard_normal(total))
    xd = np.roll(x, 37)
    xd[:37] = 0
    y = 0.8 * x + 0.05 * xd * np.exp(-2j * np.pi * 60.0 * np.arange(total) / fs) + 30.0 * (rng.standard_normal(total) + 1j * rng.standard_normal(total))
    iq = np.stack([x.real, x.imag, y.real, y.imag], axis=1)
    return np.clip(np.rint(iq), -32768, 32767).astype(np.int16)


def config(window="absent", integrate=None, cfar="ca"):
    amb = {"delayMin": SMALL[0], "delayMax": SMALL[1], "dopplerMin": SMALL[2], "dopplerMax": SMALL[3]}
    if window != "absent":
        amb["window"] = window
    cfg = {"fs": SMALL[4], "n_samples": SMALL[5], "ambiguity": amb, "detection": dict(DET, cfar=cfar), "clutter": {"enable": False}}
    if integrate:
        cfg["integrate"] = {"window": integrate, "hop": 1}
    return cfg


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("taper") / "cap.rspduo")
    capture_cpis(SMALL[5], SMALL[4], N, 3).tofile(path)
    return path


def run(path, cfg):
    from blah2_amd import replay as R
    chain = R.GpuChain(cfg, 0, batch=B, want_map=True)
    cap = R.RspduoFile(path, SMALL[5])
    try:
        return R.replay(cap, chain, batch=B), (chain.taper is not None, all("d_tmap" in s for s in chain.slots))
    finally:
        chain.close()
        cap.close()


_plain = {}


def plain_of(path, cfar):
    if cfar not in _plain:
        _plain[cfar] = run(path, config(cfar=cfar))
    return _plain[cfar]


def same_frames(a, b):
    if len(a) != len(b):
        return False
    for p, q in zip(a, b):
        if p.keys() != q.keys() or not np.array_equal(p["map"].view(np.uint32), q["map"].view(np.uint32)):
            return False
        if any(p[k] != q[k] for k in p if k != "map"):
            return False
    return True


def test_no_window_is_the_chain_without_the_feature(b2, capture):
    plain, state = plain_of(capture, "ca")
    assert state == (False, False) and [r["cpi"] for r in plain] == list(range(N))
    assert sum(len(r["delay"]) for r in plain) > 0
    for window in ("none", None, "NONE"):
        res, state = run(capture, config(window=window))
        assert state == (False, False), window  # nothing allocated, nothing to launch
        assert same_frames(res, plain), window


@pytest.mark.parametrize("integrate,cfar", [(None, "ca"), (2, "ca"), (None, "os"), (2, "os")],
                         ids=["plain", "integrate2", "os", "integrate2-os"])
def test_blackman_chain_is_taper_dev_on_the_plain_chains_maps(b2, torch, capture, integrate, cfar):
    plain, _ = plain_of(capture, cfar)
    res, state = run(capture, config("blackman", integrate, cfar))
    assert state == (True, True) and [r["cpi"] for r in res] == list(range(N))
    n, fs = SMALL[5], SMALL[4]
    amb = b2.Ambiguity(*SMALL, True, max_batch=N)
    try:
        nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
        cells = nD * nC
        st = torch.cuda.current_stream().cuda_stream
        d_in = torch.from_numpy(np.stack([r["map"] for r in plain])).cuda()
        d_t = torch.zeros_like(d_in)
        d_tmet = torch.zeros((N, 2), dtype=torch.float64, device="cuda")
        amb.taper_dev(d_in.data_ptr(), N, b2.doppler_taper_f32("blackman"), d_t.data_ptr(), d_tmet.data_ptr(), st)
        torch.cuda.synchronize()
        maps, mets = d_t.cpu().numpy(), d_tmet.cpu().numpy()
        assert not np.array_equal(maps, d_in.cpu().numpy())
        W = integrate or 1
        if integrate:
            assert all(r == {"integrating": True, "cpi": g} for g, r in enumerate(res[:W - 1]))
            integ = b2.MapIntegrator(amb, 1, W, 1)
            try:
                want = integ.process(maps[None])
            finally:
                integ.close()
            assert [m._cpi_index for m in want] == list(range(W - 1, N))
            maps = np.stack([m.data for m in want])
            mets = np.array([[m.noisePower, m.maxPower] for m in want])
        looks = {"looks": W}
        det = (b2.OsCfarDetector1D(DET["pfa"], DET["nGuard"], DET["nTrain"], DET["minDelay"], DET["minDoppler"], rank=0.75, **looks)
               if cfar == "os" else b2.CfarDetector1D(DET["pfa"], DET["nGuard"], DET["nTrain"], DET["minDelay"], DET["minDoppler"], **looks))
        fin = b2.DetectionFinisher(6, 6, 1 / (n / fs), True, True)
        step = float(amb.doppler[1] - amb.doppler[0])
        found = 0
        for i, r in enumerate(res[W - 1:]):
            assert r["cpi"] == i + W - 1 and ("window" in r) == bool(integrate)
            assert np.array_equal(r["map"].view(np.uint32), maps[i].view(np.uint32)), r["cpi"]
            assert r["noisePower"] == mets[i, 0] and r["maxPower"] == mets[i, 1]
            d_map = torch.from_numpy(maps[i][None].copy()).cuda()
            d_met = torch.from_numpy(mets[i][None].copy()).cuda()
            d_hits = torch.zeros((1, cells, 2), dtype=torch.float64, device="cuda")
            d_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
            d_out = torch.zeros((1, cells, 4), dtype=torch.float64, device="cuda")
            d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
            det.process_dev(amb, 1, d_hits.data_ptr(), cells, d_cnt.data_ptr(), d_map.data_ptr(), d_met.data_ptr(), st)
            fin.process_dev(amb, 1, d_hits.data_ptr(), cells, d_cnt.data_ptr(), d_out.data_ptr(), cells, d_n.data_ptr(),
                            d_map.data_ptr(), d_met.data_ptr(), st)
            torch.cuda.synchronize()
            host = b2.dets_to_detection(d_out[0].cpu().numpy().view(b2.DET_DTYPE).reshape(-1), int(d_n[0]), cells)
            assert r["delay"] == host.delay.tolist() and r["doppler"] == host.doppler.tolist() and r["snr"] == host.snr.tolist()
            hit = (np.abs(np.array(r["delay"]) - 37) < 1.0) & (np.abs(np.array(r["doppler"]) + 60.0) < step)
            found += bool(hit.any())
        assert found == N - W + 1, "the echo is missing from a tapered frame"
    finally:
        amb.close()


def test_normalised_window_and_refusals(b2, torch, capture):
    res, _ = run(capture, config("hamming:norm"))
    plain, _ = plain_of(capture, "ca")
    # an echo on a Doppler bin keeps its amplitude: the peak cell of the map stays within the window's scalloping of it
    for r, p in zip(res, plain):
        at = np.unravel_index(int(np.argmax(np.abs(p["map"]))), p["map"].shape)
        assert 0.5 < abs(r["map"][at]) / abs(p["map"][at]) < 1.5
    from blah2_amd import replay as R
    for bad in ("taylor", "hann:peak", "blackman:norm:norm"):
        with pytest.raises(ValueError):
            R.GpuChain(config(bad), 0, batch=B)
    narrow = config("flattop")
    narrow["ambiguity"].update(dopplerMin=-30, dopplerMax=30)  # 7 Doppler bins, 9 taps
    with pytest.raises(ValueError):
        R.GpuChain(narrow, 0, batch=B)
