"""GPU: the replay chain with the greatest-of / smallest-of detector in the place of CfarDetector1D (detection.cfar: goca |
soca).  The capture is a clutter-edge scene in the sample domain: the surveillance channel holds the reference at the
delays 60 .. 79, each under its own slow random modulation (band-limited to the map's Doppler rows), so the map has a
plateau some 14 dB over its floor, twenty columns wide, with an edge on either side.  The chain's frames equal the mirror's
(``GoCfarDetector1D.process`` and ``gocfar_hits`` on the chain's own maps); with cfar: ca, or without the key, the chain is
what it was."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 16384
CFG = {"fs": N, "n_samples": N, "ambiguity": {"delayMin": -4, "delayMax": 123, "dopplerMin": -16, "dopplerMax": 16},
       "detection": {"enable": True, "pfa": 1e-3, "nGuard": 2, "nTrain": 8, "minDelay": -128, "minDoppler": 0.0},
       "clutter": {"enable": False}}


def edge_capture(path, n_cpi=3):
    """int16 I1 Q1 I2 Q2: x white, y = sum_{d = 60 .. 79} c_d[n] x[n - d] + a little noise, c_d[n] = sum_{|f| <= 16} A e^(2 pi i f n / N)."""
    rng = np.random.default_rng(20261023)
    t = np.arange(N)
    out = []
    for _ in range(n_cpi):
        x = (rng.standard_normal(N) + 1j * rng.standard_normal(N)) / np.sqrt(2.0)
        y = 0.05 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
        for d in range(60, 80):
            spec = np.zeros(N, dtype=np.complex128)
            f = np.arange(-16, 17)
            spec[f % N] = (rng.standard_normal(f.size) + 1j * rng.standard_normal(f.size)) / np.sqrt(2.0)
            c = np.fft.ifft(spec) * N / np.sqrt(33.0 * 20.0)
            y = y + c * np.roll(x, d)
        iq = np.stack([x.real, x.imag, y.real, y.imag], axis=1) * 3000.0
        out.append(np.clip(np.rint(iq), -32767, 32767).astype(np.int16))
    np.concatenate(out).tofile(path)
    return t.size


def test_chain_with_the_split_window_detectors(built_lib, tmp_path):
    import blah2_amd as b2
    from blah2_amd import replay as R
    path = str(tmp_path / "edge.rspduo")
    edge_capture(path)
    out, cells = {}, {}
    for name, extra in (("absent", {}), ("ca", {"cfar": "ca"}), ("goca", {"cfar": "goca"}), ("soca", {"cfar": "soca"})):
        c = dict(CFG, detection=dict(CFG["detection"], **extra))
        chain = R.GpuChain(c, 0, batch=2, want_map=True)
        assert type(chain.cfar).__name__ == ("GoCfarDetector1D" if name.endswith("oca") else "CfarDetector1D")
        res = R.replay(R.RspduoFile(path, N), chain, batch=2)
        assert [r["cpi"] for r in res] == [0, 1, 2]
        cells[name] = [set(zip(r["doppler"], r["delay"])) for r in res]
        if name.endswith("oca"):
            det_c = c["detection"]
            det = b2.GoCfarDetector1D(det_c["pfa"], det_c["nGuard"], det_c["nTrain"], det_c["minDelay"], det_c["minDoppler"], kind=name[:2])
            assert chain.cfar.kind == det.kind == (1 if name == "goca" else 2)
            nD, nC = res[0]["map"].shape
            table = b2.gocfar_table_for(det.pfa, det.kind, nD, nC, (det.nGuard, det.nTrain))
            for r in res:
                m = b2.Map(None, r["map"], chain.amb.delay, chain.amb.doppler, r["noisePower"], r["maxPower"])
                want = det.process(m, amb=chain.amb)
                assert want.get_nDetections() > 0
                assert r["delay"] == want.get_delay().tolist() and r["doppler"] == want.get_doppler().tolist()
                assert np.allclose(r["snr"], want.get_snr(), rtol=0, atol=1e-9)
                rows, cols, snr = b2.gocfar_hits(r["map"], chain.amb.delay, chain.amb.doppler, r["noisePower"], table, det.kind,
                                                 (det.nGuard, det.nTrain), det.minDelay, det.minDoppler)
                assert r["delay"] == (cols + float(chain.amb.delay[0])).tolist() and r["doppler"] == chain.amb.doppler[rows].tolist()
        chain.close()
        out[name] = [{k: (v.tobytes().hex() if k == "map" else v) for k, v in r.items()} for r in res]
    assert json.dumps(out["ca"]) == json.dumps(out["absent"])
    # the ten columns inside the plateau behind its leading edge (delays 60 .. 69): smallest-of reports noise there
    inside = {k: sum(1 for s in v for _, d in s if 60 <= d < 70) for k, v in cells.items()}
    print("hits in the ten columns behind the edge, three CPIs:", inside, "| all:", {k: sum(len(s) for s in v) for k, v in cells.items()})
    assert inside["soca"] > 3 * max(inside["ca"], inside["goca"], 1)  # (at 14 dB the averaging detector's excess is a few cells)
    assert cells["goca"] != cells["ca"] and cells["soca"] != cells["ca"]
    for bad in ("go", "so"):
        with pytest.raises(ValueError):
            R.GpuChain(dict(CFG, detection=dict(CFG["detection"], cfar=bad)), 0, batch=2)
    with pytest.raises(ValueError, match="detection.cfar"):
        R.GpuChain(dict(CFG, detection=dict(CFG["detection"], cfar="goca"), integrate={"window": 2}), 0, batch=2)


def test_replay_command_line_takes_the_detector(built_lib, tmp_path, capsys):
    import yaml
    from blah2_amd import replay as R
    cap = str(tmp_path / "edge.rspduo")
    edge_capture(cap)
    cfgp = str(tmp_path / "config.yml")
    yaml.safe_dump({"capture": {"fs": N},
                    "process": {"data": {"cpi": 1.0}, "ambiguity": CFG["ambiguity"],
                                "clutter": {"enable": False, "delayMin": -4, "delayMax": 123},
                                "detection": dict(CFG["detection"], nCentroid=6)},
                    "network": {"ip": "0.0.0.0", "ports": {"map": 3001, "detection": 3002}}}, open(cfgp, "w"))
    frames = {}
    for flag in (None, "ca", "goca", "soca"):
        R.main([cap, "-c", cfgp, "--batch", "2", "--json"] + (["--cfar", flag] if flag else []))
        lines = capsys.readouterr().out.strip().split("\n")
        assert len(lines) == 6  # (map, detection) x 3 CPIs
        frames[flag] = [json.loads(x) for x in lines[1::2]]
        assert all(list(d) == ["timestamp", "delay", "doppler", "snr"] for d in frames[flag])
    assert frames["ca"] == frames[None]
    assert frames["goca"] != frames[None] and frames["soca"] != frames[None] and frames["goca"] != frames["soca"]
    for bad in ("go", "so", "goca:0.5"):
        with pytest.raises(SystemExit):
            R.main([cap, "-c", cfgp, "--cfar", bad])
    with pytest.raises(SystemExit):
        R.main([cap, "-c", cfgp, "--cfar", "goca", "--integrate", "2"])
    capsys.readouterr()
