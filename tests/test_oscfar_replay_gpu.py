"""GPU: the replay chain with the ordered-statistic detector in the place of CfarDetector1D (detection.cfar: os, replay.py
--cfar os[:RANK]).  The hit buffers, the finisher and the JSON writers are the chain's own; with cfar: ca, or without the
key, the chain is what it was."""
import json

import numpy as np
import pytest

from conftest import load_golden
from test_replay_gpu import medium_cfg

pytestmark = pytest.mark.gpu


def capture(tmp_path, g):
    path = str(tmp_path / "cap.rspduo")
    rng = np.random.default_rng(3)
    np.concatenate([g["iq"], -g["iq"], np.roll(g["iq"], int(rng.integers(1, 50)), axis=0)]).tofile(path)
    return path


def test_chain_with_the_ordered_statistic_detector(built_lib, tmp_path):
    import blah2_amd as b2
    from blah2_amd import replay as R
    g = load_golden("medium")
    n = int(g["params"][1])
    path = capture(tmp_path, g)
    cfg = medium_cfg(g)
    cfg["detection"]["pfa"] = 0.05  # (the fixture's own pfa leaves three strong echoes, which every detector finds)
    out = {}
    for name, extra in (("absent", {}), ("ca", {"cfar": "ca"}), ("os", {"cfar": "os"}), ("os-half", {"cfar": "os", "rank": 0.5})):
        c = dict(cfg, detection=dict(cfg["detection"], **extra))
        chain = R.GpuChain(c, 0, batch=2, want_map=True)
        assert type(chain.cfar).__name__ == ("OsCfarDetector1D" if name.startswith("os") else "CfarDetector1D")
        res = R.replay(R.RspduoFile(path, n), chain, batch=2)
        assert [r["cpi"] for r in res] == [0, 1, 2]
        if name.startswith("os"):
            det_c = c["detection"]
            det = b2.OsCfarDetector1D(det_c["pfa"], det_c["nGuard"], det_c["nTrain"], det_c["minDelay"], det_c["minDoppler"],
                                      rank=extra.get("rank", 0.75))
            assert chain.cfar.rank_permille == det.rank_permille == (500 if "rank" in extra else 750)
            for r in res:
                m = b2.Map(None, r["map"], chain.amb.delay, chain.amb.doppler, r["noisePower"], r["maxPower"])
                want = det.process(m, amb=chain.amb)
                assert want.get_nDetections() > 0
                assert r["delay"] == want.get_delay().tolist() and r["doppler"] == want.get_doppler().tolist()
                assert np.allclose(r["snr"], want.get_snr(), rtol=0, atol=1e-9)
                # and the restatement on the same map
                alpha, rank = b2.oscfar_alpha_table(det.pfa, 1, det.rank_permille, 2 * det.nTrain)
                rows, cols, snr = b2.oscfar_hits(r["map"], chain.amb.delay, chain.amb.doppler, r["noisePower"], alpha, rank,
                                                 (det.nGuard, det.nTrain), det.minDelay, det.minDoppler)
                assert r["delay"] == (cols + float(chain.amb.delay[0])).tolist() and r["doppler"] == chain.amb.doppler[rows].tolist()
        chain.close()
        out[name] = [{k: (v.tobytes().hex() if k == "map" else v) for k, v in r.items()} for r in res]
    assert json.dumps(out["ca"]) == json.dumps(out["absent"])
    assert min(len(r["delay"]) for r in out["absent"]) > 3
    assert [r["delay"] for r in out["os"]] != [r["delay"] for r in out["absent"]]
    assert [len(r["delay"]) for r in out["os-half"]] != [len(r["delay"]) for r in out["os"]]
    with pytest.raises(ValueError):
        R.GpuChain(dict(cfg, detection=dict(cfg["detection"], cfar="go")), 0, batch=2)


def test_replay_command_line_takes_the_detector(built_lib, tmp_path, capsys):
    """python -m blah2_amd.replay CAPTURE -c config.yml --cfar os[:RANK] emits detection frames; --integrate makes the
    detector for W looks as it does for the averaging one."""
    import yaml
    from blah2_amd import replay as R
    g = load_golden("medium")
    fs, n, dmin, dmax, fmin, fmax, rh = (int(v) for v in g["params"])
    pfa, ng, nt, md, mdop = g["det_params"][:5]
    cap = capture(tmp_path, g)
    cfgp = str(tmp_path / "config.yml")
    yaml.safe_dump({"capture": {"fs": fs},
                    "process": {"data": {"cpi": n / fs},
                                "ambiguity": {"delayMin": dmin, "delayMax": dmax, "dopplerMin": fmin, "dopplerMax": fmax},
                                "clutter": {"enable": False, "delayMin": dmin, "delayMax": dmax},
                                "detection": {"enable": True, "pfa": 0.05, "nGuard": int(ng), "nTrain": int(nt),
                                              "minDelay": int(md), "minDoppler": float(mdop), "nCentroid": 6}},
                    "network": {"ip": "0.0.0.0", "ports": {"map": 3001, "detection": 3002}}}, open(cfgp, "w"))
    frames = {}
    for flag in (None, "ca", "os", "os:0.5"):
        R.main([cap, "-c", cfgp, "--batch", "2", "--json"] + (["--cfar", flag] if flag else []))
        lines = capsys.readouterr().out.strip().split("\n")
        assert len(lines) == 6  # (map, detection) x 3 CPIs
        frames[flag] = [json.loads(x) for x in lines[1::2]]
        assert all(list(d) == ["timestamp", "delay", "doppler", "snr"] for d in frames[flag])
    assert frames["ca"] == frames[None]
    assert all(len(d["delay"]) > 0 for d in frames["os"]) and frames["os"] != frames[None] and frames["os:0.5"] != frames["os"]
    for bad in ("so", "ca:0.5", "os:0", "os:1.5", "os:x"):
        with pytest.raises(SystemExit):
            R.main([cap, "-c", cfgp, "--cfar", bad])
    capsys.readouterr()
    chain = R.GpuChain({"fs": fs, "n_samples": n,
                        "ambiguity": {"delayMin": dmin, "delayMax": dmax, "dopplerMin": fmin, "dopplerMax": fmax},
                        "detection": {"enable": True, "pfa": float(pfa), "nGuard": int(ng), "nTrain": int(nt), "minDelay": int(md),
                                      "minDoppler": float(mdop), "cfar": "os"},
                        "integrate": {"window": 2}}, 0, batch=2)
    assert type(chain.cfar).__name__ == "OsCfarDetector1D" and chain.cfar.looks == 2
    chain.close()
