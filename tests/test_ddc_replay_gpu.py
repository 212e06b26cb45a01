"""GPU: the down-converter in the replay chain (``cfg["ddc"]``, ``replay.py --ddc OFFSET_HZ:DECIM[:TAPS[:CUTOFF[:BETA]]]``) on
the two-carrier scene of ddc_scenes.py, two CPIs (seeds 7 and 8) quantised to int16 as a .rspduo capture and to int8 as a
cs8 pair, replayed in batches of one CPI, so that the batches cut the stream and the second CPI's first outputs need the
history the first left.

  * the maps of carrier A equal the restatement chain's (blah2_amd.ddc on the quantised integers of the whole stream, then
    the oracle's ambiguity stage per CPI) within the cell-wise gate of oracle/gates.py; the detection lists agree cell
    for cell under its margin rule; echo A (delay 6, 40 Hz) is in both;
  * the second CPI is not what a zero history gives;
  * without the key (absent, None, False) the capture gives the plain chain's maps, metrics and lists, bit for bit;
  * refusals: a decimation that does not divide, values outside their ranges, several ranks; the command line's forms.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ddc_scenes as S
from oracle import blah2_oracle as O
from oracle import gates as G

SEEDS = (7, 8)
DET = dict(pfa=1e-5, nGuard=2, nTrain=6, minDelay=0, minDoppler=5.0)
DDC = {"offset": S.CARRIERS[0], "decimation": S.D, "taps": S.T}


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


def quantise(v, full):
    s = full / max(np.max(np.abs(v.real)), np.max(np.abs(v.imag)))
    return np.rint(v.real * s), np.rint(v.imag * s)


@pytest.fixture(scope="module")
def captures(tmp_path_factory):
    """The stream of both scenes, each channel scaled to its format's range and rounded: paths and the integers as complex128."""
    d = tmp_path_factory.mktemp("ddc")
    xs, ys = zip(*[S.scene(seed) for seed in SEEDS])
    x, y = np.concatenate(xs), np.concatenate(ys)
    out = {}
    (xr, xi), (yr, yi) = quantise(x, 30000.0), quantise(y, 30000.0)
    np.stack([xr, xi, yr, yi], axis=1).astype(np.int16).tofile(str(d / "cap.rspduo"))
    out["rspduo"] = (str(d / "cap.rspduo"), None, np.stack([xr + 1j * xi, yr + 1j * yi]))
    (xr, xi), (yr, yi) = quantise(x, 127.0), quantise(y, 127.0)
    np.stack([xr, xi], axis=1).astype(np.int8).tofile(str(d / "ref.cs8"))
    np.stack([yr, yi], axis=1).astype(np.int8).tofile(str(d / "surv.cs8"))
    out["cs8"] = (str(d / "ref.cs8"), str(d / "surv.cs8"), np.stack([xr + 1j * xi, yr + 1j * yi]))
    return out


def config(ddc="absent", **extra):
    a = S.AMB_ARGS
    cfg = dict({"fs": S.FS, "n_samples": S.N, "ambiguity": {"delayMin": a[0], "delayMax": a[1], "dopplerMin": a[2], "dopplerMax": a[3]},
                "detection": dict(DET, enable=True), "clutter": {"enable": False}}, **extra)
    if ddc != "absent":
        cfg["ddc"] = ddc
    return cfg


def run(captures, layout, cfg, batch=1):
    from blah2_amd import replay as R
    px, py, _ = captures[layout]
    cap = R.RspduoFile(px, S.N) if layout == "rspduo" else R.Cs8Pair(px, py, S.N)
    chain = R.GpuChain(cfg, 0, batch=batch, want_map=True, layout=layout)
    try:
        return R.replay(cap, chain, batch=batch), (chain.fs, chain.n, chain._fmt_in())
    finally:
        chain.close()
        cap.close()


@pytest.mark.parametrize("layout", ["rspduo", "cs8"])
def test_replay_equals_the_restatement_chain(b2, captures, layout):
    res, (fs, n, fmt) = run(captures, layout, config(DDC))
    assert (fs, n, fmt) == (S.FS // S.D, S.N // S.D, b2.FMT_C32)
    assert [r["cpi"] for r in res] == [0, 1] and not any(r.get("skipped") for r in res)
    u = captures[layout][2]
    h = S.taps()
    v, _ = b2.ddc(u, DDC["offset"], S.FS, S.D, h)  # the whole stream: CPI 1 sees CPI 0's last samples
    cold, _ = b2.ddc(u[:, S.N:], DDC["offset"], S.FS, S.D, h, first_sample=S.N)  # ... and what it would be without them
    dims = O.ambiguity_dims(*S.AMB_ARGS)
    for c, r in enumerate(res):
        pl = v[:, c * n:(c + 1) * n]
        ref = O.ambiguity_process(dims, pl[0], pl[1])
        noise_ref, _ = O.map_metrics(ref)
        cell = G.map_cell_gate(r["map"], ref, noise_ref)
        print(f"[{layout} cpi {c}] {cell}")
        assert cell["ok"], cell
        assert abs(r["noisePower"] - noise_ref) <= 1e-3
        dl, dp, _ = O.cfar1d_fast(ref, dims.delay, dims.doppler, noise_ref, DET["pfa"], DET["nGuard"], DET["nTrain"], DET["minDelay"],
                                  DET["minDoppler"])
        mg = G.cfar1d_margins(ref, DET["pfa"], DET["nGuard"], DET["nTrain"])
        dg = G.detection_gate(zip(dl, dp), zip(r["delay"], r["doppler"]), mg, dims.doppler, dims.delay[0], G.margin_eps(cell))
        print(f"[{layout} cpi {c}] detections: {dg}")
        assert dg["ok"] and dg["n_ref"] > 0, dg
        for lst in (zip(dl, dp), zip(r["delay"], r["doppler"])):
            assert any(d == S.PEAKS[0][0] and abs(f - S.PEAKS[0][1]) < 0.5 for d, f in lst)
    # the history matters: the restatement from a zero history is at least ten times further from CPI 1's map
    ref_cold = O.ambiguity_process(dims, cold[0], cold[1])
    assert G.map_cell_gate(res[1]["map"], ref_cold)["peak_rel"] > 10.0 * cell["peak_rel"]


def test_one_batch_of_two_cpis_gives_the_same_bits(b2, captures):
    one, _ = run(captures, "rspduo", config(DDC), batch=1)
    two, _ = run(captures, "rspduo", config(DDC), batch=2)
    for a, b in zip(one, two):
        assert np.array_equal(a["map"].view(np.uint32), b["map"].view(np.uint32))
        assert a["delay"] == b["delay"] and a["doppler"] == b["doppler"] and a["noisePower"] == b["noisePower"]


def test_no_key_is_the_plain_chain(b2, captures):
    a = S.AMB_ARGS
    res, (fs, n, fmt) = run(captures, "rspduo", config())
    assert (fs, n, fmt) == (S.FS, S.N, b2.FMT_I16)
    iq = np.fromfile(captures["rspduo"][0], dtype=np.int16).reshape(len(SEEDS), S.N, 4)
    amb = b2.Ambiguity(a[0], a[1], a[2], a[3], S.FS, S.N, True)
    det = b2.CfarDetector1D(DET["pfa"], DET["nGuard"], DET["nTrain"], DET["minDelay"], DET["minDoppler"])
    for c, r in enumerate(res):
        m = amb.process_i16(iq[c])
        m.set_metrics()
        d = det.process(m)
        assert np.array_equal(r["map"].view(np.uint32), np.asarray(m.data).view(np.uint32))
        assert r["noisePower"] == m.noisePower and r["maxPower"] == m.maxPower
        assert list(r["delay"]) == list(d.get_delay()) and list(r["doppler"]) == list(d.get_doppler())
    for off in (None, False):
        res2, _ = run(captures, "rspduo", config(off))
        for p, q in zip(res, res2):
            assert p.keys() == q.keys() and np.array_equal(p["map"].view(np.uint32), q["map"].view(np.uint32))
            assert all(p[k] == q[k] for k in p if k != "map")


def test_refusals(b2, captures, tmp_path):
    from blah2_amd import replay as R
    for bad in (True, {}, {"offset": 0.0}, {"decimation": 4}, {"offset": 0.0, "decimation": 0}, {"offset": 0.0, "decimation": 65},
                {"offset": 0.0, "decimation": 3}, {"offset": 0.0, "decimation": 2.5}, {"offset": 40000.0, "decimation": 4},
                {"offset": float("nan"), "decimation": 4}, {"offset": 0.0, "decimation": 4, "taps": 0},
                {"offset": 0.0, "decimation": 4, "taps": 1025}, {"offset": 0.0, "decimation": 4, "cutoff": 0.0},
                {"offset": 0.0, "decimation": 4, "beta": -1.0}):
        with pytest.raises(ValueError, match="capture.ddc"):
            R.GpuChain(config(bad), 0, batch=1)
    chain = R.GpuChain(config(DDC), 0, batch=1)
    assert chain.ddc_cfg["taps"] == S.T and chain.ddc_cfg["cutoff"] == 0.8 and chain.ddc_cfg["beta"] == 8.0
    with pytest.raises(ValueError, match="capture.ddc over 2 ranks"):
        chain.shard_check(2)
    chain.shard_check(1)
    chain.close()
    chain = R.GpuChain(config({"offset": 0.0, "decimation": 16}), 0, batch=1)  # taps: 16 D
    assert chain.ddc_cfg["taps"] == 256 and (chain.fs, chain.n) == (S.FS // 16, S.N // 16)
    chain.close()
    small = {"delayMin": 0, "delayMax": 4, "dopplerMin": -8, "dopplerMax": 8}  # (a map that 1024 samples at 1024 Hz can hold)
    chain = R.GpuChain(config({"offset": 0.0, "decimation": 64}, ambiguity=small), 0, batch=1)  # ... at most 1024
    assert chain.ddc_cfg["taps"] == 1024 and chain.ddc.tile >= 1
    chain.close()
    # the migration carrier is the down-converted carrier's own frequency
    cfg = config(DDC)
    cfg["ambiguity"]["migration"] = {"fc": 100.0e6}
    chain = R.GpuChain(cfg, 0, batch=1)
    plain = b2.Ambiguity(*S.AMB_ARGS)
    assert np.array_equal(chain.amb.migration_table(100.0e6 + DDC["offset"]), plain.migration_table(100.0e6 + DDC["offset"]))
    assert chain.migrate
    chain.close()
    yml = tmp_path / "config.yml"
    yml.write_text("capture:\n  fs: 65536\n  fc: 100000000\nprocess:\n  data:\n    cpi: 1.0\n  ambiguity:\n"
                   "    delayMin: -4\n    delayMax: 20\n    dopplerMin: -64\n    dopplerMax: 64\n"
                   "  clutter:\n    enable: false\n  detection:\n    enable: false\n")
    for argv in (["--ddc", "16384"], ["--ddc", "x:4"], ["--ddc", "16384:4.5"], ["--ddc", "16384:4:64:0.8:8:1"], ["--ddc"]):
        with pytest.raises(SystemExit):
            R.main([captures["rspduo"][0], "--config", str(yml)] + argv)


def test_command_line(b2, captures, tmp_path, capsys):
    """--ddc 16384:4:64 through main(): one JSON line per CPI, the values of the configured chain."""
    import json
    from blah2_amd import replay as R
    yml = tmp_path / "config.yml"
    yml.write_text("capture:\n  fs: 65536\nprocess:\n  data:\n    cpi: 1.0\n  ambiguity:\n"
                   "    delayMin: -4\n    delayMax: 20\n    dopplerMin: -64\n    dopplerMax: 64\n"
                   "  clutter:\n    enable: false\n  detection:\n    enable: true\n    pfa: 0.00001\n    nGuard: 2\n    nTrain: 6\n"
                   "    minDelay: 0\n    minDoppler: 5.0\n")
    R.main([captures["rspduo"][0], "--config", str(yml), "--batch", "1", "--ddc", "16384:4:64"])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    want, _ = run(captures, "rspduo", config(DDC))
    assert [ln["cpi"] for ln in lines] == [0, 1]
    for ln, w in zip(lines, want):
        assert ln["noisePower"] == w["noisePower"] and ln["delay"] == list(w["delay"]) and ln["doppler"] == list(w["doppler"])
