"""GPU: 8-bit captures through GpuChain(layout="cs8") -- two files of int8 I, Q pairs uploaded as they are and read by
the kernels as FMT_I8 / FMT_I8X_C32Y -- against the .rspduo replay of the same integers through the existing int16
chain (bit for bit: the formats differ in the load alone), and against the fp64 oracle at the configs[1] size."""
import os

import numpy as np
import pytest

from conftest import load_golden
from test_i8_gpu import as_c128, clipped_scene
from test_replay_gpu import medium_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


def write_both(base, cpis):
    """CPIs of int8 (x, y) [n, 2] pairs as a cs8 pair and as the .rspduo words of the same integers."""
    np.concatenate([c[0] for c in cpis]).tofile(base + ".ref.cs8")
    np.concatenate([c[1] for c in cpis]).tofile(base + ".surv.cs8")
    np.concatenate([np.concatenate([c[0], c[1]], axis=1).astype(np.int16) for c in cpis]).tofile(base + ".rspduo")
    return base + ".ref.cs8", base + ".surv.cs8", base + ".rspduo"


def replay_cs8(px, py, n, cfg, read_mode="memmove", batch=2, want_map=True):
    from blah2_amd import replay as R
    cap = R.Cs8Pair(px, py, n)
    chain = R.GpuChain(cfg, 0, batch=batch, want_map=want_map, reader_threads=3, read_mode=read_mode, layout="cs8")
    try:
        res = R.replay(cap, chain, batch=batch)
        assert chain.read_mode == read_mode  # mapped: /dev/shm pages register, no fall-back
        assert chain.fused_fir is False and chain._fmt_in() == chain.b2.FMT_I8
        return res
    finally:
        chain.close()
        cap.close()


def replay_rspduo(p, n, cfg, batch=2):
    from blah2_amd import replay as R
    cap = R.RspduoFile(p, n)
    chain = R.GpuChain(cfg, 0, batch=batch, want_map=True)
    try:
        res = R.replay(cap, chain, batch=batch)
        assert chain.fused_fir is False
        return res
    finally:
        chain.close()
        cap.close()


def medium_scene(g):
    fs, n = int(g["params"][0]), int(g["params"][1])
    xi, yi, _ = clipped_scene(n, 61, fs, lo=-127)  # [-127, 127]: the negation stays in int8
    return n, xi, yi


def test_cs8_replay_equals_the_rspduo_replay_of_the_same_integers(b2):
    """Three CPIs (scene, negated scene, scene) at the medium fixture's geometry, batch 2 (a ragged last batch), every
    read path, without and with the two-stage filter: metrics, detections and map bits per CPI."""
    g = load_golden("medium")
    n, xi, yi = medium_scene(g)
    base = f"/dev/shm/blah2_test_cs8_{os.getpid()}"
    px, py, pr = write_both(base, [(xi, yi), (-xi, -yi), (xi, yi)])
    plain = medium_cfg(g)
    filt = medium_cfg(g)
    filt["clutter"] = {"enable": True, "delayMin": int(g["clutter_params"][0]), "delayMax": int(g["clutter_params"][1]),
                       "fused": False}
    try:
        for cfg in (plain, filt):
            want = replay_rspduo(pr, n, cfg)
            assert [r["cpi"] for r in want] == [0, 1, 2] and not any(r.get("skipped") for r in want)
            assert len(want[0]["delay"]) >= 1
            for mode in ("memmove", "pread", "mapped"):
                got = replay_cs8(px, py, n, cfg, mode)
                assert [r["cpi"] for r in got] == [0, 1, 2]
                for a, b in zip(got, want):
                    assert not a.get("skipped")
                    assert a["noisePower"] == b["noisePower"] and a["maxPower"] == b["maxPower"]
                    assert a["delay"] == b["delay"] and a["doppler"] == b["doppler"] and a["snr"] == b["snr"]
                    assert np.array_equal(a["map"].view(np.uint32), b["map"].view(np.uint32))
    finally:
        for p in (px, py, pr):
            os.remove(p)


def test_cs8_replay_skips_cpis_whose_clutter_filter_fails(b2, tmp_path):
    """blah2.cpp:270-273 on an 8-bit capture: an all-zero reference channel in CPI 1 drops that CPI only."""
    g = load_golden("medium")
    n, xi, yi = medium_scene(g)
    px, py, pr = write_both(str(tmp_path / "cap"), [(xi, yi), (np.zeros_like(xi), yi), (xi, yi)])
    cfg = medium_cfg(g)
    cfg["clutter"] = {"enable": True, "delayMin": int(g["clutter_params"][0]), "delayMax": int(g["clutter_params"][1])}
    res = replay_cs8(px, py, n, cfg, batch=3, want_map=False)
    assert [bool(r.get("skipped")) for r in res] == [False, True, False]
    assert res[0]["noisePower"] == res[2]["noisePower"] and res[0]["delay"] == res[2]["delay"]


def test_cs8_chain_refuses_the_other_layouts(b2, tmp_path):
    from blah2_amd import replay as R
    g = load_golden("medium")
    n, xi, yi = medium_scene(g)
    px, py, pr = write_both(str(tmp_path / "cap"), [(xi, yi)])
    chain = R.GpuChain(medium_cfg(g), 0, batch=1, layout="cs8")
    with pytest.raises(ValueError):
        R.replay(R.RspduoFile(pr, n), chain)
    with pytest.raises(ValueError):
        chain(np.zeros((1, n, 4), dtype=np.int16))
    chain.close()
    for layout, kw in (("rspduo", {}), ("usrp", {"usrp_block": 2040})):
        chain = R.GpuChain(medium_cfg(g), 0, batch=1, layout=layout, **kw)
        with pytest.raises(ValueError):
            R.replay(R.Cs8Pair(px, py, n), chain)
        chain.close()
    with pytest.raises(ValueError):
        R.GpuChain(medium_cfg(g), 0, batch=1, layout="cu8")


def test_cs8_replay_at_the_timed_size(b2):
    """configs[1] (2 MS/s, 1 s CPI, 513 x 411) with the 410-tap filter and the 1-D CFAR, two CPIs from two files in
    /dev/shm, one batch of 2, through GpuChain(layout="cs8"): both CPIs within the oracle's gates (the fp64 chain fed the
    clipped integers), as test_usrp_replay_at_the_timed_size applies them."""
    from blah2_amd import replay as R
    from gates import cfar1d_margins, detection_gate, margin_eps
    from oracle import blah2_oracle as O
    from test_full_chain_gpu import check_chain_map
    fs = n = 2_000_000
    geom = (-10, 400, -256, 256, fs, n)
    cpis = [clipped_scene(n, 41 + c, fs)[:2] for c in range(2)]
    px, py, pr = write_both(f"/dev/shm/blah2_test_cs8_cfg2_{os.getpid()}", cpis)
    os.remove(pr)
    cfg = {"fs": fs, "n_samples": n,
           "ambiguity": {"delayMin": -10, "delayMax": 400, "dopplerMin": -256, "dopplerMax": 256},
           "detection": {"enable": True, "pfa": 1e-5, "nGuard": 2, "nTrain": 6, "minDelay": 5, "minDoppler": 15.0},
           "clutter": {"enable": True, "delayMin": -10, "delayMax": 400}}
    try:
        res = replay_cs8(px, py, n, cfg)
    finally:
        os.remove(px)
        os.remove(py)
    assert [r["cpi"] for r in res] == [0, 1] and not any(r.get("skipped") for r in res)
    d = O.ambiguity_dims(*geom, True)
    for c in range(2):
        x0, y0 = as_c128(cpis[c][0]), as_c128(cpis[c][1])
        _, y_ref, _, _, b_ref = O.wiener_hopf(x0, y0, -10, 400, return_filter=True)
        ref = O.ambiguity_process(d, x0, y_ref)
        noise_ref, max_ref = O.map_metrics(ref)
        direct_level = np.max(np.abs(b_ref)) * (d.n_corr * d.n_doppler_bins / n)
        cell = check_chain_map(f"configs[1] cs8 replay cpi {c}", res[c]["map"], res[c]["noisePower"], ref, noise_ref,
                               direct_level, d.doppler, d.delay, -10, 400)
        assert abs(res[c]["noisePower"] - noise_ref) <= 1e-3 and abs(res[c]["maxPower"] - max_ref) <= 1e-3
        dl, dp, _ = O.cfar1d_fast(ref, d.delay, d.doppler, noise_ref, 1e-5, 2, 6, 5, 15.0)
        mg = cfar1d_margins(ref, 1e-5, 2, 6)
        dg = detection_gate(zip(dl, dp), zip(res[c]["delay"], res[c]["doppler"]), mg, d.doppler, d.delay[0], margin_eps(cell))
        print(f"[configs[1] cs8 replay cpi {c}] detections: {dg}")
        assert dg["ok"] and dg["n_ref"] > 0, dg
