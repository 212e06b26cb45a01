"""GPU: the clutter map in the replay chain (``cfg["detection"]["clutterMap"] = {"memory": T, "mode": "gate" | "detect"}``,
``replay.py --clutter-map T[:detect]``) on a small synthetic capture: a noise-like reference, the surveillance channel with
the direct path, a FIXED echo at 37 bins and -60 Hz in every CPI and a MOVING one at +40 Hz whose delay grows by three
bins per CPI.

  * no key, ``None`` and ``False``: the same frames, byte for byte, and no clutter map on the chain;
  * ``gate``: the detector reports the fixed echo in every CPI, the gated chain in none (a cell never exceeds 26 times --
    alpha[8] at pfa 1e-5 -- its own average while its level stays), and the moving echo stays from age 4 on (alpha[4] = 67:
    the echo stands 30 dB over the floor); age 0 reports nothing at all;
  * ``detect``: the same two statements about the clutter map's own list;
  * the ValueErrors name the key; the command line refuses its forms of them.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL = (-10, 100, -100, 100, 1_000_000, 100_000)  # 21 x 111
B, N, T = 4, 12, 8
DET = {"enable": True, "pfa": 1e-5, "nGuard": 2, "nTrain": 6, "minDelay": 5, "minDoppler": 15.0, "nCentroid": 6}
FIXED = (37, -60.0)
MOVING0, STEP, MOVING_HZ = 44, 3, 40.0


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


def capture_cpis(n, fs, n_cpi, seed):
    """int16 [n_cpi * n, 4] (I1 Q1 I2 Q2), tests/test_migrate_replay_gpu.py's capture with a second echo that moves."""
    rng = np.random.default_rng(seed)
    total = n_cpi * n
    t = np.arange(total) / fs
    x = 300.0 * (rng.standard_normal(total) + 1j * rng.standard_normal(total))
    y = 0.8 * x + 30.0 * (rng.standard_normal(total) + 1j * rng.standard_normal(total))
    xd = np.roll(x, FIXED[0])
    xd[:FIXED[0]] = 0
    y += 0.1 * xd * np.exp(2j * np.pi * FIXED[1] * t)
    for g in range(n_cpi):
        d = MOVING0 + STEP * g
        seg = slice(g * n, (g + 1) * n)
        xm = np.roll(x, d)[seg]
        if g == 0:
            xm[:d] = 0
        y[seg] += 0.1 * xm * np.exp(2j * np.pi * MOVING_HZ * t[seg])
    iq = np.stack([x.real, x.imag, y.real, y.imag], axis=1)
    return np.clip(np.rint(iq), -32768, 32767).astype(np.int16)


def config(cmap="absent", **extra):
    amb = {"delayMin": SMALL[0], "delayMax": SMALL[1], "dopplerMin": SMALL[2], "dopplerMax": SMALL[3]}
    det = dict(DET)
    if cmap != "absent":
        det["clutterMap"] = cmap
    return dict({"fs": SMALL[4], "n_samples": SMALL[5], "ambiguity": amb, "detection": det, "clutter": {"enable": False}}, **extra)


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("cmap") / "cap.rspduo")
    capture_cpis(SMALL[5], SMALL[4], N, 3).tofile(path)
    return path


def run(path, cfg):
    from blah2_amd import replay as R
    chain = R.GpuChain(cfg, 0, batch=B, want_map=True)
    cap = R.RspduoFile(path, SMALL[5])
    try:
        res = R.replay(cap, chain, batch=B)
        return res, (chain.cmap is not None, chain.cmap_mode, chain.cmap.age() if chain.cmap is not None else None)
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


def near(frame, delay, hz):
    """Is there a detection within 1.5 bins and 8 Hz (the resolution is 10 Hz) of the place?"""
    return any(abs(d - delay) <= 1.5 and abs(f - hz) <= 8.0 for d, f in zip(frame["delay"], frame["doppler"]))


_plain = {}


def plain_of(path):
    if "p" not in _plain:
        _plain["p"] = run(path, config())
    return _plain["p"]


def test_no_key_is_the_chain_without_the_feature(b2, capture):
    plain, held = plain_of(capture)
    assert held == (False, None, None) and [r["cpi"] for r in plain] == list(range(N))
    assert all(near(r, *FIXED) for r in plain)                                     # the detector reports what repeats
    assert all(near(r, MOVING0 + STEP * g, MOVING_HZ) for g, r in enumerate(plain))
    for off in (None, False):
        res, held = run(capture, config(cmap=off))
        assert held == (False, None, None) and same_frames(res, plain), off


@pytest.mark.parametrize("mode", ["gate", "detect", None], ids=["gate", "detect", "default-is-gate"])
def test_fixed_echo_goes_moving_echo_stays(b2, capture, mode):
    plain, _ = plain_of(capture)
    res, held = run(capture, config(cmap={"memory": T} if mode is None else {"memory": T, "mode": mode}))
    assert held == (True, mode or "gate", N)  # every CPI absorbed, in order, across the batches
    assert [r["cpi"] for r in res] == list(range(N))
    for p, r in zip(plain, res):  # the maps and metrics are the chain's own: the stage reads, it does not write
        assert np.array_equal(p["map"].view(np.uint32), r["map"].view(np.uint32)) and p["noisePower"] == r["noisePower"]
    assert res[0]["delay"] == []  # age 0: nothing exceeds
    fixed = [near(r, *FIXED) for r in res]
    moving = [near(r, MOVING0 + STEP * g, MOVING_HZ) for g, r in enumerate(res)]
    print(mode, "fixed", fixed, "moving", moving, "detections", [len(r["delay"]) for r in res], "plain", [len(r["delay"]) for r in plain])
    assert not any(fixed)
    assert all(moving[4:])
    if mode != "detect":  # the gate only drops: every frame a subset of the detector's hits, so never more detections
        assert all(len(r["delay"]) <= len(p["delay"]) for p, r in zip(plain, res))


def test_refusals(b2, capture, tmp_path):
    from blah2_amd import replay as R
    for bad in (True, {}, {"memory": 0}, {"memory": 65}, {"memory": "8"}, {"memory": 8.0}, {"memory": True},
                {"memory": 8, "mode": "censor"}):
        with pytest.raises(ValueError, match="detection.clutterMap"):
            R.GpuChain(config(cmap=bad), 0, batch=B)
    with pytest.raises(ValueError, match="detection.clutterMap"):
        R.GpuChain(config(cmap={"memory": 8}, integrate={"window": 2, "hop": 1}), 0, batch=B)
    cfg = config(cmap={"memory": 8})
    cfg["detection"]["enable"] = False
    with pytest.raises(ValueError, match="detection.clutterMap"):
        R.GpuChain(cfg, 0, batch=B)
    chain = R.GpuChain(config(cmap={"memory": 8}), 0, batch=B)
    try:
        chain.shard_check(1)
        with pytest.raises(ValueError, match="detection.clutterMap"):
            chain.shard_check(2)
    finally:
        chain.close()
    yml = tmp_path / "config.yml"
    yml.write_text("capture:\n  fs: 1000000\n  device:\n    type: RspDuo\nprocess:\n  data:\n    cpi: 0.1\n  ambiguity:\n"
                   "    delayMin: -10\n    delayMax: 100\n    dopplerMin: -100\n    dopplerMax: 100\n"
                   "  clutter:\n    enable: false\n  detection:\n    enable: false\n")
    for argv in (["--clutter-map", "0"], ["--clutter-map", "65"], ["--clutter-map", "eight"], ["--clutter-map", "8:censor"],
                 ["--clutter-map", "8:detect:1"], ["--integrate", "3", "--clutter-map", "8"], ["--clutter-map"]):
        with pytest.raises(SystemExit):
            R.main([capture, "--config", str(yml)] + argv)
