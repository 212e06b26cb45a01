"""GPU: strong-echo cancellation in the replay chain (``cfg["detection"]["clean"]``, ``replay.py --clean SNR_DB[:E]``) on the
demonstration scene of clean_scenes.py as a small C32 (USRP) capture of two CPIs.

  * the merged detection list equals the restatement chain's (clean_scenes.chain), cell for cell, under the margin rule of
    oracle/gates.py for cells near the threshold; the values agree to 1e-3;
  * the weak echo is reported only with the option;
  * the pass-2 map's median floor over the scene's check cells is within 0.5 dB of the restatement's;
  * without the key (absent, None, False) the frames are the plain chain's, byte for byte;
  * the refusals name the key; the command line refuses its forms of them.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import clean_scenes as S
from oracle import blah2_oracle as O
from oracle import gates as G

BLOCK, SEEDS = 4096, (20261021, 20261022)


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


@pytest.fixture(scope="module")
def scenes():
    return [S.demo_scene(seed) for seed in SEEDS]


@pytest.fixture(scope="module")
def capture(tmp_path_factory, scenes):
    """x block, then y block, BLOCK complex64 values each (Usrp.cpp's file)."""
    path = str(tmp_path_factory.mktemp("clean") / "cap.usrp")
    x = np.concatenate([s[0] for s in scenes]).reshape(-1, BLOCK)
    y = np.concatenate([s[1] for s in scenes]).reshape(-1, BLOCK)
    np.stack([x, y], axis=1).astype(np.complex64).tofile(path)
    return path


def config(clean="absent", **extra):
    a = S.AMB_ARGS
    det = dict(S.DET, enable=True)
    if clean != "absent":
        det["clean"] = clean
    return dict({"fs": S.FS, "n_samples": S.N, "ambiguity": {"delayMin": a[0], "delayMax": a[1], "dopplerMin": a[2], "dopplerMax": a[3]},
                 "detection": det, "clutter": {"enable": False}}, **extra)


def run(path, cfg, **kw):
    from blah2_amd import replay as R
    chain = R.GpuChain(cfg, 0, batch=2, want_map=True, layout="usrp", usrp_block=BLOCK, **kw)
    cap = R.UsrpFile(path, S.N, BLOCK)
    try:
        return R.replay(cap, chain, batch=2)
    finally:
        chain.close()
        cap.close()


_plain = {}


def plain_of(path):
    if "p" not in _plain:
        _plain["p"] = run(path, config())
    return _plain["p"]


def cells(dims, delay, doppler):
    ax = np.asarray(dims.doppler)
    return [(float(np.rint(d)), float(ax[int(np.argmin(np.abs(ax - f)))])) for d, f in zip(delay, doppler)]


def test_merged_list_and_floor_against_the_restatement(b2, capture, scenes):
    res = run(capture, config(clean=dict(S.CLEAN)))
    plain = plain_of(capture)
    assert [r["cpi"] for r in res] == [0, 1]
    for (x, y), r, p in zip(scenes, res, plain):
        ref = S.chain(x, y)
        dims = ref["dims"]
        assert r["cancelled"] == len(ref["used"]) == 1
        # the pass-2 map: the floor over the check cells, and the cell gate's measured error for the margin rule
        f_got, f_ref = S.floor_db(r["map"].astype(np.complex128), dims), S.floor_db(ref["m2"], dims)
        drop = S.floor_db(p["map"].astype(np.complex128), dims) - f_got
        print(f"cpi {r['cpi']}: floor {f_got:.2f} dB (restatement {f_ref:.2f}), drop {drop:.1f} dB")
        assert abs(f_got - f_ref) <= 0.5 and drop > 20.0
        eps = G.margin_eps(G.map_cell_gate(r["map"], ref["m2"]))
        margin = G.cfar1d_margins(ref["m2"], S.DET["pfa"], S.DET["nGuard"], S.DET["nTrain"])
        got_c, ref_c = cells(dims, r["delay"], r["doppler"]), cells(dims, ref["merged"]["delay"], ref["merged"]["doppler"])
        g = G.detection_gate(ref_c, got_c, margin, dims.doppler, dims.delay[0], eps)
        print(g)
        assert g["ok"], g
        if g["n_differ"] == 0:
            assert len(got_c) == len(ref_c)
            o_g, o_r = np.lexsort(np.array(got_c).T), np.lexsort(np.array(ref_c).T)
            for k, name in (("delay", "delay"), ("doppler", "doppler"), ("snr", "snr")):
                assert np.allclose(np.asarray(r[k])[o_g], ref["merged"][name][o_r], rtol=0, atol=1e-3), k
        # the weak echo: only with the option
        assert any(abs(d - S.WEAK[1]) <= 1.5 and abs(f - S.WEAK[2]) <= 1.5 for d, f in zip(r["delay"], r["doppler"]))
        assert not any(abs(d - S.WEAK[1]) <= 1.5 and abs(f - S.WEAK[2]) <= 1.5 for d, f in zip(p["delay"], p["doppler"]))
        assert any(abs(d - S.STRONG[1]) <= 1.5 and abs(f - S.STRONG[2]) <= 1.5 for d, f in zip(r["delay"], r["doppler"]))


def test_no_key_is_the_chain_without_the_feature(b2, capture):
    plain = plain_of(capture)
    assert all("cancelled" not in r for r in plain)
    for off in (None, False):
        res = run(capture, config(clean=off))
        assert len(res) == len(plain)
        for p, q in zip(plain, res):
            assert p.keys() == q.keys() and np.array_equal(p["map"].view(np.uint32), q["map"].view(np.uint32))
            assert all(p[k] == q[k] for k in p if k != "map")


def test_refusals(b2, capture, tmp_path):
    from blah2_amd import replay as R
    kw = dict(layout="usrp", usrp_block=BLOCK)
    for bad in (True, {}, {"snr": "18"}, {"snr": 18, "echoes": 0}, {"snr": 18, "echoes": 33}, {"snr": 18, "sideDelay": 3},
                {"snr": 18, "sideDoppler": 2}, {"snr": 18, "loading": -1.0}, {"snr": float("nan")}):
        with pytest.raises(ValueError, match="detection.clean"):
            R.GpuChain(config(clean=bad), 0, batch=2, **kw)
    with pytest.raises(ValueError, match="detection.clean"):  # the integrator would see every CPI twice
        R.GpuChain(config(clean={"snr": 18}, integrate={"window": 2, "hop": 1}), 0, batch=2, **kw)
    with pytest.raises(ValueError, match="detection.clean"):  # int16 words and no filter: no fp32 surveillance plane
        R.GpuChain(config(clean={"snr": 18}), 0, batch=2)
    with pytest.raises(ValueError, match="detection.clean"):  # the final lists are made on the host
        R.GpuChain(config(clean={"snr": 18}), 0, batch=2, detect="host", **kw)
    cfg = config(clean={"snr": 18})
    del cfg["detection"]["nCentroid"]
    with pytest.raises(ValueError, match="detection.clean"):
        R.GpuChain(cfg, 0, batch=2, **kw)
    yml = tmp_path / "config.yml"
    yml.write_text("capture:\n  fs: 32768\n  device:\n    type: Usrp\nprocess:\n  data:\n    cpi: 1.0\n  ambiguity:\n"
                   "    delayMin: -10\n    delayMax: 100\n    dopplerMin: -64\n    dopplerMax: 64\n"
                   "  clutter:\n    enable: false\n  detection:\n    enable: false\n")
    for argv in (["--clean", "loud"], ["--clean", "18:0"], ["--clean", "18:33"], ["--clean", "18:4:1"], ["--clean"],
                 ["--integrate", "3", "--clean", "18"], ["--clutter-map", "8", "--clean", "18"]):
        with pytest.raises(SystemExit):
            R.main([capture, "--config", str(yml), "--format", "usrp", "--usrp-block", str(BLOCK)] + argv)
