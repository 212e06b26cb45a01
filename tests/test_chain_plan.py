"""CPU, no library: ``blah2_amd.chain_plan.plan_chain`` -- the replay chain's config validated and normalised without a
device -- and the command line of ``blah2_amd.replay`` in front of it.

  * every refusal that the dictionary alone decides, with the bad values the ``*_replay_gpu.py`` files hand to ``GpuChain``,
    names its key; the values that only a handle can refuse pass the plan;
  * the defaults; absent, None and False are one plan; pfa over the hypothesis counts; carriers behind a down-converter;
    ``clean`` and the fused FIR; ``needs_order``; ``fmt_in`` per layout;
  * ``main()`` with ``gpu_processor`` stubbed: the bad argument lists of the GPU files exit, a good form of each flag hands the
    chain the dictionary form of its key, a bad value in the YAML exits before a chain is made.
"""
import json
import subprocess
import sys

import numpy as np
import pytest
import yaml

from blah2_amd import _lib, ddc_design
from blah2_amd import replay as R
from blah2_amd.chain_plan import plan_chain

FS = N = 65536
FC = 204640000.0
PFA = 1e-5
DET = dict(enable=True, pfa=PFA, nGuard=2, nTrain=6, minDelay=0, minDoppler=5.0)
USRP = dict(layout="usrp", usrp_block=363)


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the plan loaded the library")
    monkeypatch.setattr(_lib, "load", refuse)


def config(ddc="absent", amb=None, det=None, **extra):
    cfg = dict({"fs": FS, "n_samples": N,
                "ambiguity": dict({"delayMin": -4, "delayMax": 20, "dopplerMin": -64, "dopplerMax": 64}, **(amb or {})),
                "detection": dict(DET, **(det or {})), "clutter": {"enable": False}}, **extra)
    if ddc != "absent":
        cfg["ddc"] = ddc
    return cfg


def test_plan_needs_no_torch():
    code = ("import sys; from blah2_amd.chain_plan import plan_chain; "
            "p = plan_chain({'fs': 8, 'n_samples': 8, 'ambiguity': {}, 'ddc': {'offset': 1.0, 'decimation': 2}}); "
            "assert p.n == 4 and 'torch' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=R.__file__.rsplit("/", 2)[0])


def test_argument_refusals():
    with pytest.raises(ValueError, match="layout"):
        plan_chain({}, layout="kraken")
    for block in (None, 0, -3):
        with pytest.raises(ValueError, match="usrp_block"):
            plan_chain({}, layout="usrp", usrp_block=block)
    with pytest.raises(ValueError, match="detect"):
        plan_chain({}, detect="elsewhere")


DDC_BAD = (True, {}, {"offset": 0.0}, {"decimation": 4}, {"offset": 0.0, "decimation": 0}, {"offset": 0.0, "decimation": 65},
           {"offset": 0.0, "decimation": 3}, {"offset": 0.0, "decimation": 2.5}, {"offset": 40000.0, "decimation": 4},
           {"offset": float("nan"), "decimation": 4}, {"offset": 0.0, "decimation": 4, "taps": 0},
           {"offset": 0.0, "decimation": 4, "taps": 1025}, {"offset": 0.0, "decimation": 4, "cutoff": 0.0},
           {"offset": 0.0, "decimation": 4, "beta": -1.0})
CMAP_BAD = (True, {}, {"memory": 0}, {"memory": 65}, {"memory": "8"}, {"memory": 8.0}, {"memory": True}, {"memory": 8, "mode": "censor"})
CLEAN_BAD = (True, {}, {"snr": "18"}, {"snr": 18, "echoes": 0}, {"snr": 18, "echoes": 33}, {"snr": 18, "sideDelay": 3},
             {"snr": 18, "sideDoppler": 2}, {"snr": 18, "loading": -1.0}, {"snr": float("nan")})
RATE_BAD = (8, {"max": 4, "step": 0.5}, {"step": 1.0}, {}, {"max": 2, "step": 0.0}, {"max": 2, "step": -1.0}, -1.0, float("nan"),
            {"max": float("inf")}, "fast", True)
MIGRATION_BAD = ({}, {"fc": None}, {"fc": 0.0}, {"fc": -1e8}, {"fc": float("nan")}, {"fc": float("inf")})
TRACKS_BAD = (True, {}, {"rate": 1}, {"fc": -1.0}, {"fc": float("nan")}, {"fc": "carrier"}, {"fc": FC, "rate": 8},
              {"fc": FC, "rate": True}, {"fc": FC, "rate": {"step": 1.0}}, {"fc": FC, "rate": {"max": 2, "step": 0.0}})
REFUSALS = (
    [("capture.ddc", config(bad), {}) for bad in DDC_BAD] +
    [("detection.clutterMap", config(det={"clutterMap": bad}), {}) for bad in CMAP_BAD] +
    [("detection.clutterMap", config(det={"clutterMap": {"memory": 8}}, integrate={"window": 2, "hop": 1}), {}),
     ("detection.clutterMap", config(det={"clutterMap": {"memory": 8}, "enable": False}), {})] +
    [("detection.clean", config(det={"clean": bad, "nCentroid": 6}), USRP) for bad in CLEAN_BAD] +
    [("detection.clean", config(det={"clean": {"snr": 18}, "nCentroid": 6}, integrate={"window": 2, "hop": 1}), USRP),
     ("detection.clean", config(det={"clean": {"snr": 18}, "nCentroid": 6, "clutterMap": {"memory": 8}}), USRP),
     ("detection.clean", config(det={"clean": {"snr": 18}, "nCentroid": 6}), {}),  # int16 words and no filter: no fp32 plane
     ("detection.clean", config(det={"clean": {"snr": 18}, "nCentroid": 6}), {"layout": "cs8"}),
     ("detection.clean", config(det={"clean": {"snr": 18}, "nCentroid": 6}), dict(USRP, detect="host")),
     ("detection.clean", config(det={"clean": {"snr": 18}}), USRP)] +  # no nCentroid: no device finisher
    [("ambiguity.dopplerRate", config(amb={"dopplerRate": bad}), {}) for bad in RATE_BAD] +
    [("ambiguity.migration", config(amb={"migration": bad}), {}) for bad in MIGRATION_BAD] +
    [("integrate.tracks", config(integrate={"window": 3, "hop": 1, "tracks": bad}), {}) for bad in TRACKS_BAD] +
    [("detection.cfar", config(det={"cfar": "go"}), {})] +
    [("ambiguity.window", config(amb={"window": bad}), {}) for bad in ("taylor", "hann:peak", "blackman:norm:norm")])


@pytest.mark.parametrize("key,cfg,kw", REFUSALS, ids=[f"{k}-{i}" for i, (k, _, _) in enumerate(REFUSALS)])
def test_refusals_name_the_key(key, cfg, kw):
    with pytest.raises(ValueError, match=key):
        plan_chain(cfg, **kw)


def test_what_only_a_handle_refuses_passes_the_plan():
    nD = 129
    assert len(plan_chain(config(amb={"dopplerRate": {"max": 10 * nD, "step": 5.0 * nD}})).rates) == 5  # |q| above the Doppler bins
    assert plan_chain(config(amb={"migration": {"fc": 1.0}})).migrate_fc == 1.0                          # a walk beyond MAX_MIGRATION
    assert plan_chain(config(integrate={"window": 3, "tracks": {"fc": 1.0}})).tracks == (1.0, None)      # ... beyond MAX_TRACK_SHIFT
    assert plan_chain(config(amb={"window": "flattop", "dopplerMin": -3, "dopplerMax": 3})).taper == ("flattop", False)  # 9 taps, 7 bins


def test_defaults():
    p = plan_chain(config())
    assert (p.fs_in, p.n_in, p.fs, p.n, p.layout, p.usrp_block, p.batch) == (FS, N, FS, N, "rspduo", None, 1)
    assert (p.ddc, p.taper, p.migrate_fc, p.rates, p.integrate, p.tracks, p.cmap, p.clean, p.centroid, p.detect, p.cap) == (None,) * 11
    assert (p.cfar_kind, p.rank, p.pfa, p.needs_order) == ("ca", 0.75, PFA, False)
    assert p.clutter == {"enable": False, "blocks": 1, "fused": False}
    assert plan_chain(config(det={"cfar": "OS"})).cfar_kind == "os" and plan_chain(config(det={"cfar": "os", "rank": 0.5})).rank == 0.5
    assert plan_chain(config(det={"enable": False})).cfar_kind is None
    assert plan_chain(config(det={"capacity": 100}), batch=4).cap == 100
    for D, taps in ((4, 64), (16, 256), (64, 1024)):  # 16 D, at most 1024
        d = plan_chain(config({"offset": 0.0, "decimation": D})).ddc
        assert {k: d[k] for k in d if k != "h"} == {"offset": 0.0, "decimation": D, "taps": taps, "cutoff": 0.8, "beta": 8.0}
        assert np.array_equal(d["h"], ddc_design(D, taps, 0.8, 8.0))
    d = plan_chain(config({"offset": 0.0, "decimation": 4, "taps": 33, "cutoff": None, "beta": 5}))
    assert (d.ddc["taps"], d.ddc["cutoff"], d.ddc["beta"], d.fs, d.n) == (33, 0.8, 5.0, FS // 4, N // 4)
    p = plan_chain(config(det={"nCentroid": 6, "clean": {"snr": 18}}), **USRP)
    assert p.clean == {"snr": 18.0, "echoes": 4, "sideDelay": 1, "sideDoppler": 0, "loading": 1e-6}
    assert (p.centroid, p.detect, p.usrp_block) == (6, "device", 363)
    assert plan_chain(config(det={"nCentroid": 6}), detect="host").detect == "host"
    assert plan_chain(config(det={"clutterMap": {"memory": 8}})).cmap == (8, "gate")
    assert plan_chain(config(det={"clutterMap": {"memory": 64, "mode": "Detect"}})).cmap == (64, "detect")
    assert plan_chain(config(amb={"window": "Hann:norm"})).taper == ("hann", True)
    assert plan_chain(config(amb={"window": "none"})).taper is None
    assert plan_chain(config(integrate={"window": 3})).integrate == (3, 1)
    assert plan_chain(config(integrate={"window": 4, "hop": 2})).integrate == (4, 2)


def test_absent_none_and_false_are_one_plan():
    plain = plan_chain(config())
    for off in (None, False):
        assert plan_chain(config(off)) == plain
        for key in ("window", "migration", "dopplerRate"):
            assert plan_chain(config(amb={key: off})) == plain
        for key in ("clutterMap", "clean"):
            assert plan_chain(config(det={key: off})) == plain
        assert plan_chain(config(integrate=off)) == plain
        summed = plan_chain(config(integrate={"window": 2, "hop": 1}))
        assert plan_chain(config(integrate={"window": 2, "hop": 1, "tracks": off})) == summed
        assert plan_chain(config(integrate={"window": 2, "tracks": {"fc": FC, "rate": off}})).tracks == (FC, None)


def test_pfa_over_the_hypotheses_and_carriers_behind_a_down_converter():
    p = plan_chain(config(amb={"dopplerRate": {"max": 2, "step": 1}}))
    assert np.array_equal(p.rates, [-2.0, -1.0, 0.0, 1.0, 2.0]) and p.pfa == PFA / 5
    assert np.array_equal(plan_chain(config(amb={"dopplerRate": 1.5})).rates, [-1.0, 0.0, 1.0])
    p = plan_chain(config(amb={"dopplerRate": 2}, integrate={"window": 3, "tracks": {"fc": FC, "rate": {"max": 1, "step": 1}}}))
    assert np.array_equal(p.tracks[1], [-1.0, 0.0, 1.0]) and p.pfa == (PFA / 5) / 3
    assert plan_chain(config(integrate={"window": 3, "tracks": {"fc": FC}})).pfa == PFA  # the walk only: one hypothesis
    dd = {"offset": 16384.0, "decimation": 4}
    p = plan_chain(config(dd, amb={"migration": {"fc": FC}}, integrate={"window": 2, "tracks": {"fc": 1.0e8}}))
    assert (p.migrate_fc, p.tracks[0]) == (FC + 16384.0, 1.0e8 + 16384.0)
    with pytest.raises(ValueError, match="ambiguity.migration"):  # fc + offset = 0
        plan_chain(config({"offset": -16384.0, "decimation": 4}, amb={"migration": {"fc": 16384.0}}))


def test_clean_and_the_fused_filter():
    clu = {"enable": True, "delayMin": -4, "delayMax": 20}
    assert plan_chain(config(clutter=clu)).clutter == {"enable": True, "blocks": 1, "fused": True}
    assert plan_chain(config(clutter=dict(clu, fused=False, blocks=4))).clutter == {"enable": True, "blocks": 4, "fused": False}
    p = plan_chain(config(clutter=clu, det={"nCentroid": 6, "clean": {"snr": 18, "echoes": 2}}))  # the filter's output is the plane
    assert p.clutter["fused"] is False and p.clean["echoes"] == 2
    assert plan_chain(config({"offset": 0.0, "decimation": 4}, det={"nCentroid": 6, "clean": {"snr": 18}})).clean is not None


def test_needs_order_and_fmt_in():
    dd = {"offset": 0.0, "decimation": 4}
    assert not plan_chain(config()).needs_order and not plan_chain(config(integrate={"window": 2})).needs_order
    assert plan_chain(config(det={"clutterMap": {"memory": 4}})).needs_order and plan_chain(config(dd)).needs_order
    for kw, fmt in (({}, _lib.FMT_I16), ({"layout": "cs8"}, _lib.FMT_I8), (USRP, _lib.FMT_C32)):
        assert plan_chain(config(), **kw).fmt_in == fmt
        assert plan_chain(config(dd), **kw).fmt_in == _lib.FMT_C32


# ---- the command line --------------------------------------------------------------------------------------------------
def stub(batch):
    return [{"noisePower": 0.0, "maxPower": float(np.asarray(c).max())} for c in batch]


class _StubChain:
    def __call__(self, batch):
        return stub(batch)

    def close(self):
        pass


@pytest.fixture
def stub_chain(monkeypatch):
    made = {}

    def fake(cfg, device=0, batch=1, want_map=False, **kw):
        made.update(kw, cfg=cfg, batch=batch, chain=_StubChain())
        return made["chain"]
    monkeypatch.setattr(R, "gpu_processor", fake)
    return made


CLI_FS, CLI_N = 4096, 1024


@pytest.fixture
def files(tmp_path):
    """A two-CPI .rspduo capture and a writer of its config: capture.fc or none, detection and the filter on or off."""
    cap = str(tmp_path / "cap.rspduo")
    np.random.default_rng(5).integers(-2000, 2000, size=(2 * CLI_N, 4), dtype=np.int16).tofile(cap)

    def write(fc=FC, detection=False, device="RspDuo", **det):
        capture = {"fs": CLI_FS, "device": {"type": device}}
        if fc is not None:
            capture["fc"] = fc
        detection = dict(DET, nCentroid=6, **det) if detection or det else {"enable": False}
        yaml.safe_dump({"capture": capture,
                        "process": {"data": {"cpi": CLI_N / CLI_FS},
                                    "ambiguity": {"delayMin": -4, "delayMax": 20, "dopplerMin": -64, "dopplerMax": 64},
                                    "clutter": {"enable": bool(detection.get("enable")), "delayMin": -4, "delayMax": 20},
                                    "detection": detection}}, open(str(tmp_path / "config.yml"), "w"))
        return [cap, "--config", str(tmp_path / "config.yml")]
    return write


BAD_ARGV = (
    [({}, ["--ddc"] + v) for v in (["16384"], ["x:4"], ["16384:4.5"], ["16384:4:64:0.8:8:1"], [])] +
    [({}, v) for v in (["--clutter-map", "0"], ["--clutter-map", "65"], ["--clutter-map", "eight"], ["--clutter-map", "8:censor"],
                       ["--clutter-map", "8:detect:1"], ["--integrate", "3", "--clutter-map", "8"], ["--clutter-map"])] +
    [({"device": "Usrp"}, ["--format", "usrp", "--usrp-block", "363"] + v)
     for v in (["--clean", "loud"], ["--clean", "18:0"], ["--clean", "18:33"], ["--clean", "18:4:1"], ["--clean"],
               ["--integrate", "3", "--clean", "18"], ["--clutter-map", "8", "--clean", "18"])] +
    [({}, ["--doppler-rate", v]) for v in ("8", "2:0", "-1", "fast", "1:1:1", "nan")] +
    [({"fc": None}, ["--migration"])] + [({"fc": None}, ["--migration", v]) for v in ("-5", "nan", "carrier")] +
    [({}, v) for v in (["--integrate-tracks"], ["--integrate-tracks", "1"], ["--integrate", "3", "--integrate-tracks", "8"],
                       ["--integrate", "3", "--integrate-tracks", "2:0"], ["--integrate", "3", "--integrate-tracks", "-1"],
                       ["--integrate", "3", "--integrate-tracks", "fast"], ["--integrate", "3", "--integrate-tracks", "1:1:1"])] +
    [({"fc": None}, ["--integrate", "3", "--integrate-tracks", "1"])] +  # no carrier anywhere
    [({"detection": True}, ["--cfar", v]) for v in ("so", "ca:0.5", "os:0", "os:1.5", "os:x")] +
    [({}, ["--doppler-window", v]) for v in ("taylor", "hann:peak")] +
    [({}, ["--integrate", v]) for v in ("0", "3:0", "x", "3:1:1")] + [({}, ["--clutter-blocks", "0"])])


@pytest.mark.parametrize("yml,argv", BAD_ARGV, ids=[" ".join(v) or "-" for _, v in BAD_ARGV])
def test_bad_arguments_exit_before_a_chain_is_made(files, stub_chain, capsys, yml, argv):
    with pytest.raises(SystemExit) as e:
        R.main(files(**yml) + argv)
    assert e.value.code != 0 and "chain" not in stub_chain
    capsys.readouterr()


GOOD_ARGV = [
    (["--ddc", "1024:4:64"], lambda c: c["ddc"], {"offset": 1024.0, "decimation": 4, "taps": 64}),
    (["--ddc=-512:2:32:0.7:6"], lambda c: c["ddc"], {"offset": -512.0, "decimation": 2, "taps": 32, "cutoff": 0.7, "beta": 6.0}),
    (["--clutter-blocks", "2"], lambda c: c["clutter"]["blocks"], 2),
    (["--integrate", "3"], lambda c: c["integrate"], {"window": 3, "hop": 1}),
    (["--integrate", "4:2"], lambda c: c["integrate"], {"window": 4, "hop": 2}),
    (["--integrate", "3", "--integrate-tracks"], lambda c: c["integrate"]["tracks"], {"fc": FC}),
    (["--integrate", "3", "--integrate-tracks", "1:0.5"], lambda c: c["integrate"]["tracks"], {"fc": FC, "rate": {"max": 1.0, "step": 0.5}}),
    (["--doppler-window", "HANN:norm"], lambda c: c["ambiguity"]["window"], "hann:norm"),
    (["--migration"], lambda c: c["ambiguity"]["migration"], {"fc": FC}),
    (["--migration", "9e7"], lambda c: c["ambiguity"]["migration"], {"fc": 9e7}),
    (["--doppler-rate", "2"], lambda c: c["ambiguity"]["dopplerRate"], {"max": 2.0, "step": 1.0}),
    (["--doppler-rate", "2:0.5"], lambda c: c["ambiguity"]["dopplerRate"], {"max": 2.0, "step": 0.5}),
    (["--cfar", "os:0.5"], lambda c: (c["detection"]["cfar"], c["detection"]["rank"]), ("os", 0.5)),
    (["--cfar", "ca"], lambda c: (c["detection"]["cfar"], "rank" in c["detection"]), ("ca", False)),
    (["--clutter-map", "8"], lambda c: c["detection"]["clutterMap"], {"memory": 8, "mode": "gate"}),
    (["--clutter-map", "8:detect"], lambda c: c["detection"]["clutterMap"], {"memory": 8, "mode": "detect"}),
    (["--clean", "18"], lambda c: c["detection"]["clean"], {"snr": 18.0, "echoes": 4}),
    (["--clean", "18.5:3"], lambda c: c["detection"]["clean"], {"snr": 18.5, "echoes": 3}),
]


@pytest.mark.parametrize("argv,pick,want", GOOD_ARGV, ids=[" ".join(v) for v, _, _ in GOOD_ARGV])
def test_a_flag_hands_the_chain_its_key(files, stub_chain, capsys, argv, pick, want):
    R.main(files(detection=True) + ["--batch", "1"] + argv)
    assert pick(stub_chain["cfg"]) == want and stub_chain["layout"] == "rspduo" and stub_chain["batch"] == 1
    assert [json.loads(s)["cpi"] for s in capsys.readouterr().out.strip().split("\n")] == [0, 1]
    plan_chain(stub_chain["cfg"])  # what the chain gets is a config the plan takes


def test_a_bad_value_in_the_config_exits_before_a_chain_is_made(files, stub_chain, capsys):
    with pytest.raises(SystemExit) as e:
        R.main(files(clutterMap={"memory": 0}))
    assert e.value.code != 0 and "chain" not in stub_chain and "detection.clutterMap" in capsys.readouterr().err
    R.main(files(clean={"snr": 18, "echoes": 8}) + ["--clean", "20"])  # the flag overrides snr and echoes, the rest stays
    assert stub_chain["cfg"]["detection"]["clean"] == {"snr": 20.0, "echoes": 4}
    capsys.readouterr()


def test_order_bound_stages_take_one_rank(files, stub_chain, capsys, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    for argv in (["--ddc", "1024:4"], ["--clutter-map", "8"]):
        with pytest.raises(SystemExit):
            R.main(files(detection=True) + argv)
        assert "one rank" in capsys.readouterr().err and "chain" not in stub_chain
