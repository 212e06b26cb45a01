"""CPU, no library: the replay key ``detection.cfar: goca | soca`` in ``blah2_amd.chain_plan.plan_chain`` and ``--cfar goca`` /
``--cfar soca`` on the command line of ``blah2_amd.replay``: the plan carries the kind, everything else of the plan is the
averaging detector's; ``integrate`` and several carriers (more than one look per cell) are refused with the key's name; a
rank suffix is an error; the spellings ``go`` and ``so`` stay refused."""
import json

import pytest

from blah2_amd import replay as R
from blah2_amd.chain_plan import plan_chain
from test_chain_plan import FC, PFA, config, files, no_library, stub_chain  # noqa: F401  (fixtures)


@pytest.mark.parametrize("kind", ["goca", "soca", "GOCA", "SoCa"])
def test_the_plan_carries_the_kind(kind):
    p, ca = plan_chain(config(det={"cfar": kind})), plan_chain(config(det={"cfar": "ca"}))
    assert p.cfar_kind == kind.lower()
    assert {k: v for k, v in vars(p).items() if k != "cfar_kind"} == {k: v for k, v in vars(ca).items() if k != "cfar_kind"}
    assert plan_chain(config(det={"cfar": kind, "enable": False})).cfar_kind is None


def test_what_works_behind_the_detector_is_unchanged():
    p = plan_chain(config(det={"cfar": "goca", "nCentroid": 6, "clutterMap": {"memory": 8}}, amb={"dopplerRate": {"max": 2, "step": 1}}))
    assert (p.cfar_kind, p.pfa, p.cmap, p.centroid, p.detect) == ("goca", PFA / 5, (8, "gate"), 6, "device")
    p = plan_chain(config({"offset": 16384.0, "decimation": 4}, det={"cfar": "soca", "clean": {"snr": 18}, "nCentroid": 6}))
    assert p.cfar_kind == "soca" and p.clean is not None and p.carriers is None


@pytest.mark.parametrize("kind", ["goca", "soca"])
def test_more_than_one_look_is_refused_by_name(kind):
    with pytest.raises(ValueError, match="detection.cfar"):
        plan_chain(config(det={"cfar": kind}, integrate={"window": 3}))
    with pytest.raises(ValueError, match="detection.cfar"):
        plan_chain(config(det={"cfar": kind}, integrate={"window": 3, "tracks": {"fc": FC}}))
    with pytest.raises(ValueError, match="detection.cfar"):
        plan_chain(config({"offset": [0.0, 16384.0], "decimation": 4}, det={"cfar": kind}, fc=FC))
    assert plan_chain(config({"offset": [0.0, 16384.0], "decimation": 4}, det={"cfar": "ca"}, fc=FC)).carriers is not None
    assert plan_chain(config({"offset": [16384.0], "decimation": 4}, det={"cfar": kind}, fc=FC)).cfar_kind == kind  # one carrier


@pytest.mark.parametrize("bad", ["go", "so", "goca:0.5", "gosoca", ""])
def test_other_spellings_stay_refused(bad):
    with pytest.raises(ValueError, match="detection.cfar"):
        plan_chain(config(det={"cfar": bad}))


@pytest.mark.parametrize("kind", ["goca", "soca"])
def test_the_flag_hands_the_chain_its_key(files, stub_chain, capsys, kind):
    R.main(files(detection=True) + ["--batch", "1", "--cfar", kind])
    det = stub_chain["cfg"]["detection"]
    assert det["cfar"] == kind and "rank" not in det
    assert [json.loads(s)["cpi"] for s in capsys.readouterr().out.strip().split("\n")] == [0, 1]
    assert plan_chain(stub_chain["cfg"]).cfar_kind == kind
    R.main(files(detection=True, cfar="os") + ["--batch", "1", "--cfar", kind])  # the flag overrides the config's key
    assert stub_chain["cfg"]["detection"]["cfar"] == kind
    capsys.readouterr()


@pytest.mark.parametrize("argv", [["--cfar", "goca:0.5"], ["--cfar", "soca:0.75"], ["--cfar", "go"], ["--cfar", "so"],
                                  ["--cfar", "goca", "--integrate", "3"], ["--integrate", "2:1", "--cfar", "soca"]],
                         ids=" ".join)
def test_bad_arguments_exit_before_a_chain_is_made(files, stub_chain, capsys, argv):
    with pytest.raises(SystemExit) as e:
        R.main(files(detection=True) + argv)
    assert e.value.code != 0 and "chain" not in stub_chain
    err = capsys.readouterr().err
    assert "--cfar" in err or "detection.cfar" in err


def test_the_config_key_reaches_the_plan_through_main(files, stub_chain, capsys):
    R.main(files(detection=True, cfar="soca") + ["--batch", "1"])
    assert plan_chain(stub_chain["cfg"]).cfar_kind == "soca"
    capsys.readouterr()
    with pytest.raises(SystemExit):
        R.main(files(detection=True, cfar="goca") + ["--integrate", "3"])
    assert "detection.cfar" in capsys.readouterr().err
