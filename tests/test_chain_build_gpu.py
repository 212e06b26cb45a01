"""GPU: a GpuChain whose build fails after handles exist closes every one of them, once, last first, and the ValueError
names the key.  Geometry of ddc_scenes.py (fs 65 536 Hz, a one-second CPI), batch 1; nothing is replayed.

  * ``ambiguity.dopplerRate`` beyond the Doppler bins: ``set_rates`` refuses it when only the ambiguity handle exists;
  * ``integrate.tracks`` at a 1 Hz carrier (a walk beyond BLAH2HIP_MAX_TRACK_SHIFT): refused when the ambiguity handle, the
    filter and the integrator exist.

No dictionary passes :func:`blah2_amd.chain_plan.plan_chain` and is then refused by ``Channelizer``: the plan already holds
every check of blah2hip_ddc_create that the config decides (decimation, taps, finite taps, the offset against fs / 2, a CPI
that the decimation divides); what is left there depends on the batch and the device, not on the dictionary.
"""
import pytest

import ddc_scenes as S

pytestmark = pytest.mark.gpu

N_DOPPLER = 129


def config(**extra):
    cfg = {"fs": S.FS, "n_samples": S.N, "ambiguity": {"delayMin": -4, "delayMax": 20, "dopplerMin": -64, "dopplerMax": 64},
           "clutter": {"enable": True, "delayMin": -4, "delayMax": 20}, "integrate": {"window": 2, "hop": 1},
           "detection": {"enable": True, "pfa": 1e-5, "nGuard": 2, "nTrain": 6, "minDelay": 0, "minDoppler": 5.0}}
    for k, v in extra.items():
        cfg[k] = dict(cfg[k], **v)
    return cfg


@pytest.mark.parametrize("key,extra,made_want", [
    ("ambiguity.dopplerRate", {"ambiguity": {"dopplerRate": {"max": 10 * N_DOPPLER, "step": 5.0 * N_DOPPLER}}}, {"Ambiguity": 1}),
    ("integrate.tracks", {"integrate": {"tracks": {"fc": 1.0}}}, {"Ambiguity": 1, "WienerHopf": 1, "MapIntegrator": 1}),
])
def test_a_build_that_fails_late_closes_what_it_made(built_lib, monkeypatch, key, extra, made_want):
    import blah2_amd as b2
    from blah2_amd import replay as R
    from blah2_amd.chain_plan import plan_chain
    made, closes, order = {}, {}, []

    def watch(cls):
        init, close = cls.__init__, cls.close

        def init_(self, *a, **kw):
            init(self, *a, **kw)
            made[id(self)] = cls.__name__  # (only a handle that came to exist)

        def close_(self):
            if getattr(self, "_h", None):  # a close of a live handle (the later ones, __del__'s among them, do nothing)
                closes[id(self)] = closes.get(id(self), 0) + 1
                order.append(cls.__name__)
            close(self)
        monkeypatch.setattr(cls, "__init__", init_)
        monkeypatch.setattr(cls, "close", close_)

    for cls in (b2.Ambiguity, b2.WienerHopf, b2.MapIntegrator):
        watch(cls)
    cfg = config(**extra)
    plan_chain(cfg, batch=1)  # the dictionary alone is in order: the refusal needs a handle
    with pytest.raises(ValueError, match=key):
        R.GpuChain(cfg, 0, batch=1)
    count = {}
    for name in made.values():
        count[name] = count.get(name, 0) + 1
    print(key, "made", count, "closed", order)
    assert count == made_want
    assert closes == {i: 1 for i in made}
    assert order == [n for n in ("MapIntegrator", "WienerHopf", "Ambiguity") if n in made_want]  # last made, first closed
