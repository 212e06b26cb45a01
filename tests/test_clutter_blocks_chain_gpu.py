"""GPU: the clutter filter with taps per block in front of the ambiguity engine -- WienerHopf(blocks=4) followed by
Ambiguity on small_sym's geometry, two CPIs in one batch -- against the oracle map of the restatement's filtered channel
(tests/clutter_blocks_ref.py), with the chain's gates (tests/test_full_chain_gpu.py: every cell above the mean level outside
the cancelled notch to 1e-4, the dB map gate, the error against the uncancelled direct-path level to 1e-4).  The fused FIR
takes one tap set per CPI: fir_fusable gives a reason, set_fir raises, and a GpuChain configured with clutter: {blocks: 4}
runs the two-stage chain and gives the same maps."""
import numpy as np
import pytest

import clutter_blocks_ref as R
import test_full_chain_gpu as fc
from conftest import load_golden
from oracle import blah2_oracle as O

pytestmark = pytest.mark.gpu
BLOCKS = 4


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


@pytest.fixture(scope="module")
def scene():
    """small_sym's geometry; two different int16-valued CPIs; per CPI the restatement's filter and the oracle's map of it."""
    g = load_golden("small_sym")
    fs, n, dmin, dmax, fmin, fmax, rh = (int(v) for v in g["params"])
    cmin, cmax = (int(v) for v in g["clutter_params"])
    assert n % BLOCKS == 0
    d = O.ambiguity_dims(dmin, dmax, fmin, fmax, fs, n, bool(rh))
    cpis = []
    for c in range(2):
        x, y = O.synth_iq(n, seed=910 + c, fs=fs, targets=((7, -40.0, 0.05), (cmin + 2, 0.0, 0.3), (12, 0.0, 0.2)))
        ok, y_ref, _, _, b_ref = R.wiener_hopf_blocks(x, y, cmin, cmax, BLOCKS)
        assert ok.all()
        m_ref = O.ambiguity_process(d, x, y_ref)
        noise_ref, max_ref = O.map_metrics(m_ref)
        direct = sum(np.max(np.abs(b)) for b in b_ref) * (d.n_corr * d.n_doppler_bins / n)
        cpis.append(dict(x=x, y=y, m_ref=m_ref, noise=noise_ref, max=max_ref, direct=direct))
    iq = np.stack([np.stack([c["x"].real, c["x"].imag, c["y"].real, c["y"].imag], axis=-1) for c in cpis]).astype(np.int16)
    return dict(geom=(dmin, dmax, fmin, fmax, fs, n, bool(rh)), clutter=(cmin, cmax), d=d, cpis=cpis, iq=iq)


def check_maps(tag, scene, maps, noises):
    d, (cmin, cmax) = scene["d"], scene["clutter"]
    for c, ref in enumerate(scene["cpis"]):
        fc.check_chain_map(f"{tag} cpi {c}", np.asarray(maps[c], dtype=np.complex128), noises[c], ref["m_ref"], ref["noise"],
                           ref["direct"], d.doppler, d.delay, cmin, cmax)
        assert abs(noises[c] - ref["noise"]) <= 1e-3, (tag, c, noises[c], ref["noise"])


def direct_chain(b2, scene):
    """The two-stage chain through the Python mirror, on the .rspduo words: (maps [2, nD, nC], metrics [2, 2], wh, amb)."""
    import torch
    (cmin, cmax), n = scene["clutter"], scene["geom"][5]
    wh = b2.WienerHopf(cmin, cmax, n, max_batch=2, blocks=BLOCKS)
    amb = b2.Ambiguity(*scene["geom"], max_batch=2)
    iq = torch.from_numpy(scene["iq"]).cuda()
    yf = torch.empty((2, n), dtype=torch.complex64, device="cuda")
    ok = torch.zeros(2 * BLOCKS, dtype=torch.int32, device="cuda")
    maps = torch.zeros((2, amb.get_n_doppler_bins(), amb.get_n_delay_bins()), dtype=torch.complex64, device="cuda")
    met = torch.zeros((2, 2), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    wh.process_dev_fmt(b2.FMT_I16, iq.data_ptr(), None, 2, n, yf.data_ptr(), n, ok.data_ptr(), st)
    amb.process_dev(b2.FMT_I16X_C32Y, iq.data_ptr(), yf.data_ptr(), 2, n, maps.data_ptr(), met.data_ptr(), st)
    torch.cuda.synchronize()
    assert ok.cpu().numpy().all()
    return maps.cpu().numpy(), met.cpu().numpy(), wh, amb


def test_blocks_then_ambiguity(b2, scene):
    maps, met, wh, amb = direct_chain(b2, scene)
    check_maps("blocks chain", scene, maps, met[:, 0])
    # the fused FIR has one tap set per CPI
    reason = amb.fir_fusable(wh, b2.FMT_I16)
    assert reason and "blocks" in reason
    with pytest.raises(ValueError):
        amb.set_fir(wh)
    one = b2.WienerHopf(*scene["clutter"], scene["geom"][5], max_batch=2)  # without blocks the question goes to the library
    assert amb.fir_fusable(one, b2.FMT_I16) != reason


def test_gpu_chain_with_blocks(b2, scene):
    from blah2_amd import replay
    dmin, dmax, fmin, fmax, fs, n, _ = scene["geom"]
    cmin, cmax = scene["clutter"]
    cfg = {"fs": fs, "n_samples": n,
           "ambiguity": {"delayMin": dmin, "delayMax": dmax, "dopplerMin": fmin, "dopplerMax": fmax},
           "clutter": {"enable": True, "delayMin": cmin, "delayMax": cmax, "blocks": BLOCKS}}
    chain = replay.GpuChain(cfg, 0, batch=2, want_map=True)
    try:
        assert chain.clutter_blocks == BLOCKS and not chain.fused_fir and chain.wh.blocks == BLOCKS
        res = chain(scene["iq"])
    finally:
        chain.close()
    assert len(res) == 2 and not any(r.get("skipped") for r in res)
    maps = [r["map"] for r in res]
    check_maps("GpuChain blocks", scene, maps, [r["noisePower"] for r in res])
    direct, _, _, _ = direct_chain(b2, scene)
    for c in range(2):
        assert np.array_equal(maps[c], direct[c]), f"cpi {c}: the chain's map differs from the mirror's two-stage chain"
