"""GPU: USRP captures through the HIP engine -- blah2hip_deblock_c32_dev against the NumPy de-block (bit for bit), and
GpuChain's USRP layout (de-block, then the FMT_C32 chain) against the compiled-reference fixtures, the .rspduo replay of
the same samples, a power-of-two rescaling and the fp64 oracle at the configs[1] geometry."""
import os

import numpy as np
import pytest

from conftest import load_golden
from test_replay_gpu import medium_cfg
from test_usrp_capture import write_usrp

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no copy produces


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


def iq_to_xy(iq):
    """A .rspduo CPI's int16 samples as the fp32 values a USRP capture would hold."""
    iq = iq.astype(np.float32)
    return (iq[:, 0] + 1j * iq[:, 1]).astype(np.complex64), (iq[:, 2] + 1j * iq[:, 3]).astype(np.complex64)


def write_cpis(path, cpis, block, scale=1.0):
    """CPIs of int16 samples [n, 4], end to end, as a USRP capture of ``block``."""
    xs, ys = zip(*(iq_to_xy(c) for c in cpis))
    x, y = np.concatenate(xs), np.concatenate(ys)
    if scale != 1.0:
        x, y = (x * np.float32(scale)).astype(np.complex64), (y * np.float32(scale)).astype(np.complex64)
    write_usrp(path, x, y, block)


# (block, first, n, n_cpi, cpi_stride, plane offset in samples): odd and even B, B > n, first mid-block, the 16-byte
# path (B, first, n, stride even and aligned planes) and the 8-byte one
KERNEL_CASES = [
    (2040, 1000, 1000, 3, 1024, 0),   # 16-byte path, B > n
    (2040, 6, 1000, 2, 1001, 0),      # even B, odd stride: 8-byte path
    (2040, 6, 1000, 2, 1002, 1),      # even everything, planes 8-byte aligned only: 8-byte path
    (363, 100, 1000, 5, 1001, 0),     # odd B
    (7, 3, 999, 2, 1003, 0),
    (1, 0, 1000, 1, 1000, 0),
    (2048, 2046, 4096, 4, 4100, 0),   # 16-byte path, a CPI spans blocks
    (5001, 4999, 777, 5, 800, 0),     # odd B > n, first at a block's last sample
    (2040, 200_000, 190_647, 2, 190_700, 0),  # first several blocks in
]


@pytest.mark.parametrize("block,first,n,n_cpi,stride,pad", KERNEL_CASES)
def test_deblock_kernel_is_an_exact_copy(b2, block, first, n, n_cpi, stride, pad):
    import torch
    from blah2_amd import replay as R
    rng = np.random.default_rng(block + first + n)
    pairs = (first + n_cpi * n - 1) // block + 1  # every block pair a sample of the batch lies in
    raw = (rng.standard_normal(2 * pairs * block) + 1j * rng.standard_normal(2 * pairs * block)).astype(np.complex64)
    raw.view(np.uint32)[::97] = 0x80000000  # some negative zeros: a copy, not arithmetic
    want = R.usrp_deblock(raw, block, first, n, n_cpi)
    rows = max(stride, n)
    d_raw = torch.from_numpy(raw).cuda()
    guard64 = int(np.array([GUARD, GUARD], dtype=np.uint32).view(np.int64)[0])  # one complex value of guard
    d_x = torch.full((n_cpi * rows + pad,), guard64, dtype=torch.int64, device="cuda")
    d_y = d_x.clone()
    px, py = d_x.data_ptr() + 8 * pad, d_y.data_ptr() + 8 * pad
    b2.deblock_c32_dev(d_raw.data_ptr(), block, first, n, n_cpi, px, py, stride, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for c, d in ((0, d_x), (1, d_y)):
        got = d.cpu().numpy().view(np.uint32).reshape(-1, 2)  # one row per complex value
        assert np.all(got[:pad] == GUARD)
        got = got[pad:].reshape(n_cpi, rows, 2)
        assert np.array_equal(got[:, :n].reshape(n_cpi, n * 2), want[:, c].view(np.uint32).reshape(n_cpi, n * 2)), c
        assert np.all(got[:, n:] == GUARD)  # nothing beyond a row's n samples


def test_deblock_kernel_rejects_bad_arguments(b2):
    import torch
    raw = torch.zeros(4096, dtype=torch.complex64, device="cuda")
    planes = torch.full((2, 2, 512), 7.0, dtype=torch.complex64, device="cuda")
    r, x, y = raw.data_ptr(), planes[0].data_ptr(), planes[1].data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    bad = [(r, 0, 0, 512, 2, x, y, 512),        # block 0
           (None, 64, 0, 512, 2, x, y, 512),    # NULL raw
           (r, 64, 0, 512, 2, None, y, 512),    # NULL x
           (r, 64, 0, 512, 2, x, None, 512),    # NULL y
           (r, 64, 0, 0, 2, x, y, 512),         # n_samples 0
           (r, 64, 0, 512, 2, x, y, 511)]       # rows would overlap
    for args in bad:
        with pytest.raises(b2.Blah2HipError) as e:
            b2.deblock_c32_dev(*args, st)
        assert e.value.code == b2._lib.ERR_INVALID, args
    b2.deblock_c32_dev(r, 64, 0, 512, 0, x, y, 0, st)  # no CPIs: nothing to do
    torch.cuda.synchronize()
    assert torch.all(planes == 7.0)  # nothing was enqueued
    b2.deblock_c32_dev(r, 64, 0, 512, 1, x, y, 0, st)  # one CPI: the stride does not matter
    torch.cuda.synchronize()
    assert torch.all(planes[:, 0] == 0) and torch.all(planes[:, 1] == 7.0)


def fixture_capture(g, block, path, scale=1.0):
    write_cpis(path, [g["iq"], -g["iq"], g["iq"]], block, scale)


def clutter_cfg(g):
    cfg = medium_cfg(g)
    cfg["clutter"] = {"enable": True, "delayMin": int(g["clutter_params"][0]), "delayMax": int(g["clutter_params"][1])}
    return cfg


def replay_usrp(path, n, block, cfg, read_mode="memmove", batch=2):
    from blah2_amd import replay as R
    cap = R.UsrpFile(path, n, block)
    chain = R.GpuChain(cfg, 0, batch=batch, reader_threads=3, read_mode=read_mode, layout="usrp", usrp_block=block)
    try:
        res = R.replay(cap, chain, batch=batch)
        assert chain.read_mode == read_mode  # mapped: /dev/shm pages register, no fall-back
        return res, chain
    finally:
        chain.close()
        cap.close()


@pytest.mark.parametrize("block", [2040, 363])
def test_usrp_replay_matches_the_compiled_reference(b2, block):
    """The medium fixture as a USRP capture (g, -g, g), batch 2 (a ragged last batch), every read path, without and with
    the clutter filter: the compiled reference's metrics and detections."""
    g = load_golden("medium")
    n = int(g["params"][1])
    path = f"/dev/shm/blah2_test_usrp_{os.getpid()}_{block}.usrp.iq"
    fixture_capture(g, block, path)
    try:
        for mode in ("memmove", "pread", "mapped"):
            res, _ = replay_usrp(path, n, block, medium_cfg(g), mode)
            assert [r["cpi"] for r in res] == [0, 1, 2]
            for r in res:
                assert abs(r["noisePower"] - g["metrics"][0]) < 1e-3
                assert abs(r["maxPower"] - g["metrics"][1]) < 1e-3
                assert r["delay"] == g["cfar"][0].tolist() and r["doppler"] == g["cfar"][1].tolist()
                assert np.allclose(r["snr"], g["cfar"][2], rtol=0, atol=1e-3)
            res, _ = replay_usrp(path, n, block, clutter_cfg(g), mode)
            assert [r["cpi"] for r in res] == [0, 1, 2]
            for r in res:
                assert not r.get("skipped")
                assert abs(r["noisePower"] - g["chain_metrics"][0]) < 1e-3
                assert set(zip(r["delay"], r["doppler"])) == set(zip(g["chain_cfar"][0], g["chain_cfar"][1]))
    finally:
        os.remove(path)


def test_usrp_replay_skips_cpis_whose_clutter_filter_fails(b2, tmp_path):
    """blah2.cpp:270-273 on a USRP capture: an all-zero reference channel in CPI 1 drops that CPI only."""
    g = load_golden("medium")
    n = int(g["params"][1])
    dead = g["iq"].copy()
    dead[:, 0:2] = 0
    path = str(tmp_path / "cap.usrp.iq")
    write_cpis(path, [g["iq"], dead, g["iq"]], 2040)
    res, _ = replay_usrp(path, n, 2040, clutter_cfg(g), batch=3)
    assert [bool(r.get("skipped")) for r in res] == [False, True, False]
    assert abs(res[0]["noisePower"] - g["chain_metrics"][0]) < 1e-3 and abs(res[2]["noisePower"] - g["chain_metrics"][0]) < 1e-3


def test_usrp_chain_refuses_the_other_layout(b2, tmp_path):
    from blah2_amd import replay as R
    g = load_golden("medium")
    n = int(g["params"][1])
    p_usrp, p_rsp = str(tmp_path / "a.usrp.iq"), str(tmp_path / "a.rspduo")
    write_cpis(p_usrp, [g["iq"]], 2040)
    g["iq"].tofile(p_rsp)
    chain = R.GpuChain(medium_cfg(g), 0, batch=1, layout="usrp", usrp_block=2040)
    with pytest.raises(ValueError):
        R.replay(R.RspduoFile(p_rsp, n), chain)
    with pytest.raises(ValueError):
        R.replay(R.UsrpFile(p_usrp, n, 363), chain)
    with pytest.raises(ValueError):
        chain(g["iq"][None])
    chain.close()
    chain = R.GpuChain(medium_cfg(g), 0, batch=1)
    with pytest.raises(ValueError):
        R.replay(R.UsrpFile(p_usrp, n, 2040), chain)
    chain.close()


def test_usrp_replay_runs_the_fused_fir_where_it_is_covered(b2, tmp_path):
    """The geometry of test_replay_gpu's fused test (31 pulses of 6149 samples, 2047 taps) from a USRP capture: the fused
    range kernel on the de-blocked planes, clutter: {fused: false} the two-stage chain; both agree with each other and
    with the .rspduo replay of the same samples."""
    from blah2_amd import replay as R
    from test_fused_fir_gpu import synth
    n = 190_647
    x, y = synth(n, n, 77)
    iq = np.stack([x.real, x.imag, y.real, y.imag], axis=-1).astype(np.int16)
    dead = iq.copy()
    dead[:, 0:2] = 0
    p_usrp, p_rsp = str(tmp_path / "cap.usrp.iq"), str(tmp_path / "cap.rspduo")
    write_cpis(p_usrp, [iq, dead, iq], 2040)
    np.concatenate([iq, dead, iq]).tofile(p_rsp)
    cfg = {"fs": n, "n_samples": n,
           "ambiguity": {"delayMin": -24, "delayMax": 2023, "dopplerMin": -15, "dopplerMax": 15},
           "detection": {"enable": True, "pfa": 1e-5, "nGuard": 2, "nTrain": 6, "minDelay": 5, "minDoppler": 1.0},
           "clutter": {"enable": True, "delayMin": -24, "delayMax": 2023}}
    out = {}
    for fused in (True, False):
        cfg["clutter"]["fused"] = fused
        res, chain = replay_usrp(p_usrp, n, 2040, cfg)
        assert chain.fused_fir == fused
        assert chain.amb.info(b2._lib.INFO_LAST_RANGE_KERNEL) == (b2._lib.RANGE_FIR if fused else b2._lib.RANGE_E16)
        assert [bool(r.get("skipped")) for r in res] == [False, True, False]
        out[fused] = res
        rsp = R.replay(R.RspduoFile(p_rsp, n), R.gpu_processor(cfg, 0, batch=2), batch=2)
        out[("rspduo", fused)] = rsp
    for other in (out[False], out[("rspduo", True)], out[("rspduo", False)]):
        for a, b in zip(out[True], other):
            assert bool(a.get("skipped")) == bool(b.get("skipped"))
            if a.get("skipped"):
                continue
            assert abs(a["noisePower"] - b["noisePower"]) < 1e-4 and abs(a["maxPower"] - b["maxPower"]) < 1e-4
            assert list(zip(a["delay"], a["doppler"])) == list(zip(b["delay"], b["doppler"])) and len(a["delay"]) >= 1
            assert np.allclose(a["snr"], b["snr"], rtol=0, atol=1e-3)


def test_usrp_replay_of_fc32_sized_values(b2, tmp_path):
    """UHD's fc32 samples are about int16 / 32767: the fixture capture times 2^-15 must give the same detections and SNRs,
    noisePower and the peak 10 log10(2^-30) dB lower, with and without the filter.  A power-of-two scale is exact through the filter
    and the transforms, so a detection's cell level (SNR + noisePower, fp64 from the map cell) moves by exactly that;
    noisePower, a mean of per-cell fp32 dB values (log2f of 2^-60 times a value does not round like log2f of the
    value, minus 60), moves by it up to fp32 rounding: a few 1e-6 dB, the same for every SNR of the CPI."""
    g = load_golden("medium")
    n = int(g["params"][1])
    p1, p2 = str(tmp_path / "a.usrp.iq"), str(tmp_path / "b.usrp.iq")
    fixture_capture(g, 2040, p1)
    fixture_capture(g, 2040, p2, scale=2.0 ** -15)
    shift = 10 * np.log10(2.0 ** -30)
    for cfg in (medium_cfg(g), clutter_cfg(g)):
        big, _ = replay_usrp(p1, n, 2040, cfg)
        small, _ = replay_usrp(p2, n, 2040, cfg)
        for a, b in zip(big, small):
            assert not a.get("skipped") and not b.get("skipped")
            assert list(zip(a["delay"], a["doppler"])) == list(zip(b["delay"], b["doppler"])) and len(a["delay"]) >= 1
            level_a = np.asarray(a["snr"]) + a["noisePower"]
            level_b = np.asarray(b["snr"]) + b["noisePower"]
            assert np.allclose(level_b - level_a, shift, rtol=0, atol=1e-9)  # the cells: exact
            assert np.allclose(a["snr"], b["snr"], rtol=0, atol=1e-5)
            assert abs(b["noisePower"] - a["noisePower"] - shift) < 1e-3
            # Map.cpp:187-206: maxPower = max(0, peak dB) - noisePower (the running maximum starts at 0): the peak moves
            # by the shift, and where that takes it below 0 dB the 0 stands in for it
            peak_a = a["maxPower"] + a["noisePower"]
            assert peak_a > 0
            assert abs(b["maxPower"] - (max(0.0, peak_a + shift) - b["noisePower"])) < 1e-4


def test_usrp_replay_at_the_timed_size(b2, tmp_path):
    """configs[1] (2 MS/s, 1 s CPI, 513 x 411) with the 410-tap filter and the 1-D CFAR, two CPIs from a USRP capture of
    block 2040, one batch of 2: maps bit-identical to the same planes fed straight into the FMT_C32 chain (the de-block is
    an exact copy, the chain deterministic), and CPI 0 within the oracle's gates."""
    import torch
    from blah2_amd import replay as R
    from gates import cfar1d_margins, detection_gate, margin_eps
    from oracle import blah2_oracle as O
    from test_full_chain_gpu import check_chain_map
    fs = n = 2_000_000
    geom = (-10, 400, -256, 256, fs, n)
    xs, ys = [], []
    for c in range(2):
        x, y = O.synth_iq(n, seed=41 + c, fs=fs, targets=((37, -63.0, 0.05), (250, 120.0, 0.03)))
        xs.append(x.astype(np.complex64))
        ys.append(y.astype(np.complex64))
    path = str(tmp_path / "cfg2.usrp.iq")
    write_usrp(path, np.concatenate(xs), np.concatenate(ys), 2040)
    cfg = {"fs": fs, "n_samples": n,
           "ambiguity": {"delayMin": -10, "delayMax": 400, "dopplerMin": -256, "dopplerMax": 256},
           "detection": {"enable": True, "pfa": 1e-5, "nGuard": 2, "nTrain": 6, "minDelay": 5, "minDoppler": 15.0},
           "clutter": {"enable": True, "delayMin": -10, "delayMax": 400}}
    cap = R.UsrpFile(path, n, 2040)
    assert cap.n_cpis == 2
    chain = R.GpuChain(cfg, 0, batch=2, want_map=True, layout="usrp", usrp_block=2040)
    try:
        res = R.replay(cap, chain, batch=2)
        assert [r["cpi"] for r in res] == [0, 1] and not any(r.get("skipped") for r in res)
        # the same planes straight into the chain's own handles, FMT_C32, one batch of 2
        st = torch.cuda.current_stream().cuda_stream
        dx = torch.from_numpy(np.stack(xs)).cuda()
        dy = torch.from_numpy(np.stack(ys)).cuda()
        nD, nC = chain.amb.get_n_doppler_bins(), chain.amb.get_n_delay_bins()
        d_map = torch.zeros((2, nD, nC), dtype=torch.complex64, device="cuda")
        d_met = torch.zeros((2, 2), dtype=torch.float64, device="cuda")
        d_ok = torch.zeros(2, dtype=torch.int32, device="cuda")
        if chain.fused_fir:
            chain.wh.estimate_dev_fmt(b2.FMT_C32, dx.data_ptr(), dy.data_ptr(), 2, n, d_ok.data_ptr(), st)
            chain.amb.process_dev(b2.FMT_C32, dx.data_ptr(), dy.data_ptr(), 2, n, d_map.data_ptr(), d_met.data_ptr(), st)
        else:
            yf = torch.empty((2, n), dtype=torch.complex64, device="cuda")
            chain.wh.process_dev_fmt(b2.FMT_C32, dx.data_ptr(), dy.data_ptr(), 2, n, yf.data_ptr(), n, d_ok.data_ptr(), st)
            chain.amb.process_dev(b2.FMT_C32, dx.data_ptr(), yf.data_ptr(), 2, n, d_map.data_ptr(), d_met.data_ptr(), st)
        torch.cuda.synchronize()
        assert d_ok.cpu().tolist() == [1, 1]
        direct_maps, direct_met = d_map.cpu().numpy(), d_met.cpu().numpy()
    finally:
        chain.close()
        cap.close()
    for c in range(2):
        assert np.array_equal(res[c]["map"].view(np.uint32), direct_maps[c].view(np.uint32)), c
        assert res[c]["noisePower"] == direct_met[c, 0] and res[c]["maxPower"] == direct_met[c, 1]
    # CPI 0 against the fp64 oracle's chain on the same fp32 values
    x0, y0 = xs[0].astype(np.complex128), ys[0].astype(np.complex128)
    _, y_ref, _, _, b_ref = O.wiener_hopf(x0, y0, -10, 400, return_filter=True)
    d = O.ambiguity_dims(*geom, True)
    ref = O.ambiguity_process(d, x0, y_ref)
    noise_ref, max_ref = O.map_metrics(ref)
    direct_level = np.max(np.abs(b_ref)) * (d.n_corr * d.n_doppler_bins / n)
    cell = check_chain_map("configs[1] USRP replay", res[0]["map"], res[0]["noisePower"], ref, noise_ref, direct_level,
                           d.doppler, d.delay, -10, 400)
    assert abs(res[0]["noisePower"] - noise_ref) <= 1e-3 and abs(res[0]["maxPower"] - max_ref) <= 1e-3
    dl, dp, _ = O.cfar1d_fast(ref, d.delay, d.doppler, noise_ref, 1e-5, 2, 6, 5, 15.0)
    mg = cfar1d_margins(ref, 1e-5, 2, 6)
    dg = detection_gate(zip(dl, dp), zip(res[0]["delay"], res[0]["doppler"]), mg, d.doppler, d.delay[0], margin_eps(cell))
    print(f"[configs[1] USRP replay] detections: {dg}")
    assert dg["ok"] and dg["n_ref"] > 0, dg
