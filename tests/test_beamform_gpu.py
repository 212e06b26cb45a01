"""GPU: the surveillance channels as one array -- beams in the map domain (blah2hip_amb_beamform_dev, beamform_kernel)
and the per-detection array snapshot (blah2hip_amb_snapshot_dev, snapshot_kernel).

No reference counterpart; the check is an fp64 NumPy restatement.  The kernels read any buffer with the map layout, so
most cases feed crafted maps: unit-variance complex normal cells, channel k scaled by 10^k (a dropped or swapped channel
shows), no cell zero.  The handle is only there for its dimensions.

Bounds
  * cells: |out - sum_k w[b][k] M_k| <= 4 (K + 1) 2^-24 sum_k |w[b][k]| |M_k|, derived, not measured: a complex fp32
    product carries under 3 ulp of its magnitude and each of the K - 1 additions one.  It is relative to the TERMS, so
    beams that cancel are held to what fp32 can deliver.
  * metrics: 1e-3 dB (the project's DB_TOL) against fp64 Map::set_metrics of the device's OWN output cells: the
    reduction is tested, not the cells again.
Geometries: 21 x 111 cells (an odd count: with several CPIs every other map starts 8 bytes off a 16-byte boundary, and
with an odd number of CPIs the channels' blocks do as well), 21 x 112 (even: every map aligned) and the configs[1] size
513 x 411 (hundreds of workgroups per CPI, and with 6 CPIs workgroups that walk more than one stretch).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces
PAD = 64
MAX_BATCH = 24
SMALL = (-10, 100, -100, 100, 1_000_000, 100_000)    # 21 x 111
EVEN = (-10, 101, -100, 100, 1_000_000, 100_000)     # 21 x 112
CFG2 = (-10, 400, -256, 256, 2_000_000, 2_000_000)   # configs[1]: 513 x 411
DB_TOL = 1e-3
# (geometry, K, n_beams, n_cpi)
CASES = [(SMALL, 1, 1, 1), (SMALL, 2, 1, 3), (SMALL, 3, 3, 2), (SMALL, 4, 4, 3), (SMALL, 8, 8, 3), (SMALL, 5, 2, 1),
         (EVEN, 3, 2, 3), (EVEN, 8, 8, 2), (CFG2, 4, 4, 6), (CFG2, 3, 2, 1)]
IDS = [f"{g[1] - g[0] + 1}cols-K{k}-b{b}-cpi{c}" for g, k, b, c in CASES]


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


_handles = {}


def handle(b2, geom):
    if geom not in _handles:
        _handles[geom] = b2.Ambiguity(*geom, True, max_batch=MAX_BATCH)
    return _handles[geom]


def guarded(torch, shape, dtype):
    words = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size() // 4
    whole = torch.full((words + PAD,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    return whole, whole[:words].view(dtype).view(shape)


def guard_intact(whole):
    return bool((whole[-PAD:].cpu().numpy().view(np.uint32) == GUARD).all())


def untouched(whole):
    return bool((whole.cpu().numpy().view(np.uint32) == GUARD).all())


def crafted(K, n_cpi, nD, nC, seed):
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((K, n_cpi, nD, nC)) + 1j * rng.standard_normal((K, n_cpi, nD, nC))) * np.sqrt(0.5)
    z *= (10.0 ** np.arange(K))[:, None, None, None]
    z = z.astype(np.complex64)
    assert (z != 0).all()
    return z


def weights(K, n_beams, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_beams, K)) + 1j * rng.standard_normal((n_beams, K))).astype(np.complex64)


def beamform(torch, amb, d_in, K, n_cpi, w):
    """One call into guarded outputs -> (beam maps [n_beams, n_cpi, nD, nC], metrics [n_beams, n_cpi, 2])."""
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    wo, out = guarded(torch, (w.shape[0], n_cpi, nD, nC), torch.complex64)
    wm, met = guarded(torch, (w.shape[0], n_cpi, 2), torch.float64)
    amb.beamform_dev(d_in.data_ptr(), K, n_cpi, w, out.data_ptr(), met.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert guard_intact(wo) and guard_intact(wm)
    return out.cpu().numpy(), met.cpu().numpy()


def cell_bound_check(out, maps, w, tag):
    """out [n_beams, ...] against the fp64 combination of maps [K, ...] under the derived bound; the worst ratio is printed."""
    K = maps.shape[0]
    w64 = w.astype(np.complex64).astype(np.complex128)
    ref = np.tensordot(w64, maps.astype(np.complex128), axes=(1, 0))
    bound = 4 * (K + 1) * 2.0 ** -24 * np.tensordot(np.abs(w64), np.abs(maps.astype(np.complex128)), axes=(1, 0))
    err = np.abs(out.astype(np.complex128) - ref)
    print(f"{tag}: largest error / bound {float((err / bound).max()):.3f}")
    assert np.isfinite(out.view(np.float32)).all(), tag
    assert (err <= bound).all(), (tag, float((err / bound).max()))
    return ref


def set_metrics64(z):
    """Map::set_metrics (Map.cpp:187-206) in fp64."""
    db = 10.0 * np.log10(np.abs(z.astype(np.complex128)))
    noise = db.mean()
    return noise, max(0.0, db.max()) - noise


_results = {}


def case_result(b2, torch, case):
    """Input maps, weights and the device's outputs of one case: computed once, shared by the tests, left unchanged."""
    if case not in _results:
        geom, K, nb, n_cpi = case
        amb = handle(b2, geom)
        nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
        maps = crafted(K, n_cpi, nD, nC, seed=1000 + 100 * K + 10 * nb + n_cpi)
        w = weights(K, nb, seed=7 + K + nb)
        out, met = beamform(torch, amb, torch.from_numpy(maps).cuda(), K, n_cpi, w)
        _results[case] = (maps, w, out, met)
    return _results[case]


# ---- 1. cells ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cells_within_the_fp32_bound(b2, torch, case):
    geom, K, nb, n_cpi = case
    maps, w, out, _ = case_result(b2, torch, case)
    assert out.shape[:2] == (nb, n_cpi)
    if geom is SMALL:
        assert out[0, 0].size % 2 == 1  # the odd cell count the alignment cases rest on
    cell_bound_check(out, maps, w, f"beamform K={K} beams={nb} n_cpi={n_cpi} {out.shape[2]}x{out.shape[3]}")


# ---- 2. unit weights ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,n_cpi", [(SMALL, 3), (SMALL, 2), (EVEN, 3)], ids=["8-byte", "head-and-tail", "aligned"])
def test_permutation_weights_copy_the_channels_bit_for_bit(b2, torch, geom, n_cpi):
    amb = handle(b2, geom)
    perm = [2, 0, 1]
    maps = crafted(3, n_cpi, amb.get_n_doppler_bins(), amb.get_n_delay_bins(), seed=31 + n_cpi)
    w = np.zeros((3, 3), dtype=np.complex64)
    for b, k in enumerate(perm):
        w[b, k] = 1.0
    out, met = beamform(torch, amb, torch.from_numpy(maps).cuda(), 3, n_cpi, w)
    for b, k in enumerate(perm):
        assert np.array_equal(out[b].view(np.uint32), maps[k].view(np.uint32)), (b, k)
        for c in range(n_cpi):
            noise, peak = set_metrics64(maps[k, c])
            assert abs(met[b, c, 0] - noise) <= DB_TOL and abs(met[b, c, 1] - peak) <= DB_TOL, (b, c)


# ---- 3. metrics ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_metrics_are_set_metrics_of_the_cells_as_written(b2, torch, case):
    _, K, nb, n_cpi = case
    _, _, out, met = case_result(b2, torch, case)
    worst = 0.0
    for b in range(nb):
        for c in range(n_cpi):
            noise, peak = set_metrics64(out[b, c])
            worst = max(worst, abs(met[b, c, 0] - noise), abs(met[b, c, 1] - peak))
            assert abs(met[b, c, 0] - noise) <= DB_TOL, (b, c, met[b, c, 0], noise)
            assert abs(met[b, c, 1] - peak) <= DB_TOL, (b, c, met[b, c, 1], peak)
    print(f"beam metrics K={K} beams={nb} n_cpi={n_cpi}: largest difference {worst:.3e} dB")


# ---- 4. determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[3], CASES[4], CASES[8]], ids=[IDS[3], IDS[4], IDS[8]])
def test_two_calls_give_the_same_bits(b2, torch, case):
    geom, K, nb, n_cpi = case
    maps, w, out, met = case_result(b2, torch, case)
    out2, met2 = beamform(torch, handle(b2, geom), torch.from_numpy(maps).cuda(), K, n_cpi, w)
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32))
    assert np.array_equal(met.view(np.uint64), met2.view(np.uint64))


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(b2, torch):
    from blah2_amd import _lib
    amb = handle(b2, SMALL)
    L, h = amb._L, amb._h
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    cells = nD * nC
    d_in = torch.from_numpy(crafted(8, 3, nD, nC, seed=5)).cuda()
    wo, out = guarded(torch, (MAX_BATCH, nD, nC), torch.complex64)
    wm, met = guarded(torch, (MAX_BATCH, 2), torch.float64)
    w = np.ascontiguousarray(weights(9, 9, seed=3))
    wp = C.c_void_p(w.ctypes.data)
    int_map, int_met = C.c_void_p(), C.c_void_p()
    assert L.blah2hip_amb_result_ptrs(h, C.byref(int_map), C.byref(int_met)) == _lib.OK
    # (d_map, n_surv, n_cpi, w, n_beams, d_beam_map, d_beam_metrics)
    good = [d_in.data_ptr(), 2, 3, wp, 2, out.data_ptr(), met.data_ptr()]
    bad = {
        "n_surv 0": {1: 0}, "n_surv 9": {1: 9, 2: 1}, "n_beams 0": {4: 0}, "n_beams 9": {4: 9, 2: 1}, "n_cpi 0": {2: 0},
        "n_surv * n_cpi above max_batch": {1: 8, 2: 4, 4: 1}, "n_beams * n_cpi above max_batch": {1: 1, 2: 4, 4: 8},
        "NULL w": {3: None}, "NULL beam map": {5: None}, "NULL beam metrics": {6: None},
        "beam map inside the input": {5: d_in.data_ptr() + 8 * (2 * 3 * cells - 1)},
        "beam map around the input's start": {0: out.data_ptr() + 8 * cells},
        "beam metrics inside the input": {6: d_in.data_ptr() + 16},
        "beam map in the handle's own map": {0: None, 5: int_map.value + 8 * cells},
    }
    for name, change in bad.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert L.blah2hip_amb_beamform_dev(h, *args, None) == _lib.ERR_INVALID, name
    torch.cuda.synchronize()
    assert untouched(wo) and untouched(wm)
    # the call they were derived from is accepted (output directly behind the input is no overlap)
    assert L.blah2hip_amb_beamform_dev(h, *good, None) == _lib.OK
    torch.cuda.synchronize()
    assert guard_intact(wo) and guard_intact(wm) and not untouched(wo) and not untouched(wm)


# ---- 6. through the chain -------------------------------------------------------------------------------------------------
PHI = np.pi / 2       # phase step of the echo from channel to channel: 30 degrees off broadside at half-wave spacing
ECHO = (37, -60.0, 0.05)


def array_scene(n, fs, K, seed):
    """int8 samples [n, 2] in the manner of tests/test_multi_surv_gpu.py: a noise-like reference x; channel k is
    0.8 x + the echo with phase exp(j k PHI) + noise of its own seed, rounded and clipped like an 8-bit receiver's."""
    rng = np.random.default_rng(seed)
    x = 30.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    t = np.arange(n) / fs

    def q(v):
        return np.clip(np.stack([np.rint(v.real), np.rint(v.imag)], axis=-1), -128, 127).astype(np.int8)
    d, f, a = ECHO
    xd = np.roll(x, d)
    xd[:d] = 0
    ys = []
    for k in range(K):
        rk = np.random.default_rng(100 * seed + 1 + k)
        ys.append(q(0.8 * x + a * xd * np.exp(2j * np.pi * f * t + 1j * k * PHI) + 3.0 * (rk.standard_normal(n) + 1j * rk.standard_normal(n))))
    return q(x), ys


def test_chain_from_int8_samples_to_beam_detections(b2, torch):
    K, B, NB = 3, 2, 2
    amb = handle(b2, SMALL)
    n, fs = SMALL[5], SMALL[4]
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    st = torch.cuda.current_stream().cuda_stream
    cpis = [array_scene(n, fs, K, 40 + c) for c in range(B)]
    tx = torch.from_numpy(np.stack([c[0] for c in cpis])).cuda()
    tys = [torch.from_numpy(np.stack([c[1][k] for c in cpis])).cuda() for k in range(K)]
    wc, chan = guarded(torch, (K, B, nD, nC), torch.complex64)
    wcm, chan_met = guarded(torch, (K, B, 2), torch.float64)
    amb.process_multi_dev(b2.FMT_I8, tx.data_ptr(), [t.data_ptr() for t in tys], B, n, chan.data_ptr(), chan_met.data_ptr(), st)
    # beam 0 towards the echo, beam 1 with the echo's direction in its first null (2 pi / K further along the array)
    angles = np.rad2deg(np.arcsin([PHI / np.pi, (PHI - 2 * np.pi / K) / np.pi]))
    w = b2.ula_weights(K, 0.5, angles).astype(np.complex64)
    beams, met = beamform(torch, amb, chan, K, B, w)
    assert guard_intact(wc) and guard_intact(wcm)
    maps = chan.cpu().numpy()
    cell_bound_check(beams, maps, w, "chain beams")
    row, col = int(np.argmin(np.abs(amb.doppler - ECHO[1]))), ECHO[0] - SMALL[0]
    for c in range(B):
        terms = np.exp(-1j * PHI * np.arange(K)) * maps[:, c, row, col].astype(np.complex128)
        bound = 4 * (K + 1) * 2.0 ** -24 * np.abs(terms).sum() / K
        assert abs(complex(beams[0, c, row, col]) - terms.mean()) <= bound, c
        # the null cancels the echo: what is left in that cell is the sidelobe floor of the direct path, 0.8 sqrt(N) against
        # the echo's 0.05 N = 0.05 of it in the mean at N = 1e5 samples, Rayleigh distributed: a tenfold margin
        assert abs(beams[1, c, row, col]) < 0.5 * abs(beams[0, c, row, col]), c

    # detector + Centroid + Interpolate over the NB * B virtual CPIs, against the host functions on each downloaded beam map
    V, cap = NB * B, nD * nC
    d_beams, d_met = torch.from_numpy(beams).cuda(), torch.from_numpy(met).cuda()
    d_hits = torch.zeros((V, cap, 2), dtype=torch.float64, device="cuda")
    d_cnt = torch.zeros(V, dtype=torch.int32, device="cuda")
    d_out = torch.zeros((V, cap, 4), dtype=torch.float64, device="cuda")
    d_n = torch.full((V,), -1, dtype=torch.int32, device="cuda")
    step = float(amb.doppler[1] - amb.doppler[0])
    det = b2.CfarDetector1D(1e-5, 2, 6, 5, 15.0)
    det.process_dev(amb, V, d_hits.data_ptr(), cap, d_cnt.data_ptr(), d_beams.data_ptr(), d_met.data_ptr(), st)
    b2.DetectionFinisher(6, 6, step, True, True).process_dev(amb, V, d_hits.data_ptr(), cap, d_cnt.data_ptr(), d_out.data_ptr(), cap,
                                                             d_n.data_ptr(), d_beams.data_ptr(), d_met.data_ptr(), st)
    torch.cuda.synchronize()
    counts = d_n.cpu().numpy()
    recs = d_out.cpu().numpy().view(b2.DET_DTYPE).reshape(V, cap)
    for b in range(NB):
        for c in range(B):
            v = b * B + c
            m = b2.Map(None, beams[b, c], amb.delay.copy(), amb.doppler.copy(), float(met[b, c, 0]), float(met[b, c, 1]))
            host = b2.Interpolate(True, True).process(b2.Centroid(6, 6, step).process(det.process(m)), m)
            dev = b2.dets_to_detection(recs[v], int(counts[v]), cap)  # sorted by the hit it came from: the host's order
            assert dev.get_nDetections() == host.get_nDetections(), (b, c)
            assert np.allclose(dev.get_delay(), host.get_delay(), rtol=0, atol=1e-9, equal_nan=True), (b, c)
            assert np.allclose(dev.get_doppler() / step, host.get_doppler() / step, rtol=0, atol=1e-9, equal_nan=True), (b, c)
            assert np.allclose(dev.get_snr(), host.get_snr(), rtol=0, atol=1e-9, equal_nan=True), (b, c)
            if b == 0:
                hit = (np.abs(dev.get_delay() - ECHO[0]) < 1.0) & (np.abs(dev.get_doppler() - ECHO[1]) < step)
                assert hit.any(), ("the echo is missing from beam 0", c)


# ---- 7. snapshot ----------------------------------------------------------------------------------------------------------
def test_snapshot_gathers_the_channel_cells(b2, torch):
    from blah2_amd import _lib
    K, n_cpi, cap = 3, 2, 8
    counts = np.array([0, 1, cap, cap + 5], dtype=np.uint32)
    n_lists = counts.size  # 2 * n_cpi
    amb = handle(b2, SMALL)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    maps = crafted(K, n_cpi, nD, nC, seed=77)
    rng = np.random.default_rng(78)
    dets = np.zeros((n_lists, cap), dtype=b2.DET_DTYPE)  # every slot holds a cell of the map: one read behind a count would show
    dets["row"] = rng.integers(0, nD, size=(n_lists, cap))
    dets["col"] = rng.integers(0, nC, size=(n_lists, cap))
    dets["row"][2, 3] = nD   # outside the map: slot left unwritten
    dets["col"][3, 0] = -1
    dets["row"][3, 7], dets["col"][3, 7] = nD - 1, nC - 1  # the last cell of the map
    d_map = torch.from_numpy(maps).cuda()
    d_dets = torch.from_numpy(dets.view(np.float64).reshape(n_lists, cap, 4)).cuda()
    d_cnt = torch.from_numpy(counts.view(np.int32)).cuda()
    ws, snap = guarded(torch, (n_lists, cap, K), torch.complex64)
    st = torch.cuda.current_stream().cuda_stream
    amb.snapshot_dev(d_map.data_ptr(), K, n_cpi, d_dets.data_ptr(), cap, d_cnt.data_ptr(), n_lists, snap.data_ptr(), st)
    torch.cuda.synchronize()
    assert guard_intact(ws)
    got = snap.cpu().numpy().view(np.uint32).reshape(n_lists, cap, K, 2)
    written = 0
    for l in range(n_lists):
        for i in range(cap):
            r, c = int(dets["row"][l, i]), int(dets["col"][l, i])
            if i < min(int(counts[l]), cap) and 0 <= r < nD and 0 <= c < nC:
                want = np.ascontiguousarray(maps[:, l % n_cpi, r, c]).view(np.uint32).reshape(K, 2)
                assert np.array_equal(got[l, i], want), (l, i)
                written += 1
            else:
                assert (got[l, i] == GUARD).all(), (l, i)
    assert written == 1 + (cap - 1) + (cap - 1)
    # refusals: nothing enqueued
    L, h = amb._L, amb._h
    ws2, snap2 = guarded(torch, (n_lists, cap, K), torch.complex64)
    good = [d_map.data_ptr(), K, n_cpi, d_dets.data_ptr(), cap, d_cnt.data_ptr(), n_lists, snap2.data_ptr()]
    for name, change in {"n_lists no multiple of n_cpi": {6: 3}, "n_lists 0": {6: 0}, "NULL lists": {3: None}, "NULL counts": {5: None},
                         "NULL output": {7: None}, "cap 0": {4: 0}, "n_cpi 0": {2: 0}, "n_surv 0": {1: 0}, "n_surv 9": {1: 9}}.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert L.blah2hip_amb_snapshot_dev(h, *args, None) == _lib.ERR_INVALID, name
    torch.cuda.synchronize()
    assert untouched(ws2)


# ---- 8. the host-array helper ---------------------------------------------------------------------------------------------
def test_beamform_on_host_arrays_returns_maps_with_metrics(b2, torch):
    amb = handle(b2, SMALL)
    maps = crafted(3, 1, amb.get_n_doppler_bins(), amb.get_n_delay_bins(), seed=91)[:, 0]
    w = b2.ula_weights(3, 0.5, [0.0, 20.0])
    beams = amb.beamform(list(maps), w)
    assert len(beams) == 2
    cell_bound_check(np.stack([m.data for m in beams]), maps, w.astype(np.complex64), "beamform(host arrays)")
    for m in beams:
        noise, peak = set_metrics64(m.data)
        assert abs(m.noisePower - noise) <= DB_TOL and abs(m.maxPower - peak) <= DB_TOL
        assert np.array_equal(m.delay, amb.delay) and np.array_equal(m.doppler, amb.doppler)
