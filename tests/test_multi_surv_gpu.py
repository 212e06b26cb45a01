"""GPU: several surveillance channels against one reference channel (blah2hip_amb_process_multi_dev).

Channel k of CPI c is virtual CPI k * n_cpi + c of everything behind the range stage.  The per-channel path runs the
two-channel range stage once per channel, so its maps and metrics are the BITS of blah2hip_amb_process_dev on (x, y_k)
under the same kernels; the shared-reference kernel (rangew1k_shared_kernel) is held to the fp64 oracle through the
project's gates (tests/gates.py) at the configs[1] size, every channel carrying an echo of its own so that a swapped
or duplicated channel cannot pass.  The samples are int8-valued throughout: exact as int8 planes and as fp32 planes,
so both formats share one set of oracle maps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces
SMALL = (-10, 100, -100, 100, 1_000_000, 100_000)
ASYM = (-10, 100, -60, 100, 1_000_000, 100_000)      # asymmetric Doppler limits: the rotate pass
CHUNKS = (-30, 4400, -4, 4, 400_000, 400_000)        # 4431 delay bins: three lag chunks on the 4096-point transform
CFG2 = (-10, 400, -256, 256, 2_000_000, 2_000_000)   # configs[1]: 513 x 411
# (delay, Doppler Hz, amplitude) of channel k's own echo
ECHO = ((37, -63.0, 0.05), (250, 120.0, 0.05), (91, 33.0, 0.05), (173, -201.0, 0.05))
ECHO_SMALL = ((37, -60.0, 0.05), (72, 40.0, 0.05), (15, 80.0, 0.05))


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


def scene(n, fs, echoes, seed):
    """int8 samples [n, 2]: a noise-like reference x and one surveillance channel per echo, y_k = 0.8 x + its echo +
    its own noise, rounded and clipped like an 8-bit receiver's."""
    rng = np.random.default_rng(seed)
    x = 30.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    t = np.arange(n) / fs

    def q(v):
        return np.clip(np.stack([np.rint(v.real), np.rint(v.imag)], axis=-1), -128, 127).astype(np.int8)
    ys = []
    for d, f, a in echoes:
        xd = np.roll(x, d)
        xd[:d] = 0
        ys.append(q(0.8 * x + a * xd * np.exp(2j * np.pi * f * t) + 3.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))))
    return q(x), ys


def as_c128(a):
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


def guarded(torch, shape, dtype, pad=64):
    words = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size() // 4
    whole = torch.full((words + pad,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    return whole, whole[:words].view(dtype).view(shape)


def guard_intact(whole, pad=64):
    return bool((whole[-pad:].cpu().numpy().view(np.uint32) == GUARD).all())


def plane(torch, fmt_i8, cpis, stride):
    """int8 CPIs [B][n, 2] as a device plane of ``stride`` samples per CPI (int8 pairs, or the same values as complex
    fp32); the gaps hold a value a read beyond a CPI would pick up.  (keep-alive tensor, pointer)"""
    B, n = len(cpis), cpis[0].shape[0]
    if fmt_i8:
        host = np.full((B, stride, 2), 77, dtype=np.int8)
        for c in range(B):
            host[c, :n] = cpis[c]
    else:
        host = np.full((B, stride), 77 + 77j, dtype=np.complex64)
        for c in range(B):
            host[c, :n] = cpis[c][:, 0].astype(np.float32) + 1j * cpis[c][:, 1].astype(np.float32)
    t = torch.from_numpy(host).cuda()
    return t, t.data_ptr()


def run_multi(torch, amb, fmt, px, pys, B, stride):
    """(maps [K * B, nD, nC], metrics [K * B, 2], range kernel id) of one multi call into guarded buffers."""
    from blah2_amd import _lib
    K = len(pys)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    whole, out = guarded(torch, (K * B, nD, nC), torch.complex64)
    wm, met = guarded(torch, (K * B, 2), torch.float64)
    amb.process_multi_dev(fmt, px, pys, B, stride, out.data_ptr(), met.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert guard_intact(whole) and guard_intact(wm)
    return out.cpu().numpy(), met.cpu().numpy(), amb.info(_lib.INFO_LAST_RANGE_KERNEL)


def run_single(torch, amb, fmt, px, py, B, stride):
    from blah2_amd import _lib
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    whole, out = guarded(torch, (B, nD, nC), torch.complex64)
    wm, met = guarded(torch, (B, 2), torch.float64)
    amb.process_dev(fmt, px, py, B, stride, out.data_ptr(), met.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert guard_intact(whole) and guard_intact(wm)
    return out.cpu().numpy(), met.cpu().numpy(), amb.info(_lib.INFO_LAST_RANGE_KERNEL)


def small_planes(torch, geom, K, B, stride, seed, echoes=ECHO_SMALL):
    n, fs = geom[5], geom[4]
    cpis = [scene(n, fs, echoes[:K], seed + c) for c in range(B)]
    tx, px = plane(torch, False, [c[0] for c in cpis], stride)
    tys = [plane(torch, False, [c[1][k] for c in cpis], stride) for k in range(K)]
    return cpis, (tx, tys), px, [t[1] for t in tys]


# ---- 1. the per-channel path, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [SMALL, ASYM, CHUNKS], ids=["symmetric", "rotate-pass", "lag-chunks"])
def test_per_channel_path_is_bitwise_the_two_channel_call(b2, geom):
    """K = 3, n_cpi = 2, FMT_C32, mode per-channel: map and metrics of virtual CPI k * n_cpi + c are, as uint32 / uint64
    views, those of process_dev on (x, y_k) with the same range and Doppler kernels forced (same kernels, same inputs)."""
    import torch
    from blah2_amd import _lib
    K, B = 3, 2
    n = geom[5]
    stride = n + 37
    echoes = ((37, -2.0, 0.05), (4000, 2.0, 0.1), (17, -3.0, 0.05)) if geom is CHUNKS else ECHO_SMALL
    _, keep, px, pys = small_planes(torch, geom, K, B, stride, seed=100 + len(geom) + abs(geom[2]), echoes=echoes)
    amb = b2.Ambiguity(*geom, True, max_batch=K * B)
    if geom is CHUNKS:
        assert amb.get_n_delay_bins() == 4431 and amb.dims.fft_len == 4096
    amb.set_multi_surv_range("per_channel")
    maps, mets, rk = run_multi(torch, amb, b2.FMT_C32, px, pys, B, stride)
    dk = amb.info(_lib.INFO_LAST_DOPPLER_KERNEL)
    assert rk != _lib.RANGE_SHARED and np.abs(maps).max() > 0
    amb.set_range_kernel(rk)
    amb.set_doppler_kernel(dk)
    for k in range(K):
        m1, met1, rk1 = run_single(torch, amb, b2.FMT_C32, px, pys[k], B, stride)
        assert rk1 == rk and amb.info(_lib.INFO_LAST_DOPPLER_KERNEL) == dk
        assert np.array_equal(maps[k * B:(k + 1) * B].view(np.uint32), m1.view(np.uint32)), k
        assert np.array_equal(mets[k * B:(k + 1) * B].view(np.uint64), met1.view(np.uint64)), k
    # the channels differ (each has its own echo): no block is a copy of another
    assert not np.array_equal(maps[0:B].view(np.uint32), maps[B:2 * B].view(np.uint32))


# ---- 2. the shared-reference kernel against the oracle --------------------------------------------------------------
N_CPI = 6            # 6 x 513 pulses per channel: from 12 x CUs pulses the planner's own choice is rangew1k_kernel
CHECKED = (0, N_CPI - 1)
_cache = {}


def cfg2_scenes():
    """Two distinct CPIs (the checked ones) of one reference and four surveillance channels, and their oracle maps."""
    if "scenes" not in _cache:
        n, fs = CFG2[5], CFG2[4]
        _cache["scenes"] = {c: scene(n, fs, ECHO, 900 + c) for c in CHECKED}
    return _cache["scenes"]


def cfg2_ref(c, k):
    from oracle import blah2_oracle as O
    if ("ref", c, k) not in _cache:
        x, ys = cfg2_scenes()[c]
        d = O.ambiguity_dims(*CFG2, True)
        ref = O.ambiguity_process(d, as_c128(x), as_c128(ys[k]))
        _cache[("ref", c, k)] = (ref, O.map_metrics(ref), d)
    return _cache[("ref", c, k)]


def cfg2_planes(torch, fmt_i8, K):
    """CPIs 0 .. N_CPI - 2 hold the first scene, the last CPI the second one."""
    sc = cfg2_scenes()
    order = [CHECKED[0]] * (N_CPI - 1) + [CHECKED[1]]
    n = CFG2[5]
    tx, px = plane(torch, fmt_i8, [sc[c][0] for c in order], n)
    tys = [plane(torch, fmt_i8, [sc[c][1][k] for c in order], n) for k in range(K)]
    return (tx, tys), px, [t[1] for t in tys]


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("fmt_name", ["FMT_C32", "FMT_I8"])
def test_shared_kernel_against_the_oracle(b2, fmt_name, K):
    """configs[1] geometry, 6 CPIs per channel, mode forced to shared: the new kernel id is reported; every channel of the
    first and the last CPI passes map_cell_gate, db_map_gate and the metrics gate; the strongest cell away from the
    zero-Doppler rows is the channel's own echo.  Then the same call on the per-channel path: the difference is printed
    and asserted to be zero bits (the per-channel operation order of the shared kernel is rangew1k_kernel's)."""
    import torch
    from blah2_amd import _lib
    from gates import db_map_gate, map_cell_gate
    fmt = getattr(b2, fmt_name)
    keep, px, pys = cfg2_planes(torch, fmt == b2.FMT_I8, K)
    n = CFG2[5]
    amb = b2.Ambiguity(*CFG2, True, max_batch=K * N_CPI)
    assert amb.dims.fft_len == 1024
    amb.set_multi_surv_range("per_channel")
    pm, pmet, prk = run_multi(torch, amb, fmt, px, pys, N_CPI, n)
    assert prk == _lib.RANGE_WAVE1K  # the planner's own choice at this batch: where auto may pick the shared kernel
    amb.set_multi_surv_range("shared")
    maps, mets, rk = run_multi(torch, amb, fmt, px, pys, N_CPI, n)
    assert rk == _lib.RANGE_SHARED
    for k in range(K):
        for c in CHECKED:
            v = k * N_CPI + c
            ref, (noise_ref, max_ref), d = cfg2_ref(c, k)
            tag = f"multi {fmt_name} K={K} channel {k} cpi {c}"
            cell = map_cell_gate(maps[v], ref, noise_ref)
            dbg = db_map_gate(maps[v], mets[v, 0], ref, noise_ref)
            print(f"\n[{tag}] cell {cell}\n[{tag}] dB map {dbg}\n[{tag}] metrics {mets[v]} vs {(noise_ref, max_ref)}")
            assert cell["ok"], cell
            assert dbg["ok"], dbg
            assert abs(mets[v, 0] - noise_ref) <= 1e-3 and abs(mets[v, 1] - max_ref) <= 1e-3
            # the channel's own echo: the strongest cell of the rows 5 Hz or more from zero Doppler
            away = np.abs(d.doppler) >= 5.0
            for name, m in (("oracle", ref), ("engine", maps[v])):
                a = np.abs(m) * away[:, None]
                i, j = np.unravel_index(np.argmax(a), a.shape)
                assert (d.delay[j], i) == (ECHO[k][0], int(np.argmin(np.abs(d.doppler - ECHO[k][1])))), (name, tag, d.delay[j], d.doppler[i])
        # CPIs 1 .. N_CPI - 2 hold the first CPI's samples
        for c in range(1, N_CPI - 1):
            assert np.array_equal(maps[k * N_CPI + c].view(np.uint32), maps[k * N_CPI].view(np.uint32)), (k, c)
    differ = int((maps.view(np.uint32) != pm.view(np.uint32)).sum())
    worst = float(np.abs(maps.astype(np.complex128) - pm).max() / np.abs(pm).max())
    print(f"[multi {fmt_name} K={K}] shared vs per-channel path: {differ} of {maps.size * 2} words differ, "
          f"largest difference {worst:.3e} of the peak")
    assert differ == 0
    assert np.array_equal(mets.view(np.uint64), pmet.view(np.uint64))


# ---- 3. a lone channel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["per_channel", "shared", "auto"])
def test_one_channel_is_process_dev_bit_for_bit(b2, mode):
    import torch
    for geom, B in ((SMALL, 2), (CFG2, N_CPI)):
        if geom is CFG2:
            keep, px, pys = cfg2_planes(torch, False, 1)
            stride = geom[5]
        else:
            stride = geom[5] + 5
            _, keep, px, pys = small_planes(torch, geom, 1, B, stride, seed=31)
        amb = b2.Ambiguity(*geom, True, max_batch=B)
        amb.set_multi_surv_range(mode)
        m1, met1, rk1 = run_single(torch, amb, b2.FMT_C32, px, pys[0], B, stride)
        mm, metm, rkm = run_multi(torch, amb, b2.FMT_C32, px, pys, B, stride)
        assert rkm == rk1 and np.abs(m1).max() > 0
        assert np.array_equal(mm.view(np.uint32), m1.view(np.uint32))
        assert np.array_equal(metm.view(np.uint64), met1.view(np.uint64))


# ---- 4. everything behind the map on virtual CPIs -------------------------------------------------------------------
def test_detectors_and_read_last_on_virtual_cpis(b2):
    """cfar1d_dev and detect_dev once with n_cpi * n_surv on the handle's own buffers: per virtual CPI the lists the
    single-channel chain gives for (x, y_k); read_last(k * n_cpi + c) is that channel's map."""
    import torch
    from blah2_amd import _lib
    K, B, geom = 3, 2, SMALL
    n = geom[5]
    _, keep, px, pys = small_planes(torch, geom, K, B, n, seed=57)
    st = torch.cuda.current_stream().cuda_stream
    amb = b2.Ambiguity(*geom, True, max_batch=K * B)
    amb.set_multi_surv_range("per_channel")
    cfar = b2.CfarDetector1D(1e-5, 2, 6, 5, 15.0)
    fin = b2.DetectionFinisher(6, 6, 1.0 / amb.get_cpi())
    cap = 4096

    def chain(V, call):
        d_hits = torch.zeros((V, cap, 2), dtype=torch.float64, device="cuda")
        d_cnt = torch.zeros(V, dtype=torch.int32, device="cuda")
        d_out = torch.zeros((V, cap, 4), dtype=torch.float64, device="cuda")
        d_n = torch.zeros(V, dtype=torch.int32, device="cuda")
        call()
        cfar.process_dev(amb, V, d_hits.data_ptr(), cap, d_cnt.data_ptr(), None, None, st)
        fin.process_dev(amb, V, d_hits.data_ptr(), cap, d_cnt.data_ptr(), d_out.data_ptr(), cap, d_n.data_ptr(), None, None, st)
        torch.cuda.synchronize()
        cnt, nn = d_cnt.cpu().numpy(), d_n.cpu().numpy()
        assert cnt.min() > 0 and nn.min() > 0 and cnt.max() <= cap
        hits = [np.sort(d_hits[v, :int(cnt[v])].cpu().numpy().view(b2.HIT_DTYPE).reshape(-1), order=["row", "col"]) for v in range(V)]
        dets = [np.sort(d_out[v, :int(nn[v])].cpu().numpy().view(b2.DET_DTYPE).reshape(-1), order=["row", "col"]) for v in range(V)]
        maps = [amb.read_last(v) for v in range(V)]
        return hits, dets, maps

    hits, dets, maps = chain(K * B, lambda: amb.process_multi_dev(b2.FMT_C32, px, pys, B, n, None, None, st))
    amb.set_range_kernel(amb.info(_lib.INFO_LAST_RANGE_KERNEL))
    amb.set_doppler_kernel(amb.info(_lib.INFO_LAST_DOPPLER_KERNEL))
    for k in range(K):
        h1, d1, m1 = chain(B, lambda: amb.process_dev(b2.FMT_C32, px, pys[k], B, n, None, None, st))
        for c in range(B):
            v = k * B + c
            assert hits[v].tobytes() == h1[c].tobytes(), (k, c)
            assert dets[v].tobytes() == d1[c].tobytes(), (k, c)
            assert np.array_equal(np.ascontiguousarray(maps[v].data).view(np.uint32), np.ascontiguousarray(m1[c].data).view(np.uint32))
            assert (maps[v].noisePower, maps[v].maxPower) == (m1[c].noisePower, m1[c].maxPower)
            delays = set(b2.hits_to_detection(amb, hits[v], len(hits[v]), cap).get_delay().tolist())
            for kk in range(K):  # the channel's own echo and nobody else's
                assert (float(ECHO_SMALL[kk][0]) in delays) == (kk == k), (k, c, kk)


def test_host_planes_entry_equals_process(b2):
    """blah2hip_amb_process_multi_c32: one Map per channel, the bits Ambiguity.process gives for (x, y_k)."""
    geom, K = SMALL, 3
    x, ys = scene(geom[5], geom[4], ECHO_SMALL, 77)
    xc = as_c128(x).astype(np.complex64)
    ycs = [as_c128(y).astype(np.complex64) for y in ys]
    amb = b2.Ambiguity(*geom, True, max_batch=K)
    amb.set_multi_surv_range("per_channel")
    got = amb.process_multi(xc, ycs)
    assert len(got) == K
    for k in range(K):
        one = amb.process(xc, ycs[k])
        assert np.array_equal(np.ascontiguousarray(got[k].data).view(np.uint32), np.ascontiguousarray(one.data).view(np.uint32)), k
    with pytest.raises(RuntimeError):
        amb.process_multi(xc[:amb.dims.n_used - 1], ycs)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_leave_the_handle_usable(b2):
    import torch
    from blah2_amd import _lib
    geom, B = SMALL, 2
    n = geom[5]
    st = torch.cuda.current_stream().cuda_stream
    _, keep, px, pys = small_planes(torch, geom, 3, B, n, seed=5)
    amb = b2.Ambiguity(*geom, True, max_batch=6)
    amb.set_fft_len(1024)
    good, _, _ = run_multi(torch, amb, b2.FMT_C32, px, pys, B, n)

    def refused(code, word, fmt, planes, n_cpi):
        with pytest.raises(b2.Blah2HipError) as e:
            amb.process_multi_dev(fmt, px, planes, n_cpi, n, None, None, st)
        assert e.value.code == code and word in str(e.value), str(e.value)
        again, _, _ = run_multi(torch, amb, b2.FMT_C32, px, pys, B, n)  # a valid call on the same handle still works
        assert np.array_equal(again.view(np.uint32), good.view(np.uint32))

    refused(_lib.ERR_UNSUPPORTED, "FMT_I16", b2.FMT_I16, pys, B)
    refused(_lib.ERR_INVALID, "n_surv", b2.FMT_C32, [], B)
    refused(_lib.ERR_INVALID, "MAX_SURV", b2.FMT_C32, [pys[0]] * 9, 1)
    refused(_lib.ERR_INVALID, "NULL surveillance plane 1", b2.FMT_C32, [pys[0], None, pys[2]], B)
    refused(_lib.ERR_INVALID, "max_batch", b2.FMT_C32, [pys[0]] * 7, 1)  # 7 x 1 = max_batch + 1
    refused(_lib.ERR_INVALID, "max_batch", b2.FMT_C32, pys, 3)           # 3 x 3 > 6
    refused(_lib.ERR_INVALID, "format", 6, pys, B)
    # the shared kernel where it is not built: forced, that is an error, not a quiet other path
    amb.set_multi_surv_range("shared")
    with pytest.raises(b2.Blah2HipError) as e:
        amb.process_multi_dev(b2.FMT_F16, px, pys, B, n, None, None, st)
    assert e.value.code == _lib.ERR_UNSUPPORTED and "FMT_C32 and BLAH2HIP_FMT_I8" in str(e.value)
    amb.set_fft_len(2048)
    with pytest.raises(b2.Blah2HipError) as e:
        amb.process_multi_dev(b2.FMT_C32, px, pys, B, n, None, None, st)
    assert e.value.code == _lib.ERR_UNSUPPORTED and "1024" in str(e.value)
    amb.set_fft_len(1024)
    amb.set_multi_surv_range("auto")
    again, _, _ = run_multi(torch, amb, b2.FMT_C32, px, pys, B, n)
    assert np.array_equal(again.view(np.uint32), good.view(np.uint32))
    with pytest.raises(b2.Blah2HipError):
        amb.set_multi_surv_range(3)

    # a fused FIR set on the handle
    n2 = 190_647
    x2, y2 = scene(n2, n2, ECHO_SMALL[:2], 3)
    tx, px2 = plane(torch, False, [x2], n2)
    t0, p0 = plane(torch, False, [y2[0]], n2)
    t1, p1 = plane(torch, False, [y2[1]], n2)
    amb2 = b2.Ambiguity(-24, 2023, -15, 15, n2, n2, True, max_batch=2)
    amb2.set_fft_len(4096)
    wh = b2.WienerHopf(-24, 2023, n2)
    d_ok = torch.zeros(1, dtype=torch.int32, device="cuda")
    wh.estimate_dev_fmt(b2.FMT_C32, px2, p0, 1, n2, d_ok.data_ptr(), st)
    torch.cuda.synchronize()
    amb2.set_fir(wh)
    with pytest.raises(b2.Blah2HipError) as e:
        amb2.process_multi_dev(b2.FMT_C32, px2, [p0, p1], 1, n2, None, None, st)
    assert e.value.code == _lib.ERR_UNSUPPORTED and "fused FIR" in str(e.value)
    amb2.set_fir(None)
    amb2.process_multi_dev(b2.FMT_C32, px2, [p0, p1], 1, n2, None, None, st)
    torch.cuda.synchronize()
    assert np.abs(amb2.read_last(1).data).max() > 0
    wh.close()


# ---- 6. auto ---------------------------------------------------------------------------------------------------------
def test_auto_never_shares_outside_the_one_wave_kernels_ground(b2):
    """F != 1024, or a lone CPI per channel (a launch that would not have run rangew1k_kernel): never the new id."""
    import torch
    from blah2_amd import _lib
    keep, px, pys = cfg2_planes(torch, False, 2)
    n = CFG2[5]
    for fft_len, B in ((2048, N_CPI), (1024, 1)):
        amb = b2.Ambiguity(*CFG2, True, max_batch=2 * B)
        amb.set_fft_len(fft_len)
        assert amb.info(_lib.INFO_LAST_RANGE_KERNEL) == 0
        maps, _, rk = run_multi(torch, amb, b2.FMT_C32, px, pys, B, n)
        assert rk not in (0, _lib.RANGE_SHARED), (fft_len, B, rk)
        assert np.abs(maps).max() > 0


def test_auto_shares_exactly_where_the_measurement_won(b2):
    """profiles/r08_multi_surv_ab.json (tools/gpu_multi_surv_ab.py) is the table: at the configs[1] geometry with a batch
    that runs rangew1k_kernel, auto reports the shared kernel for the (format, K) cases recorded as wins and the one-wave
    kernel for every other one, K = 3 (not measured) included."""
    import json
    import os

    import torch
    from blah2_amd import _lib
    from conftest import ROOT
    rec = json.load(open(os.path.join(ROOT, "profiles", "r08_multi_surv_ab.json")))
    wins = {(c["format"], c["n_surv"]) for c in rec["cases"] if c["verdict"] == "win"}
    assert {(c["format"], c["n_surv"]) for c in rec["cases"]} == {(f, k) for f in ("FMT_C32", "FMT_I8") for k in (2, 4)}
    n = CFG2[5]
    for fmt_name in ("FMT_C32", "FMT_I8"):
        keep, px, pys = cfg2_planes(torch, fmt_name == "FMT_I8", 4)
        for K in (2, 3, 4):
            amb = b2.Ambiguity(*CFG2, True, max_batch=K * N_CPI)
            maps, _, rk = run_multi(torch, amb, getattr(b2, fmt_name), px, pys[:K], N_CPI, n)
            assert rk == (_lib.RANGE_SHARED if (fmt_name, K) in wins else _lib.RANGE_WAVE1K), (fmt_name, K, rk, sorted(wins))
            assert np.abs(maps).max() > 0
