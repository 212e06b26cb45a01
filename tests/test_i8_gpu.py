"""GPU: the 8-bit sample formats (BLAH2HIP_FMT_I8, BLAH2HIP_FMT_I8X_C32Y) through the C ABI.

Cross-format identity: int8 values are exact in int16 and in fp32 and the kernels differ between the formats only in
the load and the conversion, so for the same integers FMT_I8 must give the BITS FMT_I16 gives (FMT_I8X_C32Y those of
FMT_I16X_C32Y) -- for every range kernel family forced in turn, a lone CPI and a batch with cpi_stride > n, planes that
are only 2-byte aligned, odd nCorr (4761, 9767) and one-sided lag windows of both signs; likewise the clutter filter's
output, flags and taps and the spectrum.  Then the oracle's gates at the configs[1] size, the edge values, the stated
refusals and the host-plane entry."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces
CFG2 = (-10, 400, -256, 256, 2_000_000, 2_000_000)


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


def scene_i8(n, B, seed, full_scale=True):
    """int8 (x, y) [B, n, 2]: a noise-like reference, the surveillance channel an echo of it at lag 3 plus noise;
    every value of int8 occurs (-128 included) when ``full_scale``."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-128 if full_scale else -127, 128, size=(B, n, 2), dtype=np.int64)
    y = np.roll(x, 3, axis=1) // 2 + rng.integers(-40, 41, size=(B, n, 2))
    return x.astype(np.int8), np.clip(y, -128 if full_scale else -127, 127).astype(np.int8)


def guarded(torch, shape, dtype, pad=64):
    """A device buffer of ``shape`` followed by ``pad`` guard words; (whole, view)."""
    words = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size() // 4
    whole = torch.full((words + pad,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    return whole, whole[:words].view(dtype).view(shape)


def guard_intact(whole, pad=64):
    return bool((whole[-pad:].cpu().numpy().view(np.uint32) == GUARD).all())


def i8_plane(torch, a, stride):
    """int8 [B, n, 2] as a device plane with ``stride`` samples per CPI whose base is 2 bytes past a 4-byte boundary;
    the gaps hold a value (77) that a read beyond a CPI would pick up.  (keep-alive tensor, pointer)"""
    B, n, _ = a.shape
    host = np.full((B * stride + 1, 2), 77, dtype=np.int8)
    for c in range(B):
        host[1 + c * stride:1 + c * stride + n] = a[c]
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 4 == 0
    return t, t.data_ptr() + 2


def i16_words(torch, x, y, stride):
    B, n, _ = x.shape
    host = np.full((B, stride, 4), 77, dtype=np.int16)
    host[:, :n, 0:2] = x
    host[:, :n, 2:4] = y
    return torch.from_numpy(host).cuda()


def c32_plane(torch, a, stride):
    B, n, _ = a.shape
    host = np.full((B, stride), 77 + 77j, dtype=np.complex64)
    host[:, :n] = a[..., 0].astype(np.float32) + 1j * a[..., 1].astype(np.float32)
    return torch.from_numpy(host).cuda()


def make_amb(b2, geom, B, fft_len, kernel):
    from blah2_amd import _lib
    amb = b2.Ambiguity(*geom, True, max_batch=B)
    amb.set_fft_len(fft_len)
    k = {"wave1k": _lib.RANGE_WAVE1K, "wave": _lib.RANGE_WAVE, "e8": _lib.RANGE_E8, "e16": _lib.RANGE_E16, "ps": _lib.RANGE_PS}[kernel]
    amb.set_range_kernel(k)
    return amb, k


def run_fmt(b2, torch, amb, fmt, px, py, B, stride):
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    whole, out = guarded(torch, (B, nD, nC), torch.complex64)
    wm, met = guarded(torch, (B, 2), torch.float64)
    amb.process_dev(fmt, px, py, B, stride, out.data_ptr(), met.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert guard_intact(whole) and guard_intact(wm)
    from blah2_amd import _lib
    return out.cpu().numpy(), met.cpu().numpy(), amb.info(_lib.INFO_LAST_RANGE_KERNEL)


# (geometry, transform length, forced kernel): every instantiation family; nCorr 4761 and 9767 are odd, the windows
# (1, 299) and (-299, -1) one-sided (negative offsets into y for the whole window / the far range edge)
FAMILIES = [
    (CFG2, 1024, "wave1k"),                                        # rangew1k<SHORTX, OUT7, REUSE>: carried y' registers
    ((-7, 492, -50, 50, 155_540, 155_540), 1024, "wave1k"),        # <true, false>: 500 lags
    ((-5, 94, -40, 40, 240_000, 240_000), 1024, "wave1k"),         # <false, true>: long segments
    ((-10, 100, -100, 100, 1_000_000, 100_000), 1024, "wave1k"),   # odd nCorr
    ((1, 299, -50, 50, 155_540, 155_540), 1024, "wave1k"),         # delayMin > 0
    ((-299, -1, -50, 50, 155_540, 155_540), 1024, "wave1k"),       # delayMax < 0
    (CFG2, 1024, "ps"),
    ((1, 299, -100, 100, 1_000_000, 777_001), 1024, "ps"),
    ((-299, -1, -100, 100, 1_000_000, 777_001), 1024, "ps"),
    ((-10, 100, -100, 100, 1_000_000, 100_000), 1024, "ps"),       # odd nCorr
    ((-10, 100, -100, 100, 1_000_000, 100_000), 1024, "e8"),       # odd nCorr
    ((1, 299, -50, 50, 155_540, 155_540), 1024, "e8"),
    ((-299, -1, -50, 50, 155_540, 155_540), 1024, "e8"),
    (CFG2, 2048, "wave"),                                          # pruned windows
    ((-7, 492, -50, 50, 155_540, 155_540), 2048, "wave"),
    ((-299, -1, -100, 100, 1_000_000, 777_001), 2048, "wave"),
    ((1, 299, -100, 100, 1_000_000, 777_001), 2048, "wave"),
    (CFG2, 2048, "e16"),                                           # range_kernel<8>
    ((-299, -1, -50, 50, 155_540, 155_540), 2048, "e16"),
    ((-24, 2023, -64, 64, 1_260_000, 1_260_000), 4096, "e16"),     # range_kernel<16>: half-zero x segments, odd nCorr
    ((-10, 89, -20, 20, 123_000, 123_000), 4096, "e16"),           # full segments
    ((1, 99, -20, 20, 123_000, 123_000), 4096, "e16"),
]


@pytest.mark.parametrize("geom,fft_len,kernel", FAMILIES)
@pytest.mark.parametrize("B", [1, 3])
def test_i8_maps_are_bit_identical_to_int16(b2, geom, fft_len, kernel, B):
    """FMT_I8 == FMT_I16 and FMT_I8X_C32Y == FMT_I16X_C32Y, bit for bit, map and metrics, same kernel reported."""
    import torch
    n = geom[5]
    stride = n if B == 1 else n + 37  # odd gap: CPI 1 starts at an odd sample of the plane
    x, y = scene_i8(n, B, seed=(abs(sum(geom)) * 31 + fft_len + 7 * len(kernel) + B) % (1 << 31))
    amb, k = make_amb(b2, geom, B, fft_len, kernel)
    words = i16_words(torch, x, y, stride)
    tx, px = i8_plane(torch, x, stride)
    ty, py = i8_plane(torch, y, stride)
    yf = c32_plane(torch, y, stride)
    m16, met16, k16 = run_fmt(b2, torch, amb, b2.FMT_I16, words.data_ptr(), 0, B, stride)
    m8, met8, k8 = run_fmt(b2, torch, amb, b2.FMT_I8, px, py, B, stride)
    assert k16 == k8 == k
    assert np.abs(m16).max() > 0
    assert np.array_equal(m8.view(np.uint32), m16.view(np.uint32))
    assert np.array_equal(met8.view(np.uint64), met16.view(np.uint64))
    m16c, met16c, _ = run_fmt(b2, torch, amb, b2.FMT_I16X_C32Y, words.data_ptr(), yf.data_ptr(), B, stride)
    m8c, met8c, k8c = run_fmt(b2, torch, amb, b2.FMT_I8X_C32Y, px, yf.data_ptr(), B, stride)
    assert k8c == k
    assert np.array_equal(m8c.view(np.uint32), m16c.view(np.uint32))
    assert np.array_equal(met8c.view(np.uint64), met16c.view(np.uint64))


def test_i8_reports_the_planners_kernel_like_int16(b2):
    """No forced kernel: the plan depends on the geometry, not on the storage format."""
    import torch
    from blah2_amd import _lib
    for geom, B in ((CFG2, 1), (CFG2, 3), ((-10, 100, -100, 100, 1_000_000, 100_000), 2)):
        n = geom[5]
        x, y = scene_i8(n, B, seed=5 + B)
        amb = b2.Ambiguity(*geom, True, max_batch=B)
        words = i16_words(torch, x, y, n)
        tx, px = i8_plane(torch, x, n)
        ty, py = i8_plane(torch, y, n)
        m16, _, k16 = run_fmt(b2, torch, amb, b2.FMT_I16, words.data_ptr(), 0, B, n)
        m8, _, k8 = run_fmt(b2, torch, amb, b2.FMT_I8, px, py, B, n)
        assert k8 == k16 and k8 in (_lib.RANGE_WAVE1K, _lib.RANGE_PS, _lib.RANGE_E8, _lib.RANGE_WAVE, _lib.RANGE_E16)
        assert np.array_equal(m8.view(np.uint32), m16.view(np.uint32))


def test_i8_rotated_reference_channel(b2):
    """Asymmetric Doppler limits (Ambiguity.cpp:95-102): rotate_kernel<InI8> / <InI8C32> against the int16 forms."""
    import torch
    geom, B = (-10, 100, -60, 100, 1_000_000, 100_000), 2
    n = geom[5]
    x, y = scene_i8(n, B, seed=11)
    amb = b2.Ambiguity(*geom, True, max_batch=B)
    words = i16_words(torch, x, y, n + 5)
    tx, px = i8_plane(torch, x, n + 5)
    ty, py = i8_plane(torch, y, n + 5)
    yf = c32_plane(torch, y, n + 5)
    m16, _, _ = run_fmt(b2, torch, amb, b2.FMT_I16, words.data_ptr(), 0, B, n + 5)
    m8, _, _ = run_fmt(b2, torch, amb, b2.FMT_I8, px, py, B, n + 5)
    m8c, _, _ = run_fmt(b2, torch, amb, b2.FMT_I8X_C32Y, px, yf.data_ptr(), B, n + 5)
    assert np.array_equal(m8.view(np.uint32), m16.view(np.uint32)) and np.array_equal(m8c.view(np.uint32), m16.view(np.uint32))


@pytest.mark.parametrize("fft_len", [1024, 2048, 4096])
@pytest.mark.parametrize("form", ["half", "window"])
@pytest.mark.parametrize("lags", [(-10, 100), (0, 60)])
def test_i8_clutter_filter_is_bit_identical_to_int16(b2, fft_len, form, lags):
    """clutter_corr(_half)_kernel and clutter_fir_kernel at R3 = 4 / 8 / 16: filtered channel, ok flags and taps of
    process_dev_fmt(FMT_I8) and the taps of estimate_dev_fmt(FMT_I8) equal FMT_I16's, an odd sample count, stride > n."""
    import torch
    n, B = 60_001, 2
    stride = n + 11
    x, y = scene_i8(n, B, seed=fft_len + len(form) + lags[1])
    words = i16_words(torch, x, y, stride)
    tx, px = i8_plane(torch, x, stride)
    ty, py = i8_plane(torch, y, stride)
    st = torch.cuda.current_stream().cuda_stream
    got = {}
    for fmt in (b2.FMT_I16, b2.FMT_I8):
        wh = b2.WienerHopf(lags[0], lags[1], n, max_batch=B)
        wh.set_fft_len(fft_len)
        wh.set_corr_form(form)
        assert wh.fft_len == fft_len
        whole, out = guarded(torch, (B, stride), torch.complex64)
        wo, ok = guarded(torch, (B,), torch.int32)
        a = (words.data_ptr(), 0) if fmt == b2.FMT_I16 else (px, py)
        wh.process_dev_fmt(fmt, a[0], a[1], B, stride, out.data_ptr(), stride, ok.data_ptr(), st)
        torch.cuda.synchronize()
        assert guard_intact(whole) and guard_intact(wo)
        taps = [wh.read_last(c) for c in range(B)]
        ok.fill_(7)
        wh.estimate_dev_fmt(fmt, a[0], a[1], B, stride, ok.data_ptr(), st)
        torch.cuda.synchronize()
        got[fmt] = (out.cpu().numpy()[:, :n], ok.cpu().numpy(), taps, [wh.read_last(c) for c in range(B)],
                    out.cpu().numpy()[:, n:])
        wh.close()
    f16, f8 = got[b2.FMT_I16], got[b2.FMT_I8]
    assert f8[1].tolist() == [1] * B == f16[1].tolist()
    assert np.array_equal(f8[0].view(np.uint32), f16[0].view(np.uint32))
    assert (f8[4].view(np.uint32) == GUARD).all()  # nothing written between the CPIs' rows
    for taps8, taps16 in ((f8[2], f16[2]), (f8[3], f16[3])):
        for (ok8, w8, r8, b8), (ok16, w16, r16, b16) in zip(taps8, taps16):
            assert ok8 and ok16 and np.abs(w8).max() > 0
            assert np.array_equal(w8.view(np.uint32), w16.view(np.uint32))
            assert np.array_equal(r8.view(np.uint64), r16.view(np.uint64)) and np.array_equal(b8.view(np.uint64), b16.view(np.uint64))


def test_i8_spectrum_is_bit_identical_to_int16(b2):
    import torch
    n, B = 200_001, 2
    stride = n + 3
    x, y = scene_i8(n, B, seed=9)
    words = i16_words(torch, x, y, stride)
    tx, px = i8_plane(torch, x, stride)
    sp = b2.SpectrumAnalyser(n, 1000.0, max_batch=B)
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for fmt, p in ((b2.FMT_I16, words.data_ptr()), (b2.FMT_I8, px)):
        whole, out = guarded(torch, (B, sp.nSpectrum), torch.complex128)
        sp.process_dev(fmt, p, B, stride, out.data_ptr(), st)
        torch.cuda.synchronize()
        assert guard_intact(whole)
        outs.append(out.cpu().numpy())
    assert np.abs(outs[0]).max() > 0 and np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64))
    sp.close()


def clipped_scene(n, seed, fs, lo=-128):
    """The issue's scene: synth_iq at ref_amp 30, noise_amp 3, rounded and clipped to int8 per component."""
    from oracle import blah2_oracle as O
    x, y = O.synth_iq(n, seed=seed, fs=fs, targets=((37, -63.0, 0.05), (250, 120.0, 0.03)), ref_amp=30.0, noise_amp=3.0,
                      quantise=False)

    def q(v):
        a = np.stack([np.rint(v.real), np.rint(v.imag)], axis=-1)
        return np.clip(a, lo, 127).astype(np.int8), float(np.mean((a < lo) | (a > 127)))
    (xi, cx), (yi, cy) = q(x), q(y)
    return xi, yi, max(cx, cy)


def as_c128(a):
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


@pytest.mark.parametrize("filtered", [False, True])
def test_i8_oracle_parity_at_the_timed_size(b2, filtered):
    """configs[1] (2 MS/s, 1 s, 513 x 411), two CPIs in one batch, FMT_I8 (and FMT_I8X_C32Y behind the 410-tap filter)
    with the 1-D CFAR, against the fp64 oracle fed the clipped integers: the project's gates (tests/gates.py) as
    test_usrp_replay_at_the_timed_size applies them."""
    import torch
    from gates import cfar1d_margins, db_map_gate, detection_gate, map_cell_gate, margin_eps
    from oracle import blah2_oracle as O
    from test_full_chain_gpu import check_chain_map
    fs = n = 2_000_000
    B = 2
    xs, ys = [], []
    for c in range(B):
        xi, yi, clipped = clipped_scene(n, 41 + c, fs)
        print(f"\n[i8 configs[1]] cpi {c}: clipped share {clipped:.2e}")
        assert clipped < 1e-3
        xs.append(xi)
        ys.append(yi)
    x, y = np.stack(xs), np.stack(ys)
    tx, px = i8_plane(torch, x, n)
    ty, py = i8_plane(torch, y, n)
    st = torch.cuda.current_stream().cuda_stream
    amb = b2.Ambiguity(*CFG2, True, max_batch=B)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    wmap, d_map = guarded(torch, (B, nD, nC), torch.complex64)
    wmet, d_met = guarded(torch, (B, 2), torch.float64)
    if filtered:
        wh = b2.WienerHopf(-10, 400, n, max_batch=B)
        wyf, yf = guarded(torch, (B, n), torch.complex64)
        d_ok = torch.zeros(B, dtype=torch.int32, device="cuda")
        wh.process_dev_fmt(b2.FMT_I8, px, py, B, n, yf.data_ptr(), n, d_ok.data_ptr(), st)
        amb.process_dev(b2.FMT_I8X_C32Y, px, yf.data_ptr(), B, n, d_map.data_ptr(), d_met.data_ptr(), st)
    else:
        amb.process_dev(b2.FMT_I8, px, py, B, n, d_map.data_ptr(), d_met.data_ptr(), st)
    cfar = b2.CfarDetector1D(1e-5, 2, 6, 5, 15.0)
    cap = 1 << 16
    d_hits = torch.zeros((B, cap, 2), dtype=torch.float64, device="cuda")
    d_cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    cfar.process_dev(amb, B, d_hits.data_ptr(), cap, d_cnt.data_ptr(), d_map.data_ptr(), d_met.data_ptr(), st)
    torch.cuda.synchronize()
    assert guard_intact(wmap) and guard_intact(wmet)
    if filtered:
        assert guard_intact(wyf) and d_ok.cpu().tolist() == [1] * B
    maps, mets, cnts = d_map.cpu().numpy(), d_met.cpu().numpy(), d_cnt.cpu().numpy()
    d = O.ambiguity_dims(*CFG2, True)
    for c in range(B):
        x0, y0 = as_c128(x[c]), as_c128(y[c])
        tag = f"i8 configs[1] cpi {c}" + (" filtered" if filtered else "")
        if filtered:
            _, y_ref, _, _, b_ref = O.wiener_hopf(x0, y0, -10, 400, return_filter=True)
            ref = O.ambiguity_process(d, x0, y_ref)
            noise_ref, max_ref = O.map_metrics(ref)
            direct_level = np.max(np.abs(b_ref)) * (d.n_corr * d.n_doppler_bins / n)
            cell = check_chain_map(tag, maps[c], mets[c, 0], ref, noise_ref, direct_level, d.doppler, d.delay, -10, 400)
        else:
            ref = O.ambiguity_process(d, x0, y0)
            noise_ref, max_ref = O.map_metrics(ref)
            cell = map_cell_gate(maps[c], ref, noise_ref)
            dbg = db_map_gate(maps[c], mets[c, 0], ref, noise_ref)
            print(f"[{tag}] cell {cell}\n[{tag}] dB map {dbg}")
            assert cell["ok"], cell
            assert dbg["ok"], dbg
        print(f"[{tag}] metrics {mets[c]} vs {(noise_ref, max_ref)}")
        assert abs(mets[c, 0] - noise_ref) <= 1e-3 and abs(mets[c, 1] - max_ref) <= 1e-3
        recs = d_hits[c, :max(int(cnts[c]), 1)].cpu().numpy()
        det = b2.hits_to_detection(amb, recs.view(b2.HIT_DTYPE).reshape(-1), int(cnts[c]), cap)
        dl, dp, _ = O.cfar1d_fast(ref, d.delay, d.doppler, noise_ref, 1e-5, 2, 6, 5, 15.0)
        mg = cfar1d_margins(ref, 1e-5, 2, 6)
        dg = detection_gate(zip(dl, dp), zip(det.get_delay().tolist(), det.get_doppler().tolist()), mg, d.doppler, d.delay[0],
                            margin_eps(cell))
        print(f"[{tag}] detections: {dg}")
        assert dg["ok"] and dg["n_ref"] > 0, dg


def test_i8_all_zero_and_full_scale(b2):
    """An all-zero CPI: a map of zeros, the filter reports not-ok.  -128 in every component: the map the int16 words
    give (no overflow in the conversion), finite everywhere, and the lag-0 zero-Doppler cell's exact value."""
    import torch
    geom, B = (-10, 100, -100, 100, 1_000_000, 100_000), 2
    n = geom[5]
    x = np.zeros((B, n, 2), dtype=np.int8)
    x[1] = -128
    y = x.copy()
    amb = b2.Ambiguity(*geom, True, max_batch=B)
    tx, px = i8_plane(torch, x, n)
    ty, py = i8_plane(torch, y, n)
    words = i16_words(torch, x, y, n)
    m8, met8, _ = run_fmt(b2, torch, amb, b2.FMT_I8, px, py, B, n)
    m16, _, _ = run_fmt(b2, torch, amb, b2.FMT_I16, words.data_ptr(), 0, B, n)
    assert np.all(m8[0] == 0)  # (by value: a zero of either sign)
    assert np.isfinite(m8[1].view(np.float32)).all() and np.array_equal(m8.view(np.uint32), m16.view(np.uint32))
    row0 = int(np.argmin(np.abs(amb.doppler)))
    exact = amb.dims.n_used * 2.0 * 128.0 * 128.0  # sum of |(-128 - 128j)|^2 over the samples used
    assert abs(m8[1][row0, 10] - exact) <= 1e-5 * exact  # the peak-relative bound of the entry point's smoke run
    wh = b2.WienerHopf(-10, 100, n, max_batch=B)
    yf = torch.zeros((B, n), dtype=torch.complex64, device="cuda")
    ok = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    wh.process_dev_fmt(b2.FMT_I8, px, py, B, n, yf.data_ptr(), n, ok.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ok.cpu().tolist()[0] == 0  # blah2.cpp:270-273 skips such a CPI
    wh.close()


def test_i8_refusals(b2):
    """Fused FIR, long filters, NULL planes and unknown codes: the stated errors, with the format named."""
    import torch
    from blah2_amd import _lib
    n = 190_647
    st = torch.cuda.current_stream().cuda_stream
    x, y = scene_i8(n, 1, seed=3)
    tx, px = i8_plane(torch, x, n)
    ty, py = i8_plane(torch, y, n)
    amb = b2.Ambiguity(-24, 2023, -15, 15, n, n, True)
    amb.set_fft_len(4096)
    wh = b2.WienerHopf(-24, 2023, n)
    assert amb.fir_fusable(wh, b2.FMT_I16) is None          # the geometry itself is covered ...
    why = amb.fir_fusable(wh, b2.FMT_I8)                    # ... the format is not
    assert why and "FMT_I8" in why
    assert amb.fir_fusable(wh, b2.FMT_I8X_C32Y)
    d_ok = torch.zeros(1, dtype=torch.int32, device="cuda")
    wh.estimate_dev_fmt(b2.FMT_I8, px, py, 1, n, d_ok.data_ptr(), st)
    torch.cuda.synchronize()
    assert d_ok.cpu().tolist() == [1]
    amb.set_fir(wh)
    with pytest.raises(b2.Blah2HipError) as e:
        amb.process_dev(b2.FMT_I8, px, py, 1, n, None, None, st)
    assert e.value.code in (_lib.ERR_UNSUPPORTED, _lib.ERR_INVALID) and "FMT_I8" in str(e.value)
    amb.set_fir(None)
    amb.process_dev(b2.FMT_I8, px, py, 1, n, None, None, st)  # the plain kernels take it
    torch.cuda.synchronize()
    for fmt in (b2.FMT_I8, b2.FMT_I8X_C32Y):
        for args in ((None, py), (px, None)):
            with pytest.raises(b2.Blah2HipError) as e:
                amb.process_dev(fmt, args[0], args[1], 1, n, None, None, st)
            assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(b2.Blah2HipError) as e:
        amb.process_dev(6, px, py, 1, n, None, None, st)
    assert e.value.code == _lib.ERR_INVALID
    yf = torch.zeros(n, dtype=torch.complex64, device="cuda")
    for bad in ((None, py), (px, None)):
        with pytest.raises(b2.Blah2HipError) as e:
            wh.process_dev_fmt(b2.FMT_I8, bad[0], bad[1], 1, n, yf.data_ptr(), n, d_ok.data_ptr(), st)
        assert e.value.code == _lib.ERR_INVALID
        with pytest.raises(b2.Blah2HipError) as e:
            wh.estimate_dev_fmt(b2.FMT_I8, bad[0], bad[1], 1, n, d_ok.data_ptr(), st)
        assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(b2.Blah2HipError) as e:
        wh.process_dev_fmt(b2.FMT_I8X_C32Y, px, py, 1, n, yf.data_ptr(), n, d_ok.data_ptr(), st)
    assert e.value.code == _lib.ERR_INVALID
    wh.close()
    long = b2.WienerHopf(-10, 4999, n)  # 5010 taps: the long form, fp32 planes only
    for fmt, p in ((b2.FMT_I8, (px, py)), (b2.FMT_I16, (px, 0))):
        with pytest.raises(b2.Blah2HipError) as e:
            long.process_dev_fmt(fmt, p[0], p[1], 1, n, yf.data_ptr(), n, d_ok.data_ptr(), st)
        assert e.value.code == _lib.ERR_UNSUPPORTED
        assert ("FMT_I8" in str(e.value)) == (fmt == b2.FMT_I8)
        with pytest.raises(b2.Blah2HipError) as e:
            long.estimate_dev_fmt(fmt, p[0], p[1], 1, n, d_ok.data_ptr(), st)
        assert e.value.code == _lib.ERR_UNSUPPORTED
    long.close()
    sp = b2.SpectrumAnalyser(n, 1000.0)
    with pytest.raises(b2.Blah2HipError):
        sp.process_dev(b2.FMT_I8X_C32Y, px, 1, n, yf.data_ptr(), st)
    sp.close()
    torch.cuda.synchronize()


def test_i8_host_planes_equal_the_dev_path(b2):
    """blah2hip_amb_process_i8 (host planes in, one CPI) against process_dev on the same bytes: bit for bit; more
    samples than the CPI uses are legal, fewer raise like the reference's pop from an empty deque."""
    import torch
    geom = (-10, 100, -100, 100, 1_000_000, 100_000)
    n = geom[5]
    x, y = scene_i8(n, 1, seed=21)
    amb = b2.Ambiguity(*geom, True)
    m = amb.process_i8(x[0], y[0])
    tx, px = i8_plane(torch, x, n)
    ty, py = i8_plane(torch, y, n)
    md, metd, _ = run_fmt(b2, torch, amb, b2.FMT_I8, px, py, 1, n)
    assert np.abs(md).max() > 0 and np.array_equal(np.ascontiguousarray(m.data).view(np.uint32), md[0].view(np.uint32))
    m.set_metrics()
    assert abs(m.noisePower - metd[0, 0]) <= 1e-9 and abs(m.maxPower - metd[0, 1]) <= 1e-9
    with pytest.raises(RuntimeError):
        amb.process_i8(x[0][:amb.dims.n_used - 1], y[0][:amb.dims.n_used - 1])
