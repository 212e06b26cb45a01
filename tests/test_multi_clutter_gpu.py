"""GPU: the clutter filter for several surveillance channels against one reference (blah2hip_clutter_process_multi_dev_fmt).

What belongs to the reference alone -- its autocorrelation r, the spectra every b_k is formed against, the recursion on
toeplitz(r) -- is computed once per CPI; b_k, the taps w_k and the FIR are per channel.  Per channel the order of every
operation is the per-channel call's, so the acceptance test is equality of BITS with blah2hip_clutter_process_dev_fmt run
channel by channel on a handle forced to the one-workgroup (stepwise) solve.  Every channel has its own complex direct-path
gain and its own echo, so a swapped or duplicated channel cannot pass.  The samples are int8-valued: exact as int8 planes
and as fp32 planes, so both formats share inputs (and results)."""
import numpy as np
import pytest

from oracle import blah2_oracle as O

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces
Y_TOL = 1e-4                   # tests/test_clutter_gpu.py
GAIN = (0.8, 0.5j, -0.3 + 0.2j, 0.6 - 0.4j)
ECHO = ((37, -60.0, 0.05), (72, 40.0, 0.05), (15, 80.0, 0.05), (55, -20.0, 0.05))  # (delay, Doppler Hz, amplitude)
FS = 1_000_000


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


def scene(n, K, seed):
    """int8 samples [n, 2]: a noise-like reference x and K surveillance channels y_k = c_k x + a_k x[n - d_k] e^{j 2 pi f_k t}
    + noise_k, rounded and clipped like an 8-bit receiver's."""
    rng = np.random.default_rng(seed)
    x = 30.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    t = np.arange(n) / FS

    def q(v):
        return np.clip(np.stack([np.rint(v.real), np.rint(v.imag)], axis=-1), -128, 127).astype(np.int8)
    ys = []
    for k in range(K):
        d, f, a = ECHO[k]
        xd = np.roll(x, d)
        xd[:d] = 0
        ys.append(q(GAIN[k] * x + a * xd * np.exp(2j * np.pi * f * t) + 3.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))))
    return q(x), ys


def as_c128(a):
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


_scenes = {}


def checked_scenes(n, dmin, dmax, K, B, seed):
    """B CPIs of K channels; on the CPU first (once per geometry): the oracle solves every channel of CPI 0 and the filter
    removes the direct path there."""
    key = (n, dmin, dmax, K, B, seed)
    if key not in _scenes:
        cpis = [scene(n, K, seed + c) for c in range(B)]
        x, ys = cpis[0]
        for k in range(K):
            ok, yf = O.wiener_hopf(as_c128(x), as_c128(ys[k]), dmin, dmax)
            assert ok, (key, k)
            assert np.linalg.norm(yf) < 0.5 * np.linalg.norm(as_c128(ys[k])), (key, k)
        _scenes[key] = cpis
    return _scenes[key]


def guarded(torch, shape, dtype, pad=64):
    words = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size() // 4
    whole = torch.full((words + pad,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    return whole, whole[:words].view(dtype).view(shape)


def guard_intact(whole, pad=64):
    return bool((whole[-pad:].cpu().numpy().view(np.uint32) == GUARD).all())


def plane(torch, fmt_i8, cpis, stride):
    """int8 CPIs [B][n, 2] as a device plane of ``stride`` samples per CPI (int8 pairs, or the same values as complex
    fp32); the gaps hold a value a read beyond a CPI would pick up."""
    B, n = len(cpis), cpis[0].shape[0]
    if fmt_i8:
        host = np.full((B, stride, 2), 77, dtype=np.int8)
        for c in range(B):
            host[c, :n] = cpis[c]
    else:
        host = np.full((B, stride), 77 + 77j, dtype=np.complex64)
        for c in range(B):
            host[c, :n] = cpis[c][:, 0].astype(np.float32) + 1j * cpis[c][:, 1].astype(np.float32)
    return torch.from_numpy(host).cuda()


def planes(torch, fmt_i8, cpis, K, stride):
    tx = plane(torch, fmt_i8, [c[0] for c in cpis], stride)
    tys = [plane(torch, fmt_i8, [c[1][k] for c in cpis], stride) for k in range(K)]
    return tx, tys


def stream(torch):
    return torch.cuda.current_stream().cuda_stream


def run_multi(torch, wh, fmt, tx, tys, B, stride, n, outs=None):
    """One multi call into guarded planes.  Returns (filtered [K][B][stride] as uint32 words incl. the gaps, ok [K, B],
    per virtual CPI (ok, w, r, b))."""
    K = len(tys)
    keep = [guarded(torch, (B, stride), torch.complex64) for _ in range(K)]
    wo, ok = guarded(torch, (K, B), torch.int32)
    youts = [o.data_ptr() for _, o in keep] if outs is None else outs
    wh.process_multi_dev(fmt, tx.data_ptr(), [t.data_ptr() for t in tys], B, stride, youts, stride, ok.data_ptr(), stream(torch))
    torch.cuda.synchronize()
    assert all(guard_intact(w) for w, _ in keep) and guard_intact(wo)
    got = [o.cpu().numpy().view(np.uint32).reshape(B, stride, 2) for _, o in keep]
    return got, ok.cpu().numpy(), [wh.read_last(v) for v in range(K * B)]


def run_single(torch, wh, fmt, tx, ty, B, stride):
    whole, out = guarded(torch, (B, stride), torch.complex64)
    wo, ok = guarded(torch, (B,), torch.int32)
    wh.process_dev_fmt(fmt, tx.data_ptr(), ty.data_ptr(), B, stride, out.data_ptr(), stride, ok.data_ptr(), stream(torch))
    torch.cuda.synchronize()
    assert guard_intact(whole) and guard_intact(wo)
    return out.cpu().numpy().view(np.uint32).reshape(B, stride, 2), ok.cpu().numpy(), [wh.read_last(c) for c in range(B)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.complex128 else np.uint32)


def assert_channel_bits(multi, k, B, single, tag):
    got, okm, reads = multi
    out1, ok1, reads1 = single
    assert np.array_equal(okm[k], ok1), tag
    assert np.array_equal(got[k], out1), tag  # the CPIs and the untouched gaps between them
    for c in range(B):
        (o_m, w_m, r_m, b_m), (o_1, w_1, r_1, b_1) = reads[k * B + c], reads1[c]
        assert o_m == o_1, (tag, c)
        assert np.array_equal(bits(r_m), bits(r_1)), (tag, c, "r")
        assert np.array_equal(bits(b_m), bits(b_1)), (tag, c, "b")
        assert np.array_equal(bits(w_m), bits(w_1)), (tag, c, "w")
        assert np.array_equal(bits(r_m), bits(reads[c][2])), (tag, c, "r is the reference's: one per CPI")


def stepwise(b2, dmin, dmax, n, B, corr, fft_len=None):
    wh = b2.WienerHopf(dmin, dmax, n, max_batch=B)
    if fft_len:
        wh.set_fft_len(fft_len)
    if corr:
        wh.set_corr_form(corr)
    wh.set_solve_form("stepwise")
    return wh


# ---- 1. the per-channel call, bit for bit ----------------------------------------------------------------------------
# The planner weighs F log F per useful sample, and at 110 taps that puts F = 2048 a little ahead of F = 1024; the F = 1024
# kernels are reached by asking for that length (set_fft_len), on both handles.  The planner's own choice is a case as well.
#        n, delayMin, delayMax, correlation form, transform length asked for, transform length planned
GEOMS = [(20_000, -10, 100, None, 1024, 1024),    # 110 taps: windowed, F = 1024
         (20_000, -10, 100, None, None, 2048),    # 110 taps as planned: windowed, F = 2048 (the form of 410 taps at n = 2e6)
         (50_000, -7, 293, "half", None, None),   # 300 taps, the half-window form forced
         (20_000, -7, 2040, None, None, 4096),    # 2047 taps: F = 4096 half-window, two indices per thread in the solve
         (20_000, -7, 2093, None, None, 4096),    # 2100 taps: the R3 = 16 windowed instantiation, four indices per thread
         (4_099, -7, 1018, None, None, 2048)]     # 1025 taps, half-window on F = 2048: a CPI that ends in a segment of three samples
GEOM_IDS = ["110-window-1024", "110-window", "300-half", "2047-half-4096", "2100-window-4096", "1025-short"]


@pytest.mark.parametrize("fmt_name", ["FMT_C32", "FMT_I8"])
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_bits_of_the_per_channel_call(b2, geom, fmt_name):
    """K = 3, n_cpi = 2: r (one per CPI, identical across the channels), b_k, w_k, ok and the filtered planes equal, as
    uint32 / uint64 views, those of blah2hip_clutter_process_dev_fmt per channel on a handle forced to the stepwise solve."""
    import torch
    from blah2_amd import _lib
    n, dmin, dmax, corr, ask, F = geom
    K, B, stride = 3, 2, n + 37
    fmt = getattr(b2, fmt_name)
    cpis = checked_scenes(n, dmin, dmax, K, B, 500 + dmax)
    tx, tys = planes(torch, fmt == b2.FMT_I8, cpis, K, stride)
    wh = stepwise(b2, dmin, dmax, n, B, corr, ask)
    if F:
        assert wh.fft_len == F
    multi = run_multi(torch, wh, fmt, tx, tys, B, stride, n)
    assert wh.solve_info()["form"] == _lib.CLUTTER_SOLVE_STEPWISE
    assert multi[1].tolist() == [[1] * B] * K
    wh1 = stepwise(b2, dmin, dmax, n, B, corr, ask)
    assert wh1.fft_len == wh.fft_len
    for k in range(K):
        single = run_single(torch, wh1, fmt, tx, tys[k], B, stride)
        assert_channel_bits(multi, k, B, single, (geom, fmt_name, k))
    # the channels differ: no channel's taps or plane is a copy of another's
    assert not np.array_equal(bits(multi[2][0][1]), bits(multi[2][B][1]))
    assert not np.array_equal(multi[0][0], multi[0][1])


# ---- 2. the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,taps", [(300_000, 700), (100_000, 110)])
def test_every_channel_against_the_oracle(b2, n, taps):
    import torch
    K, B = 3, 1
    dmin, dmax = -7, taps - 7
    x, ys = scene(n, K, 40 + taps)
    tx, tys = planes(torch, False, [(x, ys)], K, n)
    wh = b2.WienerHopf(dmin, dmax, n)
    got, ok, reads = run_multi(torch, wh, b2.FMT_C32, tx, tys, B, n, n)
    assert ok.tolist() == [[1]] * K
    for k in range(K):
        ok_ref, y_ref, w_ref, r_ref, b_ref = O.wiener_hopf(as_c128(x), as_c128(ys[k]), dmin, dmax, return_filter=True)
        assert ok_ref
        _, w, r, b = reads[k]
        yf = got[k].view(np.float32).reshape(B, n, 2)[0]
        yf = yf[:, 0].astype(np.float64) + 1j * yf[:, 1].astype(np.float64)
        er = np.max(np.abs(r - r_ref)) / np.abs(r_ref[0])
        eb = np.max(np.abs(b - b_ref)) / np.max(np.abs(b_ref))
        ey = np.max(np.abs(yf - y_ref)) / np.max(np.abs(y_ref))
        print(f"\n[multi clutter n={n} taps={taps} channel {k}] r {er:.2e}  b {eb:.2e}  y {ey:.2e}")
        assert er <= 1e-5 and eb <= 1e-5
        assert ey <= Y_TOL
        assert np.linalg.norm(yf) < 0.5 * np.linalg.norm(as_c128(ys[k]))


# ---- 3. a matrix that is not positive definite -----------------------------------------------------------------------
@pytest.mark.parametrize("fmt_name", ["FMT_C32", "FMT_I8"])
def test_failure_contract(b2, fmt_name):
    """n_cpi = 2, K = 2, the reference of CPI 1 all zero: ok[k][1] = 0 for both channels, their output for CPI 1 still holds
    the guard pattern, its taps are zero, and CPI 0 is the two-good-CPI run's bits."""
    import torch
    n, dmin, dmax = 20_000, -10, 100
    K, B, stride = 2, 2, n + 37
    fmt = getattr(b2, fmt_name)
    cpis = checked_scenes(n, dmin, dmax, K, B, 77)
    bad = [cpis[0], (np.zeros_like(cpis[1][0]), cpis[1][1])]
    wh = b2.WienerHopf(dmin, dmax, n, max_batch=B)
    tx, tys = planes(torch, fmt == b2.FMT_I8, cpis, K, stride)
    good = run_multi(torch, wh, fmt, tx, tys, B, stride, n)
    assert good[1].tolist() == [[1, 1], [1, 1]]
    txb, tysb = planes(torch, fmt == b2.FMT_I8, bad, K, stride)
    got, ok, reads = run_multi(torch, wh, fmt, txb, tysb, B, stride, n)
    assert ok.tolist() == [[1, 0], [1, 0]]
    for k in range(K):
        assert (got[k][1] == GUARD).all(), k
        assert np.array_equal(got[k][0], good[0][k][0]), k
        assert not reads[k * B + 1][0] and not reads[k * B + 1][1].any()
        assert np.array_equal(bits(reads[k * B][1]), bits(good[2][k * B][1]))


# ---- 4. edges of the interface ---------------------------------------------------------------------------------------
def test_one_channel_is_the_single_call(b2):
    import torch
    n, dmin, dmax = 20_000, -10, 100
    B, stride = 2, n + 37
    cpis = checked_scenes(n, dmin, dmax, 3, B, 510)
    for fmt in (b2.FMT_C32, b2.FMT_I8):
        tx, tys = planes(torch, fmt == b2.FMT_I8, cpis, 1, stride)
        wh = stepwise(b2, dmin, dmax, n, B, None)
        multi = run_multi(torch, wh, fmt, tx, tys, B, stride, n)
        single = run_single(torch, wh, fmt, tx, tys[0], B, stride)
        assert_channel_bits(multi, 0, B, single, fmt)


def test_in_place_estimate_only_and_a_smaller_second_call(b2):
    """FMT_C32 with d_y_out[k] == d_y[k]; d_y_out = NULL leaves the taps in the handle (taps_dev, virtual CPIs); a second
    call on the same handle with fewer channels."""
    import torch
    n, dmin, dmax = 20_000, -10, 100
    K, B, stride = 3, 2, n + 37
    cpis = checked_scenes(n, dmin, dmax, K, B, 510)
    tx, tys = planes(torch, False, cpis, K, stride)
    wh = b2.WienerHopf(dmin, dmax, n, max_batch=B)
    ref = run_multi(torch, wh, b2.FMT_C32, tx, tys, B, stride, n)
    taps_ref = np.stack([ref[2][v][1] for v in range(K * B)])
    # in place
    mine = [t.clone() for t in tys]
    ok = torch.zeros((K, B), dtype=torch.int32, device="cuda")
    ptrs = [t.data_ptr() for t in mine]
    wh.process_multi_dev(b2.FMT_C32, tx.data_ptr(), ptrs, B, stride, ptrs, stride, ok.data_ptr(), stream(torch))
    torch.cuda.synchronize()
    assert ok.cpu().numpy().tolist() == [[1] * B] * K
    for k in range(K):
        inplace = mine[k].cpu().numpy().view(np.uint32).reshape(B, stride, 2)
        assert np.array_equal(inplace[:, :n], ref[0][k][:, :n]), k
        assert np.array_equal(inplace[:, n:], tys[k].cpu().numpy().view(np.uint32).reshape(B, stride, 2)[:, n:]), k  # the gaps
    # estimate only, on a fresh handle: the taps through the device pointer
    wh2 = b2.WienerHopf(dmin, dmax, n, max_batch=B)
    wh2.process_multi_dev(b2.FMT_C32, tx.data_ptr(), [t.data_ptr() for t in tys], B, stride, None, 0, None, stream(torch))
    torch.cuda.synchronize()
    p, nb, dm = wh2.taps_dev()
    assert (nb, dm) == (dmax - dmin, dmin) and p
    import ctypes
    from blah2_amd import _lib
    host = np.empty((K * B, nb), dtype=np.complex64)
    L, ctx = _lib.load(), ctypes.c_void_p()
    assert L.blah2hip_ctx_create(0, ctypes.byref(ctx)) == 0
    assert L.blah2hip_ctx_d2h(ctx, host.ctypes.data, p, host.nbytes) == 0 and L.blah2hip_ctx_sync(ctx) == 0
    L.blah2hip_ctx_destroy(ctx)
    assert np.array_equal(bits(host), bits(taps_ref))
    assert all(wh2.read_last(v)[0] for v in range(K * B))
    # fewer channels on the handle that has run three: channels 2 and 0, in that order
    again = run_multi(torch, wh, b2.FMT_C32, tx, [tys[2], tys[0]], B, stride, n)
    for j, k in enumerate((2, 0)):
        assert np.array_equal(again[0][j], ref[0][k]), k
        for c in range(B):
            for u, v in zip(again[2][j * B + c][1:], ref[2][k * B + c][1:]):
                assert np.array_equal(bits(u), bits(v)), (k, c)
    with pytest.raises(b2.Blah2HipError):
        wh.read_last(2 * B)  # virtual CPIs of the last call: 2 channels x 2 CPIs


def test_refusals_name_their_cause_and_leave_the_handle_usable(b2):
    import torch
    from blah2_amd import _lib
    n, dmin, dmax = 20_000, -10, 100
    K, B, stride = 3, 2, n + 37
    cpis = checked_scenes(n, dmin, dmax, K, B, 510)
    tx, tys = planes(torch, False, cpis, K, stride)
    wh = b2.WienerHopf(dmin, dmax, n, max_batch=B)
    good = run_multi(torch, wh, b2.FMT_C32, tx, tys, B, stride, n)
    pys = [t.data_ptr() for t in tys]
    out = torch.zeros((K, B, stride), dtype=torch.complex64, device="cuda")
    pout = [out[k].data_ptr() for k in range(K)]

    def refused(code, word, fmt, ys, outs, n_cpi):
        with pytest.raises(b2.Blah2HipError) as e:
            wh.process_multi_dev(fmt, tx.data_ptr(), ys, n_cpi, stride, outs, stride, None, stream(torch))
        assert e.value.code == code and word in str(e.value), str(e.value)

    refused(_lib.ERR_UNSUPPORTED, "FMT_I16", b2.FMT_I16, pys, pout, B)
    refused(_lib.ERR_INVALID, "n_surv", b2.FMT_C32, [], [], B)
    refused(_lib.ERR_INVALID, "MAX_SURV", b2.FMT_C32, [pys[0]] * 9, [pout[0]] * 9, 1)
    refused(_lib.ERR_INVALID, "NULL surveillance plane 1", b2.FMT_C32, [pys[0], None, pys[2]], pout, B)
    refused(_lib.ERR_INVALID, "NULL output plane 2", b2.FMT_C32, pys, [pout[0], pout[1], None], B)
    refused(_lib.ERR_INVALID, "max_batch", b2.FMT_C32, pys, pout, B + 1)
    refused(_lib.ERR_INVALID, "max_batch", b2.FMT_C32, pys, pout, 0)
    refused(_lib.ERR_INVALID, "BLAH2HIP_FMT_C32 or BLAH2HIP_FMT_I8", b2.FMT_F16, pys, pout, B)
    again = run_multi(torch, wh, b2.FMT_C32, tx, tys, B, stride, n)  # a valid call on the same handle still works
    for k in range(K):
        assert np.array_equal(again[0][k], good[0][k])


# ---- 5. into the multi-channel ambiguity stage -----------------------------------------------------------------------
def test_chain_into_the_multi_channel_maps(b2):
    """The new call feeding blah2hip_amb_process_multi_dev(FMT_I8X_C32Y): maps and metrics are the bits of the chain fed by
    the per-channel stepwise filter."""
    import torch
    SMALL = (-10, 100, -100, 100, 1_000_000, 100_000)
    n, K, B = SMALL[5], 3, 2
    stride = n + 37
    cpis = checked_scenes(n, -10, 100, K, B, 900)
    tx, tys = planes(torch, True, cpis, K, stride)
    st = stream(torch)
    amb = b2.Ambiguity(*SMALL, True, max_batch=K * B)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()

    def maps_of(filtered):
        wm, maps = guarded(torch, (K * B, nD, nC), torch.complex64)
        wt, met = guarded(torch, (K * B, 2), torch.float64)
        amb.process_multi_dev(b2.FMT_I8X_C32Y, tx.data_ptr(), [f.data_ptr() for f in filtered], B, stride, maps.data_ptr(),
                              met.data_ptr(), st)
        torch.cuda.synchronize()
        assert guard_intact(wm) and guard_intact(wt)
        return maps.cpu().numpy().view(np.uint32), met.cpu().numpy().view(np.uint64)

    wh = b2.WienerHopf(-10, 100, n, max_batch=B)
    f_multi = [torch.zeros((B, stride), dtype=torch.complex64, device="cuda") for _ in range(K)]
    ok = torch.zeros((K, B), dtype=torch.int32, device="cuda")
    wh.process_multi_dev(b2.FMT_I8, tx.data_ptr(), [t.data_ptr() for t in tys], B, stride, [f.data_ptr() for f in f_multi], stride,
                         ok.data_ptr(), st)
    maps_m, met_m = maps_of(f_multi)
    assert ok.cpu().numpy().all()
    wh1 = stepwise(b2, -10, 100, n, B, None)
    f_single = [torch.zeros((B, stride), dtype=torch.complex64, device="cuda") for _ in range(K)]
    for k in range(K):
        wh1.process_dev_fmt(b2.FMT_I8, tx.data_ptr(), tys[k].data_ptr(), B, stride, f_single[k].data_ptr(), stride, None, st)
    maps_s, met_s = maps_of(f_single)
    assert maps_m.any() and np.array_equal(maps_m, maps_s) and np.array_equal(met_m, met_s)
    assert not np.array_equal(maps_m[0], maps_m[B])
