"""Crafted inputs and the one harness of tests/test_clutter_edge_cases_gpu.py: distinct CPIs with clutter inside the lag
window, guarded device planes, one run of the filter with the plan forced and asserted, and the comparison with the fp64
oracle (oracle.blah2_oracle.wiener_hopf, which evaluates the reference's uint32 index of the shifted channel).

No GPU is touched at import; torch is imported inside the functions that need it."""
import numpy as np

from oracle import blah2_oracle as O

FS = 1_000_000
GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces
GAP = 3                        # output stride n + 3: three untouched samples behind every row
IN_GAP = 5                     # input stride n + 5; the gap holds values a read beyond a CPI would pick up
R_TOL, B_TOL, Y_TOL = 1e-5, 1e-5, 1e-4  # tests/test_clutter_gpu.py


def echo_delays(dmin, dmax, n):
    """(delay, Doppler Hz, amplitude): 0 Hz 0.3 two taps into the window, 0 Hz 0.2 mid-window, one mover a third in."""
    def red(d):
        return int(np.fmod(d, n)) if abs(d) >= n else d
    return ((red(dmin + 2), 0.0, 0.3), (red((dmin + dmax) // 2), 0.0, 0.2), (red(dmin + (dmax - dmin) // 3), 40.0, 0.05))


def clip8(v):
    return np.clip(v.real, -128, 127) + 1j * np.clip(v.imag, -128, 127)


_cpis = {}


def cpis_for(dmin, dmax, n, B, i8=False, zero_ref=()):
    """B distinct int16-valued CPIs (x, y) as complex128 (int8-valued when ``i8``); ``zero_ref``: CPIs whose reference is zero."""
    key = (dmin, dmax, n, B, i8, tuple(zero_ref))
    if key not in _cpis:
        out = []
        for c in range(B):
            x, y = O.synth_iq(n, seed=7000 + 131 * c + n % 97 + (dmax - dmin), fs=FS, targets=echo_delays(dmin, dmax, n))
            x, y = x + 0.0, y + 0.0  # no negative zeros (rint of -0.3): int16 -> fp32 cannot produce one, an fp32 plane would carry it
            if i8:
                x, y = clip8(x), clip8(y)
            if c in zero_ref:
                x = np.zeros_like(x)
            out.append((x, y))
        _cpis[key] = out
    return _cpis[key]


_refs = {}


def oracle_for(key, c, x, y, dmin, dmax):
    """(ok, y_ref, w, r, b) of one CPI, computed once per module run and left unchanged."""
    k = (key, c)
    if k not in _refs:
        _refs[k] = O.wiener_hopf(x, y, dmin, dmax, return_filter=True)
    return _refs[k]


def guarded(torch, shape, dtype, pad=64):
    words = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size() // 4
    whole = torch.full((words + pad,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    return whole, whole[:words].view(dtype).view(shape)


def guard_intact(whole, pad=64):
    return bool((whole[-pad:].cpu().numpy().view(np.uint32) == GUARD).all())


def device_inputs(torch, b2, fmt, chans):
    """chans: [B] of (x, y) -> (d_x, d_y) in format ``fmt`` with IN_GAP samples of filler behind every CPI."""
    B, n = len(chans), chans[0][0].shape[0]
    stride = n + IN_GAP
    if fmt == b2.FMT_I16:
        host = np.full((B, stride, 4), 7777, dtype=np.int16)
        for c, (x, y) in enumerate(chans):
            host[c, :n] = np.stack([x.real, x.imag, y.real, y.imag], axis=-1)
        return torch.from_numpy(host).cuda(), None, stride
    planes = []
    for which in (0, 1):
        if fmt == b2.FMT_I8:
            host = np.full((B, stride, 2), 77, dtype=np.int8)
            for c in range(B):
                v = chans[c][which]
                host[c, :n] = np.stack([v.real, v.imag], axis=-1)
        else:
            host = np.full((B, stride), 7777 + 7777j, dtype=np.complex64)
            for c in range(B):
                host[c, :n] = chans[c][which]
        planes.append(torch.from_numpy(host).cuda())
    return planes[0], planes[1], stride


def planned(b2, dmin, dmax, n, B, corr_form=None, fft_len=None, carry=None, solve=None):
    """A handle with the plan forced, and the proof (through the handle) that it is the plan that runs."""
    wh = b2.WienerHopf(dmin, dmax, n, max_batch=B)
    if fft_len:
        wh.set_fft_len(fft_len)
    if corr_form:
        wh.set_corr_form(corr_form)
    if carry is not None:
        wh.set_fir_carry(carry)
    if solve:
        wh.set_solve_form(solve)
    wh._refresh_dims()
    info = wh.plan_info()
    if fft_len:
        assert wh.fft_len == fft_len
    if corr_form:
        assert info["corr"] == corr_form
    if carry is not None:
        assert info["carry"] == carry
        nb = dmax - dmin
        assert wh.seg_len == (wh.fft_len // 2 if carry else wh.fft_len - nb + 1)
    return wh


def run_filter(b2, wh, fmt, chans, reps=1):
    """process_dev_fmt into guarded planes of stride n + 3.  Returns per repetition (filtered rows as uint32 words incl. the
    gaps [B, n + 3, 2], ok [B], [(ok, w, r, b)] per CPI); guards are asserted."""
    import torch
    B, n = len(chans), chans[0][0].shape[0]
    dx, dy, stride = device_inputs(torch, b2, fmt, chans)
    st = torch.cuda.current_stream().cuda_stream
    runs = []
    for _ in range(reps):
        whole, out = guarded(torch, (B, n + GAP), torch.complex64)
        wo, ok = guarded(torch, (B,), torch.int32)
        wh.process_dev_fmt(fmt, dx.data_ptr(), dy.data_ptr() if dy is not None else None, B, stride, out.data_ptr(), n + GAP,
                           ok.data_ptr(), st)
        torch.cuda.synchronize()
        assert guard_intact(whole) and guard_intact(wo)
        words = out.cpu().numpy().view(np.uint32).reshape(B, n + GAP, 2)
        assert (words[:, n:] == GUARD).all(), "the three gap samples behind a row were written"
        runs.append((words, ok.cpu().numpy().copy(), [wh.read_last(c) for c in range(B)]))
    return runs if reps > 1 else runs[0]


def as_c128(words, n):
    v = np.ascontiguousarray(words[:, :n]).view(np.float32)
    return v[..., 0].astype(np.float64) + 1j * v[..., 1].astype(np.float64)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.complex128 else np.uint32)


def assert_same_bits(u, v, tag):
    """Two runs (run_filter's tuples): filtered rows, ok, r, b and the taps as bit patterns."""
    assert np.array_equal(u[0], v[0]), (tag, "filtered channel")
    assert np.array_equal(u[1], v[1]), (tag, "ok")
    for c, (a, b) in enumerate(zip(u[2], v[2])):
        assert a[0] == b[0], (tag, c)
        for name, p, q in zip("wrb", a[1:], b[1:]):
            assert np.array_equal(bits(p), bits(q)), (tag, c, name)


def check_oracle(run, chans, key, dmin, dmax, tag, cpis=None):
    """Every CPI (or ``cpis``) of a run against the oracle: ok, r, b, the filtered channel."""
    words, okv, reads = run
    n = chans[0][0].shape[0]
    yf = as_c128(words, n)
    for c in (range(len(chans)) if cpis is None else cpis):
        ok_ref, y_ref, w_ref, r_ref, b_ref = oracle_for(key, c, chans[c][0], chans[c][1], dmin, dmax)
        assert ok_ref, (tag, c, "the oracle's ok")
        assert okv[c] == 1 and reads[c][0], (tag, c, okv)
        _, w, r, b = reads[c]
        er = np.max(np.abs(r - r_ref)) / np.abs(r_ref[0])
        eb = np.max(np.abs(b - b_ref)) / np.max(np.abs(b_ref))
        ey = np.max(np.abs(yf[c] - y_ref)) / np.max(np.abs(y_ref))
        ew = np.max(np.abs(w - w_ref)) / np.max(np.abs(w_ref))
        print(f"\n[clutter edge {tag} cpi {c}] r {er:.2e}  b {eb:.2e}  y {ey:.2e}  w {ew:.2e}")
        assert er <= R_TOL, (tag, c, "r", er)
        assert eb <= B_TOL, (tag, c, "b", eb)
        assert ey <= Y_TOL, (tag, c, "y", ey)
