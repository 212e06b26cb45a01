"""GPU: the clutter filter with taps per block (blah2hip_clutter_create_ex, n_blocks > 1) through the C ABI, against the fp64
restatement of tests/clutter_blocks_ref.py (taps per block from the oracle on the block alone, one continuous convolution over
the CPI-level shifted channel).

Every case: int16-valued CPIs with clutter inside the lag window (tests/clutter_crafted.py), guarded planes, input stride
n + 5 and output stride n + 3 unless a case says otherwise, then per virtual CPI v = c * blocks + j
    max|r - r_ref| / |r_ref[0]| <= 1e-5,  max|b - b_ref| / max|b_ref| <= 1e-5        (R_TOL, B_TOL)
and per CPI  max|yf - y_ref| / max|y_ref| <= 1e-4 (Y_TOL) -- the gates of tests/test_clutter_gpu.py -- ok flags, guards and
gaps intact.  The first nBins - 1 outputs of every block j > 0 are checked on their own: a history that restarted with zeros
at the block edge is wrong exactly there (asserted on the inputs: the block filtered alone misses the gate on those samples).

Measured on an MI355X, worst over the CPIs of a case (r, b, yf, the blocks' first nBins - 1 outputs; gates 1e-5, 1e-5, 1e-4, 1e-4):
    N 8192 / 4 blocks, F = 1024, delayMin 0 / -3 / 2      8.4e-8 1.2e-7 1.2e-6 7.1e-7 / 9.5e-8 1.2e-7 3.3e-7 2.4e-7 / 8.6e-8 1.4e-7 9.0e-8 7.0e-8
    N 4096 / 8 blocks (L = 512 < F), 16 / 400 taps         8.8e-8 1.3e-7 1.6e-6 1.1e-6 / 8.5e-17 5.9e-17 2.8e-7 2.8e-7 (400 taps: fp64 lag sums)
    N 4096 / 8 blocks, 300 taps from lag -3 (fp64 lag sums) 1.7e-16 1.1e-16 3.4e-7 3.4e-7; int8 1.4e-16 8.9e-17 2.2e-7; transforms forced 1.7e-7 1.9e-7 2.3e-6
    2047 taps, N 16384 / 2                                 1.2e-7 1.2e-7 1.3e-6 1.3e-6
    2047 taps, N 8188 / 4 (L = nBins, fp64 lag sums)       3.3e-16 2.0e-16 2.3e-7 2.3e-7 (9.6e-3 on the transforms' fp32 partials: see test_2047_taps)
    3 CPIs, both launch forms                              1.3e-7 1.2e-7 1.2e-6 7.3e-7 (equal bits between the forms and between calls)
    33 CPIs of 8 blocks (264 systems, N 1024)              1.7e-7 1.8e-7 1.7e-6 1.6e-6; the solve on E = 2, one workgroup per system
    int16 words / int8 planes                              9.9e-8 1.2e-7 3.3e-7 2.4e-7 / 1.2e-7 7.1e-8 1.9e-7 1.4e-7
    scene: residual -9.12 dB with one tap set, -24.91 dB with 16 blocks (the restatement: -24.91 dB)"""
import ctypes as C

import numpy as np
import pytest

import clutter_blocks_ref as R
import clutter_crafted as cc
from oracle import blah2_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


_refs = {}


def refs_for(chans, dmin, dmax, blocks, key):
    """[(ok [blocks], y_ref, w, r, b)] per CPI, computed once per module run and left unchanged."""
    k = (key, dmin, dmax, blocks, len(chans))
    if k not in _refs:
        _refs[k] = [R.wiener_hopf_blocks(x, y, dmin, dmax, blocks) for x, y in chans]
    return _refs[k]


def handle(b2, dmin, dmax, n, blocks, B, fft_len=None):
    wh = b2.WienerHopf(dmin, dmax, n, max_batch=B, blocks=blocks)
    if fft_len:
        wh.set_fft_len(fft_len)
        assert wh.fft_len == fft_len
    v = C.c_int64(0)
    b2._lib.check(b2.load().blah2hip_clutter_get_info(wh._h, b2._lib.CLUTTER_INFO_BLOCKS, C.byref(v)))
    assert v.value == blocks
    if blocks > 1:
        assert wh.plan_info()["carry"] is False  # the block FIR reads every window whole
    return wh


def device_inputs(torch, b2, fmt, chans, stride):
    """cc.device_inputs with the stride a parameter (stride == n: CPIs back to back)."""
    B, n = len(chans), chans[0][0].shape[0]
    if fmt == b2.FMT_I16:
        host = np.full((B, stride, 4), 7777, dtype=np.int16)
        for c, (x, y) in enumerate(chans):
            host[c, :n] = np.stack([x.real, x.imag, y.real, y.imag], axis=-1)
        return torch.from_numpy(host).cuda(), None
    planes = []
    for which in (0, 1):
        if fmt == b2.FMT_I8:
            host = np.full((B, stride, 2), 77, dtype=np.int8)
            for c in range(B):
                host[c, :n] = np.stack([chans[c][which].real, chans[c][which].imag], axis=-1)
        else:
            host = np.full((B, stride), 7777 + 7777j, dtype=np.complex64)
            for c in range(B):
                host[c, :n] = chans[c][which]
        planes.append(torch.from_numpy(host).cuda())
    return planes[0], planes[1]


def run(b2, wh, fmt, chans, blocks, stride=None, in_place=False, reps=1):
    """process_dev_fmt into guarded planes.  Per repetition: (filtered rows as uint32 words [B, n + GAP, 2] (in place: the
    rows of the y plane, [B, stride, 2]), ok [B * blocks], [(ok, w, r, b)] per virtual CPI)."""
    import torch
    B, n = len(chans), chans[0][0].shape[0]
    stride = n + cc.IN_GAP if stride is None else stride
    st = torch.cuda.current_stream().cuda_stream
    runs = []
    for _ in range(reps):
        dx, dy = device_inputs(torch, b2, fmt, chans, stride)
        wo, ok = cc.guarded(torch, (B * blocks,), torch.int32)
        if in_place:
            assert fmt == b2.FMT_C32
            wh.process_dev_fmt(fmt, dx.data_ptr(), dy.data_ptr(), B, stride, dy.data_ptr(), stride, ok.data_ptr(), st)
            torch.cuda.synchronize()
            words = dy.cpu().numpy().view(np.uint32).reshape(B, stride, 2)
            filler = np.array([7777 + 7777j], dtype=np.complex64).view(np.uint32)
            assert (words[:, n:] == filler).all(), "the gap behind an in-place row was written"
        else:
            whole, out = cc.guarded(torch, (B, n + cc.GAP), torch.complex64)
            wh.process_dev_fmt(fmt, dx.data_ptr(), dy.data_ptr() if dy is not None else None, B, stride, out.data_ptr(),
                               n + cc.GAP, ok.data_ptr(), st)
            torch.cuda.synchronize()
            assert cc.guard_intact(whole)
            words = out.cpu().numpy().view(np.uint32).reshape(B, n + cc.GAP, 2)
            assert (words[:, n:] == cc.GUARD).all(), "the three gap samples behind a row were written"
        assert cc.guard_intact(wo)
        runs.append((words, ok.cpu().numpy().copy(), [wh.read_last(v) for v in range(B * blocks)]))
    return runs if reps > 1 else runs[0]


def same_bits(u, v, tag, n):
    assert np.array_equal(u[0][:, :n], v[0][:, :n]), (tag, "filtered channel")
    assert np.array_equal(u[1], v[1]), (tag, "ok")
    for c, (a, b) in enumerate(zip(u[2], v[2])):
        assert a[0] == b[0], (tag, c)
        for name, p, q in zip("wrb", a[1:], b[1:]):
            assert np.array_equal(cc.bits(p), cc.bits(q)), (tag, c, name)


def check(run_, chans, refs, dmin, dmax, blocks, tag, ok_expect=None):
    """A run against the restatement: ok, r and b per virtual CPI, the filtered channel per CPI, and the first nBins - 1
    outputs of the blocks behind the first on their own."""
    words, okv, reads = run_
    n, nb = chans[0][0].shape[0], dmax - dmin
    L = n // blocks
    yf = cc.as_c128(words, n)
    for c, (x, y) in enumerate(chans):
        ok_ref, y_ref, _, r_ref, b_ref = refs[c]
        want = ok_ref if ok_expect is None else np.asarray(ok_expect, dtype=bool)
        assert np.array_equal(ok_ref, want), (tag, c, "the restatement's ok", ok_ref)
        worst = [0.0, 0.0]
        for j in range(blocks):
            v = c * blocks + j
            assert bool(okv[v]) == bool(want[j]) and reads[v][0] == bool(want[j]), (tag, c, j, okv)
            _, _, r, b = reads[v]
            if not want[j]:
                continue
            er = np.max(np.abs(r - r_ref[j])) / np.abs(r_ref[j][0])
            eb = np.max(np.abs(b - b_ref[j])) / np.max(np.abs(b_ref[j]))
            worst = [max(worst[0], er), max(worst[1], eb)]
            assert er <= cc.R_TOL, (tag, c, j, "r", er)
            assert eb <= cc.B_TOL, (tag, c, j, "b", eb)
        ymax = np.max(np.abs(y_ref))
        ey = np.max(np.abs(yf[c] - y_ref)) / ymax
        eh = 0.0
        if blocks > 1 and nb > 1:
            head = np.concatenate([np.arange(j * L, j * L + nb - 1) for j in range(1, blocks) if want[j]])
            eh = np.max(np.abs(yf[c][head] - y_ref[head])) / ymax
        print(f"\n[clutter blocks {tag} cpi {c}] r {worst[0]:.2e}  b {worst[1]:.2e}  y {ey:.2e}  block heads {eh:.2e}")
        assert ey <= cc.Y_TOL, (tag, c, "y", ey)
        assert eh <= cc.Y_TOL, (tag, c, "the first nBins - 1 outputs of the blocks", eh)


def heads_need_history(chans, refs, dmin, dmax, blocks):
    """On these inputs a block filtered alone (zero-filled history) misses Y_TOL on its first nBins - 1 outputs."""
    n, nb = chans[0][0].shape[0], dmax - dmin
    L = n // blocks
    for c, (x, y) in enumerate(chans):
        y_ref = refs[c][1]
        for j in range(1, blocks):
            _, alone = O.wiener_hopf(x[j * L:(j + 1) * L], y[j * L:(j + 1) * L], dmin, dmax)
            e = np.max(np.abs(alone[:nb - 1] - y_ref[j * L:j * L + nb - 1])) / np.max(np.abs(y_ref))
            assert e > 100 * cc.Y_TOL, (c, j, e)


@pytest.mark.parametrize("dmin,dmax", [(0, 16), (-3, 13), (2, 18)])
def test_three_segments_per_block(b2, dmin, dmax):
    """N = 8192 in 4 blocks on F = 1024: segments of 1009, 1009 and 30 samples per block, the history of every block start in
    the previous block; delayMin = -3 / 2: the CPI-level wrap in block 0's head and the last block's tail (uint32 path)."""
    n, blocks = 8192, 4
    chans = cc.cpis_for(dmin, dmax, n, 1)
    refs = refs_for(chans, dmin, dmax, blocks, "seg3")
    heads_need_history(chans, refs, dmin, dmax, blocks)
    wh = handle(b2, dmin, dmax, n, blocks, 1, fft_len=1024)
    assert wh.seg_len == 1024 - 16 + 1 and -(-(n // blocks) // wh.seg_len) == 3
    check(run(b2, wh, b2.FMT_C32, chans, blocks), chans, refs, dmin, dmax, blocks, ("seg3", dmin))


@pytest.mark.parametrize("taps", [16, 400])
def test_blocks_shorter_than_the_transform(b2, taps):
    """N = 4096 in 8 blocks of 512 < F; at 400 taps the history spans most of the previous block, and the block is shorter
    than two filter lengths: r and b are summed lag by lag in fp64 (plan_info: 'direct')."""
    n, blocks, dmin, dmax = 4096, 8, 0, taps
    chans = cc.cpis_for(dmin, dmax, n, 1)
    refs = refs_for(chans, dmin, dmax, blocks, "short")
    wh = handle(b2, dmin, dmax, n, blocks, 1)
    assert n // blocks < wh.fft_len
    assert (wh.plan_info()["corr"] == "direct") == (n // blocks < 2 * taps)
    check(run(b2, wh, b2.FMT_C32, chans, blocks), chans, refs, dmin, dmax, blocks, ("short", taps))


def test_direct_correlations(b2):
    """Blocks shorter than two filter lengths (512 samples, 300 taps from lag -3): the fp64 lag sums on two CPIs back to back
    and with cpi_stride = N + 5 (equal bits), from the int16 words (the bits of the fp32 planes) and the int8 planes (the
    bits of the int16 words of the clipped samples); a forced correlation form takes the handle back to the transforms."""
    n, blocks, dmin, dmax, B = 4096, 8, -3, 297, 2
    chans = cc.cpis_for(dmin, dmax, n, B)
    refs = refs_for(chans, dmin, dmax, blocks, "direct")
    wh = handle(b2, dmin, dmax, n, blocks, B)
    assert wh.plan_info()["corr"] == "direct"
    flat = run(b2, wh, b2.FMT_C32, chans, blocks, stride=n)
    gaps = run(b2, wh, b2.FMT_C32, chans, blocks)
    check(flat, chans, refs, dmin, dmax, blocks, "direct, stride N")
    check(gaps, chans, refs, dmin, dmax, blocks, "direct, stride N + 5")
    same_bits(flat, gaps, "direct: the two strides", n)
    same_bits(gaps, run(b2, wh, b2.FMT_I16, chans, blocks), "direct: i16 == c32", n)
    chans8 = cc.cpis_for(dmin, dmax, n, B, i8=True)
    q8 = run(b2, wh, b2.FMT_I8, chans8, blocks)
    check(q8, chans8, refs_for(chans8, dmin, dmax, blocks, "direct8"), dmin, dmax, blocks, "direct, i8")
    same_bits(run(b2, wh, b2.FMT_I16, chans8, blocks), q8, "direct: i8 == i16", n)
    wh.set_corr_form("window")
    assert wh.plan_info()["corr"] == "window"
    check(run(b2, wh, b2.FMT_C32, chans, blocks), chans, refs, dmin, dmax, blocks, "direct geometry, transforms forced")


@pytest.mark.parametrize("n,blocks", [(16384, 2), (8188, 4)])
def test_2047_taps(b2, n, blocks):
    """2047 taps on F = 4096; N = 8188 in 4 blocks: L = 2047 = nBins, the limit.

    With as many taps as the block has samples the block's circular autocorrelation matrix is a full circulant whose
    eigenvalues are the reference's power spectrum: cond(A) = 4.3e4, 2.0e5, 3.7e4 and 9.0e5 in the four blocks of this scene
    (26 at [16384-2]).  On the transforms' fp32 partial correlations (r 1.1e-7, b 1.6e-7: inside their gates) the filtered
    channel was off by 9.6e-3 of max|y_ref| there, a hundred times the gate; blocks shorter than two filter lengths therefore
    sum r and b lag by lag in fp64 (clutter_corr_direct_kernel: r 3.3e-16, b 2.0e-16, y 2.3e-7)."""
    dmin, dmax = 0, 2047
    chans = cc.cpis_for(dmin, dmax, n, 1)
    refs = refs_for(chans, dmin, dmax, blocks, "2047")
    wh = handle(b2, dmin, dmax, n, blocks, 1)
    assert wh.fft_len == 4096 and wh.nBins == 2047
    assert (wh.plan_info()["corr"] == "direct") == (n // blocks < 2 * 2047)
    check(run(b2, wh, b2.FMT_C32, chans, blocks), chans, refs, dmin, dmax, blocks, ("2047", n, blocks))


def test_error_returns(b2):
    E = b2.Blah2HipError
    for args, code in (((0, 16, 8192, 0), b2._lib.ERR_INVALID),          # n_blocks == 0
                       ((0, 16, 8190, 4), b2._lib.ERR_INVALID),          # n_samples % n_blocks != 0
                       ((0, 2047, 8184, 4), b2._lib.ERR_UNSUPPORTED),    # L = 2046 < nBins
                       ((0, 4082, 16384, 2), b2._lib.ERR_UNSUPPORTED)):  # a long filter
        with pytest.raises(E) as e:
            b2.WienerHopf(args[0], args[1], args[2], max_batch=1, blocks=args[3])
        assert e.value.code == code, (args, e.value)
    import torch
    n = 8192
    wh = handle(b2, 0, 16, n, 4, 1)
    x = torch.zeros(n, dtype=torch.complex64, device="cuda")
    y = torch.zeros(n, dtype=torch.complex64, device="cuda")
    with pytest.raises(E) as e:
        wh.process_multi_dev(b2.FMT_C32, x.data_ptr(), [y.data_ptr()], 1, n, [y.data_ptr()], n)
    assert e.value.code == b2._lib.ERR_UNSUPPORTED
    assert set(wh.get_timing()) == set(b2._lib.CLUTTER_KERNEL_NAMES.values())  # the same four slots


def test_batch_and_both_estimation_launch_forms(b2):
    """n_cpi = max_batch = 3: CPIs back to back (one correlation launch over 12 virtual CPIs of stride L) and cpi_stride =
    N + 5 (one launch per CPI into its rows of the partials): the same bits, each within the gates; a second call repeats."""
    n, blocks, dmin, dmax, B = 8192, 4, 0, 16, 3
    chans = cc.cpis_for(dmin, dmax, n, B)
    refs = refs_for(chans, dmin, dmax, blocks, "batch")
    wh = handle(b2, dmin, dmax, n, blocks, B, fft_len=1024)
    flat = run(b2, wh, b2.FMT_C32, chans, blocks, stride=n, reps=2)
    per_cpi = run(b2, wh, b2.FMT_C32, chans, blocks, stride=n + cc.IN_GAP, reps=2)
    check(flat[0], chans, refs, dmin, dmax, blocks, "batch, stride N")
    check(per_cpi[0], chans, refs, dmin, dmax, blocks, "batch, stride N + 5")
    same_bits(flat[0], flat[1], "relaunch, stride N", n)
    same_bits(per_cpi[0], per_cpi[1], "relaunch, stride N + 5", n)
    same_bits(flat[0], per_cpi[0], "the two launch forms", n)


def test_more_systems_than_compute_units(b2):
    """33 CPIs of 8 blocks: 264 Toeplitz systems in one launch, more than one per CU -- where a handle with blocks runs the
    look-ahead solve on its narrowest one-workgroup slices instead of the planner's widest (asserted through solve_info)."""
    n, blocks, dmin, dmax, B = 1024, 8, 0, 8, 33
    chans = cc.cpis_for(dmin, dmax, n, B)
    refs = refs_for(chans, dmin, dmax, blocks, "many")
    wh = handle(b2, dmin, dmax, n, blocks, B)
    got = run(b2, wh, b2.FMT_C32, chans, blocks, stride=n)
    info = wh.solve_info()
    assert info["form"] == b2._lib.CLUTTER_SOLVE_LOOKAHEAD and info["E"] == 2 and info["G"] == 1 and info["fault"] == 0, info
    check(got, chans, refs, dmin, dmax, blocks, "264 systems")


def test_formats(b2):
    """FMT_I16 equals FMT_C32 bit for bit (int16 -> fp32 is exact), FMT_I8 equals FMT_I16 on the clipped samples -- where
    tests/test_clutter_edge_cases_gpu.py asserts them without blocks -- and each is within the gates."""
    n, blocks, dmin, dmax = 8192, 4, -3, 13
    chans = cc.cpis_for(dmin, dmax, n, 2)
    refs = refs_for(chans, dmin, dmax, blocks, "fmt")
    r32 = run(b2, handle(b2, dmin, dmax, n, blocks, 2, fft_len=1024), b2.FMT_C32, chans, blocks)
    r16 = run(b2, handle(b2, dmin, dmax, n, blocks, 2, fft_len=1024), b2.FMT_I16, chans, blocks)
    check(r32, chans, refs, dmin, dmax, blocks, "c32")
    check(r16, chans, refs, dmin, dmax, blocks, "i16")
    same_bits(r32, r16, "i16 == c32", n)
    chans8 = cc.cpis_for(dmin, dmax, n, 2, i8=True)
    refs8 = refs_for(chans8, dmin, dmax, blocks, "fmt8")
    q16 = run(b2, handle(b2, dmin, dmax, n, blocks, 2, fft_len=1024), b2.FMT_I16, chans8, blocks)
    q8 = run(b2, handle(b2, dmin, dmax, n, blocks, 2, fft_len=1024), b2.FMT_I8, chans8, blocks)
    check(q8, chans8, refs8, dmin, dmax, blocks, "i8")
    same_bits(q16, q8, "i8 == i16", n)


def test_failed_block_passes_through(b2):
    """The reference zeroed over block 2: ok = [1, 1, 0, 1], block 2 is y bit for bit, the others are filtered."""
    n, blocks, dmin, dmax = 8192, 4, 0, 16
    L = n // blocks
    x, y = cc.cpis_for(dmin, dmax, n, 1)[0]
    x = x.copy()
    x[2 * L:3 * L] = 0
    chans = [(x, y)]
    refs = refs_for(chans, dmin, dmax, blocks, "failed")
    got = run(b2, handle(b2, dmin, dmax, n, blocks, 1, fft_len=1024), b2.FMT_C32, chans, blocks)
    check(got, chans, refs, dmin, dmax, blocks, "failed block", ok_expect=[1, 1, 0, 1])
    assert got[1].tolist() == [1, 1, 0, 1]
    want = y[2 * L:3 * L].astype(np.complex64).view(np.uint32).reshape(L, 2)
    assert np.array_equal(got[0][0, 2 * L:3 * L], want), "a block that is not positive definite passes y through"
    assert not got[2][2][1].any()  # its taps are zero


def test_one_block_is_the_existing_filter(b2):
    """create_ex(..., n_blocks = 1, ...) against create: equal bits of the filtered channel, the taps, r and b."""
    n, dmin, dmax = 8192, -3, 13
    chans = cc.cpis_for(dmin, dmax, n, 2)
    L_ = b2.load()
    h = C.c_void_p()
    b2._lib.check(L_.blah2hip_clutter_create(dmin, dmax, n, 0, 2, C.byref(h)))
    plain = b2.WienerHopf.__new__(b2.WienerHopf)  # the mirror's constructor goes through create_ex: wrap the handle of create
    plain._h, plain._L, plain.nSamples, plain.max_batch, plain.blocks = h, L_, n, 2, 1
    plain._refresh_dims()
    ex = handle(b2, dmin, dmax, n, 1, 2)
    a, b = run(b2, plain, b2.FMT_C32, chans, 1), run(b2, ex, b2.FMT_C32, chans, 1)
    same_bits(a, b, "create_ex(1) == create", n)
    assert a[1].tolist() == [1, 1]


def test_in_place(b2):
    """d_y_out == d_y (FMT_C32) equals out of place bit for bit."""
    n, blocks, dmin, dmax = 8192, 4, 2, 18
    chans = cc.cpis_for(dmin, dmax, n, 2)
    wh = handle(b2, dmin, dmax, n, blocks, 2, fft_len=1024)
    out = run(b2, wh, b2.FMT_C32, chans, blocks)
    inp = run(b2, wh, b2.FMT_C32, chans, blocks, in_place=True)
    same_bits(out, inp, "in place", n)


def test_estimate_leaves_per_block_taps(b2):
    """blah2hip_clutter_estimate_dev_fmt on a handle with blocks: flags, r, b and taps per virtual CPI, the bits of the
    process call; taps_dev describes one block's filter."""
    import torch
    n, blocks, dmin, dmax, B = 8192, 4, -3, 13, 2
    chans = cc.cpis_for(dmin, dmax, n, B)
    full = run(b2, handle(b2, dmin, dmax, n, blocks, B, fft_len=1024), b2.FMT_C32, chans, blocks)
    est = handle(b2, dmin, dmax, n, blocks, B, fft_len=1024)
    dx, dy = device_inputs(torch, b2, b2.FMT_C32, chans, n + cc.IN_GAP)
    wo, ok = cc.guarded(torch, (B * blocks,), torch.int32)
    est.estimate_dev_fmt(b2.FMT_C32, dx.data_ptr(), dy.data_ptr(), B, n + cc.IN_GAP, ok.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert cc.guard_intact(wo) and np.array_equal(ok.cpu().numpy(), full[1])
    for v in range(B * blocks):
        got = est.read_last(v)
        assert got[0] == full[2][v][0]
        for name, p, q in zip("wrb", got[1:], full[2][v][1:]):
            assert np.array_equal(cc.bits(p), cc.bits(q)), (v, name)
    ptr, nb, dm = est.taps_dev()
    assert ptr and nb == dmax - dmin and dm == dmin


def test_host_entry_point(b2):
    """WienerHopf(blocks=4).process: the AND of the blocks' flags and the filtered channel; a failed block: False, y back."""
    n, blocks, dmin, dmax = 8192, 4, 0, 16
    L = n // blocks
    x, y = cc.cpis_for(dmin, dmax, n, 1)[0]
    wh = handle(b2, dmin, dmax, n, blocks, 1)
    ok, yf = wh.process(x.astype(np.complex64), y.astype(np.complex64))
    y_ref = refs_for([(x, y)], dmin, dmax, blocks, "host")[0][1]
    assert ok and np.max(np.abs(yf - y_ref)) / np.max(np.abs(y_ref)) <= cc.Y_TOL
    x0 = x.copy()
    x0[2 * L:3 * L] = 0
    ok, yf = wh.process(x0, y)  # the fp64 entry point
    assert not ok and np.array_equal(yf, y)
    assert [wh.read_last(v)[0] for v in range(blocks)] == [True, True, False, True]


def test_scene_property(b2):
    """The drifting-clutter scene: the device's residual with 16 blocks is the restatement's to 0.1 dB, and at least 12 dB
    under the device's own result with one tap set per CPI."""
    x, y = R.drifting_scene()
    chans = [(x, y)]
    res = {}
    for blocks in (1, 16):
        wh = handle(b2, R.SCENE_DMIN, R.SCENE_DMAX, R.SCENE_N, blocks, 1)
        words, okv, _ = run(b2, wh, b2.FMT_C32, chans, blocks)
        assert okv.all()
        res[blocks] = R.residual_db(cc.as_c128(words, R.SCENE_N)[0], y)
    _, y_ref, _, _, _ = R.wiener_hopf_blocks(x, y, R.SCENE_DMIN, R.SCENE_DMAX, 16)
    want = R.residual_db(y_ref, y)
    print(f"\n[clutter blocks scene] residual dB: device B=1 {res[1]:.2f}, device B=16 {res[16]:.2f}, restatement B=16 {want:.2f}")
    assert abs(res[16] - want) <= 0.1
    assert res[1] - res[16] >= 12.0
