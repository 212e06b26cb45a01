"""GPU: long clutter filters (more than 4081 taps; csrc/clutter.hip long_process) where their index arithmetic sits on a
boundary: chunk edges, several surveillance channels, a lone CPI with any stride.

The long form splits the lag window into chunks of 2048 taps.  long_plane_kernel<0/1/2> rotate or delay the channels by
c * 2048, long_gather_kernel / long_taps_kernel move r, b and the taps between the children's layout and the filter's,
and blah2hip_clutter_process_multi_dev_fmt runs it channel by channel into the virtual-CPI layout (d_wM, d_rbM).
tests/test_long_filter_model.py states the identities on the CPU; here the device runs them where the guards
(`k >= n`, `k < n`, `(m + off) % N`, `m >= off`) are on their edge: a tap count that is a whole number of chunks, a last
chunk of one tap, as many taps as samples.

1. Chunk edges, one channel: ok, r, b, the filtered channel and the taps against the fp64 oracle, the Toeplitz residual,
   and the FIR against the engine's OWN taps (y - (w * xs)[0..N) in fp64), which pins long_plane_kernel<2> and
   long_taps_kernel at any conditioning.
2. K = 3 channels: the bits of the per-channel call, the oracle, a failed CPI, estimate only, K growing on one handle,
   a refusal that leaves the handle usable.
3. n_cpi = 1 with cpi_stride = out_stride = 0 and nSamples - 1: the bits of the call with stride nSamples, on a long
   handle and on a short one.

The inputs are those of tests/clutter_crafted.py and tests/test_multi_clutter_gpu.py; every oracle result is computed
once (clutter_crafted.oracle_for, and _multi_refs below) and left unchanged."""
import ctypes

import numpy as np
import pytest

import clutter_crafted as cc
import test_multi_clutter_gpu as mc
from oracle import blah2_oracle as O
from test_long_filter_model import xs_of

pytestmark = pytest.mark.gpu

LONG_C = 2048  # csrc/clutter_kernels.hpp


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


# ---- 1. chunk edges, one channel -------------------------------------------------------------------------------------
#         (dmin, dmax, n)            the oracle's Toeplitz matrix: cond
GEOMS = [(0, 4096, 12_288),       # 4096 taps: two whole chunks, N a multiple of 2048                      4e1
         (-3, 4094, 12_301),      # 4097 taps: a third chunk of ONE tap, odd N                              6e1
         (-7, 6137, 18_433),      # 6144 taps: three whole chunks                                           5e1
         (5, 4102, 12_301),       # 4097 taps from a positive first lag: the uint32 index is no rotation    6e1
         (-2, 4098, 8209),        # 4100 taps, N about twice the taps                                       1.5e2
         (0, 4100, 4100)]         # 4100 taps = nSamples, the most that create accepts                      2.4e4
GEOM_IDS = ["4096-two-chunks", "4097-one-tap-chunk", "6144-three-chunks", "4097-positive-lag", "4100-n-2x", "4100-taps-eq-n"]
B1 = 2


def fir_with_own_taps(x, y, w, dmin):
    """y - (w * xs)[0..N) in fp64, w the complex64 taps the engine reports (WienerHopf.cpp:125-160)."""
    n = x.shape[0]
    xs = xs_of(x, dmin)
    L = n + w.shape[0]
    return y - np.fft.ifft(np.fft.fft(xs, n=L) * np.fft.fft(w.astype(np.complex128), n=L))[:n]


@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_chunk_edges_against_the_oracle(b2, geom):
    dmin, dmax, n = geom
    nb = dmax - dmin
    ill = nb == n  # circulant-like, cond 2.4e4: a 1e-6 change of r, b moves the oracle's own taps by 5e-4
    key = (dmin, dmax, n, B1, False)
    chans = cc.cpis_for(dmin, dmax, n, B1)
    wh = b2.WienerHopf(dmin, dmax, n, max_batch=B1)
    assert wh.nBins == nb and wh.plan_info()["chunks"] == -(-nb // LONG_C)
    run = cc.run_filter(b2, wh, b2.FMT_C32, chans)  # input stride n + 5, output stride n + 3, guards asserted
    words, okv, reads = run
    yf = cc.as_c128(words, n)
    if not ill:
        cc.check_oracle(run, chans, key, dmin, dmax, GEOM_IDS[GEOMS.index(geom)])  # ok, r, b, the filtered channel
    for c in range(B1):
        x, y = chans[c]
        ok_ref, y_ref, w_ref, r_ref, b_ref = cc.oracle_for(key, c, x, y, dmin, dmax)
        assert ok_ref and okv[c] == 1 and reads[c][0], (geom, c, okv)
        _, w, r, b = reads[c]
        ew = np.max(np.abs(w - w_ref)) / np.max(np.abs(w_ref))
        res = O.toeplitz_residual(r, w.astype(np.complex128), b)
        # the engine's FIR against the engine's own taps
        efir = np.max(np.abs(yf[c] - fir_with_own_taps(x, y, w, dmin))) / np.max(np.abs(y_ref))
        # the residual the oracle's taps leave in the oracle's r, b once they are rounded to complex64
        res_ref = O.toeplitz_residual(r_ref, w_ref.astype(np.complex64).astype(np.complex128), b_ref)
        print(f"\n[long edge {geom} cpi {c}] w {ew:.2e}  residual {res:.2e} (the oracle's taps as complex64: {res_ref:.2e})  "
              f"FIR against own taps {efir:.2e}")
        assert efir <= cc.Y_TOL, (geom, c, "FIR against own taps", efir)
        if ill:
            # r and b are gated as everywhere; the taps and the filtered channel against the oracle are printed, not
            # gated (the conditioning, see `ill`).  Residual: 4 x that of the oracle's taps rounded to complex64, measured
            # on the CPU 3.0e-8 (CPI 0) and 3.1e-8 (CPI 1), so the bound is 1.2e-7; the engine's taps also carry the
            # recursion's own rounding.  On an MI355X: 2.2e-8 and 3.4e-8.
            er = np.max(np.abs(r - r_ref)) / np.abs(r_ref[0])
            eb = np.max(np.abs(b - b_ref)) / np.max(np.abs(b_ref))
            ey = np.max(np.abs(yf[c] - y_ref)) / np.max(np.abs(y_ref))
            print(f"[long edge {geom} cpi {c}] r {er:.2e}  b {eb:.2e}  y {ey:.2e} (not gated)")
            assert er <= cc.R_TOL, (geom, c, "r", er)
            assert eb <= cc.B_TOL, (geom, c, "b", eb)
            assert res <= 4.0 * res_ref, (geom, c, "residual", res, res_ref)
        else:
            assert ew <= 2e-5, (geom, c, "w", ew)
            assert res <= 1e-5, (geom, c, "residual", res)
    wh.close()


# ---- 2. several channels on a long filter ----------------------------------------------------------------------------
MN, MDMIN, MDMAX, MK = 12_301, -3, 4094, 3  # 4097 taps: three chunks, the last of one tap
MSTRIDE = MN + 5


def multi_scenes(B):
    """checked_scenes(12_301, -3, 4094, K = 3, B, seed = 500): CPI c is scene(seed + c) whatever B is, so one checked set
    of three CPIs serves the two-CPI tests as well (the check itself is three fp64 solves)."""
    return mc.checked_scenes(MN, MDMIN, MDMAX, MK, 3, seed=500)[:B]


_multi_runs = {}


def multi_and_singles(b2, B):
    """(planes, the K = 3 multi call on a fresh handle, the per-channel calls on a second fresh handle), once per B."""
    import torch
    if B not in _multi_runs:
        tx, tys = mc.planes(torch, False, multi_scenes(B), MK, MSTRIDE)
        wh = b2.WienerHopf(MDMIN, MDMAX, MN, max_batch=B)
        assert wh.plan_info()["chunks"] == 3
        multi = mc.run_multi(torch, wh, b2.FMT_C32, tx, tys, B, MSTRIDE, MN)
        wh1 = b2.WienerHopf(MDMIN, MDMAX, MN, max_batch=B)
        singles = [mc.run_single(torch, wh1, b2.FMT_C32, tx, tys[k], B, MSTRIDE) for k in range(MK)]
        wh.close()
        wh1.close()
        _multi_runs[B] = (tx, tys, multi, singles)
    return _multi_runs[B]


_multi_refs = {}


def multi_oracle(k, c):
    if (k, c) not in _multi_refs:
        x, ys = multi_scenes(2)[c]
        _multi_refs[k, c] = O.wiener_hopf(mc.as_c128(x), mc.as_c128(ys[k]), MDMIN, MDMAX, return_filter=True)
    return _multi_refs[k, c]


def words_c128(words, n):
    v = np.ascontiguousarray(words[:n]).view(np.float32)
    return v[..., 0].astype(np.float64) + 1j * v[..., 1].astype(np.float64)


def assert_multi_bits(u, v, tag):
    """Two multi runs (run_multi's tuples): planes with their gaps, ok, and (ok, w, r, b) of every virtual CPI."""
    for k, (p, q) in enumerate(zip(u[0], v[0])):
        assert np.array_equal(p, q), (tag, k, "filtered channel")
    assert np.array_equal(u[1], v[1]), (tag, "ok")
    assert len(u[2]) == len(v[2])
    for i, (a, b) in enumerate(zip(u[2], v[2])):
        assert a[0] == b[0], (tag, i)
        for name, p, q in zip("wrb", a[1:], b[1:]):
            assert np.array_equal(mc.bits(p), mc.bits(q)), (tag, i, name)


def test_multi_bits_of_the_per_channel_call(b2):
    """K = 3, n_cpi = 2 on a long handle: filtered rows with their gaps, ok [K][B], r, b, w per virtual CPI are the bits of
    process_dev_fmt channel by channel on a second long handle (the same code per channel), r shared across channels."""
    B = 2
    tx, tys, multi, singles = multi_and_singles(b2, B)
    assert multi[1].tolist() == [[1] * B] * MK
    for k in range(MK):
        mc.assert_channel_bits(multi, k, B, singles[k], ("long multi", k))
        assert (multi[0][k][:, MN:] == mc.GUARD).all(), k
    # the channels differ: no channel's taps or plane is a copy of another's
    assert not np.array_equal(mc.bits(multi[2][0][1]), mc.bits(multi[2][B][1]))
    assert not np.array_equal(mc.bits(multi[2][B][1]), mc.bits(multi[2][2 * B][1]))
    assert not np.array_equal(multi[0][0], multi[0][1]) and not np.array_equal(multi[0][1], multi[0][2])


def test_multi_every_channel_against_the_oracle(b2):
    B = 2
    tx, tys, multi, singles = multi_and_singles(b2, B)
    got, okv, reads = multi
    for k in range(MK):
        for c in range(B):
            ok_ref, y_ref, w_ref, r_ref, b_ref = multi_oracle(k, c)
            assert ok_ref and okv[k][c] == 1 and reads[k * B + c][0], (k, c)
            _, w, r, b = reads[k * B + c]
            yf = words_c128(got[k][c], MN)
            er = np.max(np.abs(r - r_ref)) / np.abs(r_ref[0])
            eb = np.max(np.abs(b - b_ref)) / np.max(np.abs(b_ref))
            ey = np.max(np.abs(yf - y_ref)) / np.max(np.abs(y_ref))
            print(f"\n[long multi channel {k} cpi {c}] r {er:.2e}  b {eb:.2e}  y {ey:.2e}")
            assert er <= cc.R_TOL, (k, c, "r", er)
            assert eb <= cc.B_TOL, (k, c, "b", eb)
            assert ey <= cc.Y_TOL, (k, c, "y", ey)


def test_multi_failed_cpi(b2):
    """n_cpi = 3, the reference of CPI 1 all zero: ok[:, 1] = 0, the rows of CPI 1 keep the guard pattern in every channel
    (the single call passes y through; the multi entry point leaves them unwritten), its virtual CPIs read ok = 0 and zero
    taps, and CPIs 0 and 2 keep the bits of the same call with the reference in place."""
    import torch
    B = 3
    tx, tys, good, _ = multi_and_singles(b2, B)
    assert good[1].tolist() == [[1] * B] * MK
    cpis = multi_scenes(B)
    bad = [cpis[0], (np.zeros_like(cpis[1][0]), cpis[1][1]), cpis[2]]
    txb, tysb = mc.planes(torch, False, bad, MK, MSTRIDE)
    wh = b2.WienerHopf(MDMIN, MDMAX, MN, max_batch=B)
    got, ok, reads = mc.run_multi(torch, wh, b2.FMT_C32, txb, tysb, B, MSTRIDE, MN)
    assert ok.tolist() == [[1, 0, 1]] * MK
    for k in range(MK):
        assert (got[k][1] == mc.GUARD).all(), k
        bad_ok, bad_w = reads[k * B + 1][:2]
        assert not bad_ok and not bad_w.any(), k
        for c in (0, 2):
            assert np.array_equal(got[k][c], good[0][k][c]), (k, c)
            assert reads[k * B + c][0]
            for name, p, q in zip("wrb", reads[k * B + c][1:], good[2][k * B + c][1:]):
                assert np.array_equal(mc.bits(p), mc.bits(q)), (k, c, name)
    wh.close()


def taps_through_the_pointer(wh, rows):
    """[rows][nBins] complex64 read from the handle's taps_dev() pointer."""
    from blah2_amd import _lib
    p, nb, dm = wh.taps_dev()
    assert (nb, dm) == (wh.nBins, MDMIN) and p
    host = np.empty((rows, nb), dtype=np.complex64)
    L, ctx = _lib.load(), ctypes.c_void_p()
    assert L.blah2hip_ctx_create(0, ctypes.byref(ctx)) == 0
    assert L.blah2hip_ctx_d2h(ctx, host.ctypes.data, p, host.nbytes) == 0 and L.blah2hip_ctx_sync(ctx) == 0
    L.blah2hip_ctx_destroy(ctx)
    return p, host


def test_multi_estimate_only(b2):
    """d_y_out = NULL: the taps of the filtering call, bit for bit, through read_last and through taps_dev (virtual CPIs);
    the channels are left as they were."""
    import torch
    B = 2
    tx, tys, multi, _ = multi_and_singles(b2, B)
    before = [t.clone() for t in (tx, *tys)]
    wo, ok = mc.guarded(torch, (MK, B), torch.int32)
    wh = b2.WienerHopf(MDMIN, MDMAX, MN, max_batch=B)
    wh.process_multi_dev(b2.FMT_C32, tx.data_ptr(), [t.data_ptr() for t in tys], B, MSTRIDE, None, 0, ok.data_ptr(), mc.stream(torch))
    torch.cuda.synchronize()
    assert mc.guard_intact(wo) and ok.cpu().numpy().tolist() == [[1] * B] * MK
    for t, u in zip((tx, *tys), before):
        assert torch.equal(t.view(torch.int32), u.view(torch.int32))
    taps_ref = np.stack([multi[2][v][1] for v in range(MK * B)])
    for v in range(MK * B):
        o, w, r, b = wh.read_last(v)
        assert o
        for name, p, q in zip("wrb", (w, r, b), multi[2][v][1:]):
            assert np.array_equal(mc.bits(p), mc.bits(q)), (v, name)
    assert np.array_equal(mc.bits(taps_through_the_pointer(wh, MK * B)[1]), mc.bits(taps_ref))
    wh.close()


def test_multi_growing_k_then_a_single_call(b2):
    """One long handle: K = 1, then K = 3 (the multi buffers grow), then process_dev_fmt.  Each is the bits of a fresh
    handle; after the last, read_last and taps_dev address the single call's layout again."""
    import torch
    B = 2
    tx, tys, multi3, singles = multi_and_singles(b2, B)
    fresh = b2.WienerHopf(MDMIN, MDMAX, MN, max_batch=B)
    multi1 = mc.run_multi(torch, fresh, b2.FMT_C32, tx, tys[:1], B, MSTRIDE, MN)
    fresh.close()
    wh = b2.WienerHopf(MDMIN, MDMAX, MN, max_batch=B)
    assert_multi_bits(mc.run_multi(torch, wh, b2.FMT_C32, tx, tys[:1], B, MSTRIDE, MN), multi1, "K = 1")
    mc.assert_channel_bits(multi1, 0, B, singles[0], "K = 1 is the single call")
    with pytest.raises(b2.Blah2HipError):
        wh.read_last(1 * B)  # virtual CPIs of the last call: 1 channel x 2 CPIs
    assert_multi_bits(mc.run_multi(torch, wh, b2.FMT_C32, tx, tys, B, MSTRIDE, MN), multi3, "K = 3 behind K = 1")
    assert wh.read_last(MK * B - 1)[0]
    p_multi, _ = taps_through_the_pointer(wh, MK * B)
    out, okv, reads = mc.run_single(torch, wh, b2.FMT_C32, tx, tys[2], B, MSTRIDE)
    assert np.array_equal(out, singles[2][0]) and np.array_equal(okv, singles[2][1])
    for c in range(B):
        assert reads[c][0] == singles[2][2][c][0]
        for name, p, q in zip("wrb", reads[c][1:], singles[2][2][c][1:]):
            assert np.array_equal(mc.bits(p), mc.bits(q)), (c, name)
    with pytest.raises(b2.Blah2HipError):
        wh.read_last(B)  # the single call's layout: max_batch CPIs, not K x B virtual ones
    p_single, taps = taps_through_the_pointer(wh, B)
    assert p_single != p_multi
    assert np.array_equal(mc.bits(taps), mc.bits(np.stack([singles[2][2][c][1] for c in range(B)])))
    wh.close()


def test_multi_refuses_int8_and_stays_usable(b2):
    import torch
    B = 2
    tx, tys, multi, singles = multi_and_singles(b2, B)
    wh = b2.WienerHopf(MDMIN, MDMAX, MN, max_batch=B)
    out = torch.zeros((MK, B, MSTRIDE), dtype=torch.complex64, device="cuda")
    pys, pout = [t.data_ptr() for t in tys], [out[k].data_ptr() for k in range(MK)]
    st = mc.stream(torch)
    calls = (lambda: wh.process_multi_dev(b2.FMT_I8, tx.data_ptr(), pys, B, MSTRIDE, pout, MSTRIDE, None, st),
             lambda: wh.process_multi_dev(b2.FMT_I8, tx.data_ptr(), pys, B, MSTRIDE, None, 0, None, st),
             lambda: wh.process_dev_fmt(b2.FMT_I8, tx.data_ptr(), pys[0], B, MSTRIDE, pout[0], MSTRIDE, None, st),
             lambda: wh.estimate_dev_fmt(b2.FMT_I8, tx.data_ptr(), pys[0], B, MSTRIDE, None, st))
    for call in calls:
        with pytest.raises(b2.Blah2HipError) as e:
            call()
        assert e.value.code == b2._lib.ERR_UNSUPPORTED and "fp32 planes only, not BLAH2HIP_FMT_I8" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert not out.any()
    assert_multi_bits(mc.run_multi(torch, wh, b2.FMT_C32, tx, tys, B, MSTRIDE, MN), multi, "behind the refusals")
    wh.close()


# ---- 3. a lone CPI with any stride -----------------------------------------------------------------------------------
def lone_cpi_call(b2, wh, which, x, ys, stride):
    """One n_cpi = 1 call with cpi_stride = out_stride = ``stride`` on contiguous planes of exactly n samples.  Returns the
    bit patterns of everything the call leaves: output planes, ok, and (ok, w, r, b) per (virtual) CPI."""
    import torch
    n = x.shape[0]
    st = mc.stream(torch)
    tx = torch.from_numpy(x.astype(np.complex64)).cuda()
    tys = [torch.from_numpy(y.astype(np.complex64)).cuda() for y in ys]
    K = len(tys) if which == "multi" else 1
    keep = [mc.guarded(torch, (n,), torch.complex64) for _ in range(K)]
    wo, ok = mc.guarded(torch, (K,), torch.int32)
    if which == "process":
        wh.process_dev_fmt(b2.FMT_C32, tx.data_ptr(), tys[0].data_ptr(), 1, stride, keep[0][1].data_ptr(), stride, ok.data_ptr(), st)
    elif which == "estimate":
        wh.estimate_dev_fmt(b2.FMT_C32, tx.data_ptr(), tys[0].data_ptr(), 1, stride, ok.data_ptr(), st)
    else:
        wh.process_multi_dev(b2.FMT_C32, tx.data_ptr(), [t.data_ptr() for t in tys], 1, stride, [o.data_ptr() for _, o in keep], stride,
                             ok.data_ptr(), st)
    torch.cuda.synchronize()
    assert all(mc.guard_intact(w) for w, _ in keep) and mc.guard_intact(wo)
    outs = [o.cpu().numpy().view(np.uint32) for _, o in keep]
    if which == "estimate":
        assert all((o == mc.GUARD).all() for o in outs)
    return outs, ok.cpu().numpy(), [wh.read_last(v) for v in range(K)]


@pytest.mark.parametrize("which", ["process", "estimate", "multi"])
@pytest.mark.parametrize("dmax", [4094, 407], ids=["long-4097", "short-410"])
def test_lone_cpi_with_any_stride(b2, dmax, which):
    """The entry points check cpi_stride / out_stride only for n_cpi > 1; with one CPI any value is allowed and callers
    pass 0.  The long form's copies into and out of its private planes must not take the value for a pitch."""
    dmin, n = -3, 12_301
    chans = cc.cpis_for(-3, 4094, n, 2)  # the samples of the one-tap-chunk geometry, on both handles
    x, ys = chans[0][0], [chans[0][1], chans[1][1]]
    wh = b2.WienerHopf(dmin, dmax, n)
    assert (wh.plan_info()["chunks"] > 0) == (dmax - dmin > 4081)
    ref = lone_cpi_call(b2, wh, which, x, ys, n)
    assert ref[1].all() and all(r[0] and r[1].any() for r in ref[2])
    if which != "estimate":
        assert all(o.view(np.float32).any() and not (o == mc.GUARD).any() for o in ref[0])
    for stride in (0, n - 1):
        got = lone_cpi_call(b2, wh, which, x, ys, stride)
        for k, (p, q) in enumerate(zip(got[0], ref[0])):
            assert np.array_equal(p, q), (stride, k, "filtered channel")
        assert np.array_equal(got[1], ref[1]), stride
        for v, (a, b) in enumerate(zip(got[2], ref[2])):
            assert a[0] == b[0], (stride, v)
            for name, p, q in zip("wrb", a[1:], b[1:]):
                assert np.array_equal(mc.bits(p), mc.bits(q)), (stride, v, name)
    wh.close()
