"""The digital down-converter on the device (blah2hip_ddc_*) against the fp64 restatement blah2_amd.process.ddc.

Contract, per output, with the oracle's taps read back from the handle and its own sum S = sum_t |g[t]| |u[m D - t]|:
|v_dev - v_oracle| <= (3 T + 8) 2^-24 S.  Every comparison below is made under it; each test prints its worst error as
a fraction of the bound.  Streams delivered in one call, in rows, in calls and in calls shorter than the history must
agree bit for bit.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ddc_scenes as S

FS = 65536.0
IRR = FS / (2.0 * math.pi)        # no rational fraction of fs
IRR2 = -FS * (math.sqrt(2.0) - 1.0) / 3.0
WORST = {}


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    if blah2_amd.device_count() == 0:
        pytest.fail("no GPU visible: the HIP path has no fallback")
    return blah2_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def make_input(b2, rng, fmt, n, small=False):
    """(raw x, raw y or None, u complex128 [2][n]) of n samples in the format; the integer formats at full scale."""
    if fmt == b2.FMT_C32:
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
        y = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
        return x, y, np.stack([x, y]).astype(np.complex128)
    if fmt == b2.FMT_I16:
        lim = 100 if small else 32767
        w = rng.integers(-lim - 1, lim + 1, size=(n, 4), dtype=np.int64).astype(np.int16)
        if not small:
            w[:: 7] = 32767
            w[3:: 11] = -32768
        u = np.stack([w[:, 0] + 1j * w[:, 1], w[:, 2] + 1j * w[:, 3]]).astype(np.complex128)
        return w, None, u
    x = rng.integers(-128, 128, size=(n, 2), dtype=np.int64).astype(np.int8)
    y = rng.integers(-128, 128, size=(n, 2), dtype=np.int64).astype(np.int8)
    x[:: 5] = 127
    y[2:: 9] = -128
    return x, y, np.stack([x[:, 0] + 1j * x[:, 1], y[:, 0] + 1j * y[:, 1]]).astype(np.complex128)


def check_contract(b2, name, ch, h, u, first, got_x, got_y, history=None):
    """got_* [C][n_out] complex64 against the restatement with the read-back taps."""
    T = ch.n_taps
    worst = WORST.get(name, 0.0)
    for c, f in enumerate(ch.offsets):
        g = ch.taps(c)
        v, _, Sv = b2.ddc(u, f, ch.fs, ch.decim, None, first_sample=first, history=history, g=g, detail=True)
        bound = (3 * T + 8) * 2.0 ** -24 * Sv
        for k, got in enumerate((got_x, got_y)):
            err = np.abs(got[c].astype(np.complex128) - v[k])
            assert np.all(err <= bound[k]), (name, c, k, float(np.max(err / np.maximum(bound[k], 1e-300))))
            nz = bound[k] > 0
            if nz.any():
                worst = max(worst, float(np.max(err[nz] / bound[k][nz])))
    WORST[name] = worst
    print(f"{name}: worst error {worst:.3f} of the bound")
    return worst


def one_call(b2, torch, ch, fmt, raw_x, raw_y, n_in, n_rows=1, in_stride=None, out_stride=None, carrier_stride=None):
    """One process_dev over contiguous (or strided) rows; returns ([C][rows * n_out] x, y) complex64 and the raw output buffers."""
    Cn, D = ch.n_carriers, ch.decim
    n_out = n_in // D
    in_stride = n_in if in_stride is None else in_stride
    out_stride = n_out if out_stride is None else out_stride
    carrier_stride = (n_rows - 1) * out_stride + n_out if carrier_stride is None else carrier_stride
    total = (Cn - 1) * carrier_stride + (n_rows - 1) * out_stride + n_out
    d_x = dev(torch, raw_x)
    d_y = dev(torch, raw_y) if raw_y is not None else None
    ox = dev(torch, np.full(total, 5 + 5j, dtype=np.complex64))
    oy = dev(torch, np.full(total, 6 - 6j, dtype=np.complex64))
    ch.process_dev(fmt, d_x.data_ptr(), d_y.data_ptr() if d_y is not None else None, n_in, n_rows, in_stride, ox.data_ptr(), oy.data_ptr(),
                   out_stride, carrier_stride)
    torch.cuda.synchronize()
    hx, hy = host(ox, np.complex64), host(oy, np.complex64)

    def gather(hb):
        return np.stack([np.concatenate([hb[c * carrier_stride + r * out_stride: c * carrier_stride + r * out_stride + n_out]
                                         for r in range(n_rows)]) for c in range(Cn)])
    return gather(hx), gather(hy), hx, hy


def n_out_of(spec, tile):
    return {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "3tile+5": 3 * tile + 5}.get(spec, spec)


def taps_of(spec, D):
    return {"D-1": D - 1, "D": D, "D+1": D + 1, "8D": 8 * D}.get(spec, spec)


C8 = (0.0, FS / 2, -FS / 2, FS / 3, IRR, IRR2, 1000.0, -FS / 3)
# (D, T, n_out, offsets, format): every value of the issue's sets at least once, every (outputs per thread, carrier block)
# instantiation of the kernel (R in 1, 2, 4 by (D, T); block 1, 2, 4 by the carrier count), several workgroups, and the
# tiles below 64 outputs whose taps are split over four segments of the workgroup (D = 64: 59 at T = 512, 51 at T = 1024)
SHAPES = [
    (1, 1024, "3tile+5", (IRR,), "C32"),
    (2, 1, 1, (0.0, FS / 2), "I16"),
    (3, 2, 2, (-FS / 2, FS / 3, IRR), "I8"),
    (4, "D-1", 63, C8, "C32"),
    (7, "D", 64, (IRR2,), "I16"),
    (16, "D+1", 65, (FS / 3, IRR), "I8"),
    (64, "8D", "tile-1", (0.0, IRR, -FS / 2), "C32"),
    (4, 1024, "tile", (IRR, FS / 2), "I16"),
    (64, 1024, "tile+1", C8, "I8"),
    (2, "8D", "3tile+5", (FS / 3, IRR, 0.0), "I16"),
    (1, 1024, "tile+1", (FS / 3, IRR, 0.0), "I8"),
    (2, 1024, 65, (IRR, -FS / 2), "C32"),
    (4, 1024, 2, (IRR,), "I8"),
    (4, 1024, "tile-1", C8, "C32"),
]


@pytest.mark.parametrize("D, T, n_out, offsets, fmt", SHAPES, ids=[f"D{s[0]}-T{s[1]}-n{s[2]}-C{len(s[3])}-{s[4]}" for s in SHAPES])
def test_shapes(b2, torch, D, T, n_out, offsets, fmt):
    fmt = getattr(b2, "FMT_" + fmt)
    T = max(1, taps_of(T, D))
    h = b2.ddc_design(D, T)
    rng = np.random.default_rng(100 + D + T)
    probe = b2.Channelizer(FS, D, h, offsets, D)
    n_out = n_out_of(n_out, probe.tile)
    probe.close()
    n_in = n_out * D
    ch = b2.Channelizer(FS, D, h, offsets, n_in)
    first = 12345 * D
    ch.reset(first)
    rx, ry, u = make_input(b2, rng, fmt, n_in)
    gx, gy, _, _ = one_call(b2, torch, ch, fmt, rx, ry, n_in)
    check_contract(b2, f"shape D={D} T={T} n_out={n_out} C={len(offsets)} fmt={fmt} tile={ch.tile}", ch, h, u, first, gx, gy)
    assert ch.next_sample == first + n_in
    ch.close()


def test_read_back_taps(b2):
    for D, T, offsets in [(4, 64, (IRR, FS / 2, -FS / 2, 0.0, FS / 3)), (7, 1024, (IRR2,)), (1, 1, (FS / 3, 1.0))]:
        h = b2.ddc_design(D, T)
        ch = b2.Channelizer(FS, D, h, offsets, D)
        for c, f in enumerate(offsets):
            g, want = ch.taps(c), b2.ddc_taps(h, f, FS).astype(np.complex64)
            for a, b in ((g.real, want.real), (g.imag, want.imag)):
                assert np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b)).astype(np.float64))
        ch.close()


@pytest.mark.parametrize("fmt", ["C32", "I16", "I8"])
def test_stream_splits_are_bit_identical(b2, torch, fmt):
    fmt = getattr(b2, "FMT_" + fmt)
    D, N = 4, 20000
    T = 4 * D + 1
    h = b2.ddc_design(D, T)
    offsets = (IRR, -FS / 3)
    rng = np.random.default_rng(5)
    rx, ry, u = make_input(b2, rng, fmt, N)
    ch = b2.Channelizer(FS, D, h, offsets, N, max_rows=5)
    first = 77 * D
    # one row
    ch.reset(first)
    ax, ay, _, _ = one_call(b2, torch, ch, fmt, rx, ry, N)
    check_contract(b2, f"stream fmt={fmt}", ch, h, u, first, ax, ay)
    # five rows
    ch.reset(first)
    bx, by, _, _ = one_call(b2, torch, ch, fmt, rx, ry, N // 5, n_rows=5)
    assert np.array_equal(ax.view(np.uint64), bx.view(np.uint64)) and np.array_equal(ay.view(np.uint64), by.view(np.uint64))
    assert ch.next_sample == first + N

    # calls: the outputs of call k land behind those of call k - 1
    def in_calls(n_in):
        ch.reset(first)
        Cn, n_out_all = len(offsets), N // D
        d_x = dev(torch, rx)
        d_y = dev(torch, ry) if ry is not None else None
        ox = dev(torch, np.zeros(Cn * n_out_all, dtype=np.complex64))
        oy = dev(torch, np.zeros(Cn * n_out_all, dtype=np.complex64))
        sb = rx.dtype.itemsize * (rx.shape[1] if rx.ndim == 2 else 1)  # bytes per sample of the raw planes
        for k in range(N // n_in):
            ch.process_dev(fmt, d_x.data_ptr() + k * n_in * sb, d_y.data_ptr() + k * n_in * sb if d_y is not None else None, n_in, 1, n_in,
                           ox.data_ptr() + 8 * k * (n_in // D), oy.data_ptr() + 8 * k * (n_in // D), n_in // D, n_out_all)
        torch.cuda.synchronize()
        assert ch.next_sample == first + N
        return host(ox, np.complex64).reshape(Cn, n_out_all), host(oy, np.complex64).reshape(Cn, n_out_all)

    for n_in in (N // 5, D):  # n_in = D: every call shorter than the history of 4 D samples, which shifts
        cx, cy = in_calls(n_in)
        assert np.array_equal(ax.view(np.uint64), cx.view(np.uint64)), n_in
        assert np.array_equal(ay.view(np.uint64), cy.view(np.uint64)), n_in
    # twice the same: the same bits
    ch.reset(first)
    dx, dy, _, _ = one_call(b2, torch, ch, fmt, rx, ry, N)
    assert np.array_equal(ax.view(np.uint64), dx.view(np.uint64)) and np.array_equal(ay.view(np.uint64), dy.view(np.uint64))
    ch.close()


@pytest.mark.parametrize("fmt", ["C32", "I16"])
def test_stride_gaps(b2, torch, fmt):
    """Canaries in the input gap never reach a result (NaN for fp32; full scale beside samples of at most 100 for int16:
    either would break the bound), those of the output and carrier gaps survive."""
    fmt = getattr(b2, "FMT_" + fmt)
    D, T, rows = 3, 40, 3
    n_in, gap = 50 * D, 13
    n_out = n_in // D
    h = b2.ddc_design(D, T)
    offsets = (IRR, FS / 3, 0.0)
    rng = np.random.default_rng(6)
    rx, ry, u = make_input(b2, rng, fmt, rows * n_in, small=True)
    if fmt == b2.FMT_C32:
        sx = np.full((rows, n_in + gap), np.nan + 1j * np.nan, dtype=np.complex64)
        sy = sx.copy()
        sx[:, :n_in], sy[:, :n_in] = rx.reshape(rows, n_in), ry.reshape(rows, n_in)
    else:
        sx = np.full((rows, n_in + gap, 4), 32767, dtype=np.int16)
        sx[:, :n_in] = rx.reshape(rows, n_in, 4)
        sy = None
    ch = b2.Channelizer(FS, D, h, offsets, n_in, max_rows=rows)
    out_stride, carrier_stride = n_out + 7, 3 * (n_out + 7) + 11
    gx, gy, hx, hy = one_call(b2, torch, ch, fmt, sx, sy, n_in, n_rows=rows, in_stride=n_in + gap, out_stride=out_stride,
                              carrier_stride=carrier_stride)
    check_contract(b2, f"gaps fmt={fmt}", ch, h, u, 0, gx, gy)
    written = np.zeros(hx.shape[0], dtype=bool)
    for c in range(len(offsets)):
        for r in range(rows):
            written[c * carrier_stride + r * out_stride: c * carrier_stride + r * out_stride + n_out] = True
    assert np.all(hx[~written] == np.complex64(5 + 5j)) and np.all(hy[~written] == np.complex64(6 - 6j))
    assert (~written).sum() > 0
    ch.close()


def test_reset_in_mid_stream(b2, torch):
    D, T, n_in = 4, 33, 400
    h = b2.ddc_design(D, T)
    ch = b2.Channelizer(FS, D, h, (IRR,), n_in)
    rng = np.random.default_rng(8)
    rx, ry, u = make_input(b2, rng, b2.FMT_C32, n_in)
    one_call(b2, torch, ch, b2.FMT_C32, rx, ry, n_in)
    assert ch.next_sample == n_in
    # carried: the second call's outputs see the first call's samples
    gx, gy, _, _ = one_call(b2, torch, ch, b2.FMT_C32, rx, ry, n_in)
    check_contract(b2, "carried history", ch, h, u, n_in, gx, gy, history=u[:, n_in - (T - 1):])
    first = 9000 * D
    ch.reset(first)
    assert ch.next_sample == first
    zx, zy, _, _ = one_call(b2, torch, ch, b2.FMT_C32, rx, ry, n_in)
    check_contract(b2, "after reset", ch, h, u, first, zx, zy)
    assert not np.array_equal(zx[:, :T // D], gx[:, :T // D])
    with pytest.raises(b2.Blah2HipError) as e:
        ch.reset(first + 1)
    assert e.value.code == -1 and ch.next_sample == first + n_in
    ch.close()


def test_phase_at_large_indices(b2, torch):
    """first_sample = 2^40 D: a phase from an fp32 product, or from r m without its residual, is wrong by whole turns."""
    D, T, n_in = 4, 32, 4096
    h = b2.ddc_design(D, T)
    ch = b2.Channelizer(FS, D, h, (IRR, IRR2), n_in)
    first = (2 ** 40) * D
    ch.reset(first)
    rng = np.random.default_rng(9)
    rx, ry, u = make_input(b2, rng, b2.FMT_C32, n_in)
    gx, gy, _, _ = one_call(b2, torch, ch, b2.FMT_C32, rx, ry, n_in)
    check_contract(b2, "large indices", ch, h, u, first, gx, gy)
    assert ch.next_sample == first + n_in
    ch.close()


def test_refusals_enqueue_nothing(b2, torch):
    D, T, n_in, rows = 4, 16, 64, 2
    n_out = n_in // D
    h = b2.ddc_design(D, T)
    ch = b2.Channelizer(FS, D, h, (IRR, 0.0), n_in, max_rows=rows)
    ch.reset(40)
    x = dev(torch, np.ones(rows * n_in + 8, dtype=np.complex64))
    y = dev(torch, np.ones(rows * n_in + 8, dtype=np.complex64))
    cs = rows * n_out
    ox = dev(torch, np.full(2 * cs + 8, 5 + 5j, dtype=np.complex64))
    oy = dev(torch, np.full(2 * cs + 8, 6 - 6j, dtype=np.complex64))
    X, Y, OX, OY = x.data_ptr(), y.data_ptr(), ox.data_ptr(), oy.data_ptr()
    good = dict(fmt=b2.FMT_C32, x=X, y=Y, n_in=n_in, rows=rows, in_stride=n_in, ox=OX, oy=OY, out_stride=n_out, cs=cs)
    bad = [(dict(x=None), -1), (dict(y=None), -1), (dict(ox=None), -1), (dict(oy=None), -1), (dict(n_in=0), -1),
           (dict(n_in=n_in + D), -1), (dict(n_in=n_in - 1), -1), (dict(rows=0), -1), (dict(rows=rows + 1), -1),
           (dict(in_stride=n_in - 1), -1), (dict(out_stride=n_out - 1), -1), (dict(cs=cs - 1), -1),
           (dict(ox=X), -1), (dict(oy=Y + 8 * (n_in - 1)), -1), (dict(oy=OX + 8 * (2 * cs - 1)), -1), (dict(oy=OX), -1),
           (dict(x=X + 4), -1), (dict(ox=OX + 4), -1),
           (dict(fmt=b2.FMT_F16), -3), (dict(fmt=b2.FMT_I16X_C32Y), -3), (dict(fmt=b2.FMT_I8X_C32Y), -3), (dict(fmt=99), -3)]
    for kw, code in bad:
        a = dict(good, **kw)
        with pytest.raises(b2.Blah2HipError) as e:
            ch.process_dev(a["fmt"], a["x"], a["y"], a["n_in"], a["rows"], a["in_stride"], a["ox"], a["oy"], a["out_stride"], a["cs"])
        assert e.value.code == code, (kw, e.value)
        assert ch.next_sample == 40, kw
    torch.cuda.synchronize()
    assert np.all(host(ox, np.complex64) == np.complex64(5 + 5j)) and np.all(host(oy, np.complex64) == np.complex64(6 - 6j))
    # the good call still runs, from the position the refusals left alone
    a = good
    ch.process_dev(a["fmt"], a["x"], a["y"], a["n_in"], a["rows"], a["in_stride"], a["ox"], a["oy"], a["out_stride"], a["cs"])
    torch.cuda.synchronize()
    assert ch.next_sample == 40 + rows * n_in
    got = host(ox, np.complex64)
    assert np.all(got[:2 * cs] != np.complex64(5 + 5j)) and np.all(got[2 * cs:] == np.complex64(5 + 5j))
    for kw in [dict(decim=0), dict(decim=65), dict(offsets=(FS,)), dict(offsets=()), dict(offsets=(0.0,) * 9), dict(max_in=n_in + 1),
               dict(max_rows=0), dict(h=np.zeros(1025)), dict(h=np.array([1.0, np.nan]))]:
        a = dict(dict(fs=FS, decim=D, h=h, offsets=(0.0,), max_in=n_in, max_rows=1), **kw)
        with pytest.raises(b2.Blah2HipError) as e:
            b2.Channelizer(a["fs"], a["decim"], a["h"], a["offsets"], a["max_in"], a["max_rows"])
        assert e.value.code == -1, kw
    ch.close()


def test_timing_through_the_handle(b2, torch):
    D, T, n_in = 4, 16, 4096
    ch = b2.Channelizer(FS, D, b2.ddc_design(D, T), (IRR,), n_in)
    ch.set_timing(True)
    rx, ry, _ = make_input(b2, np.random.default_rng(1), b2.FMT_C32, n_in)
    one_call(b2, torch, ch, b2.FMT_C32, rx, ry, n_in)
    one_call(b2, torch, ch, b2.FMT_C32, rx, ry, n_in)
    t = ch.get_timing()
    assert set(t) == {"ddc", "ddc_tail"} and t["ddc"][1] == 2 and t["ddc_tail"][1] == 2 and t["ddc"][0] > 0.0
    assert ch.get_timing()["ddc"][1] == 0
    ch.close()


def test_capturable_in_a_graph(b2, torch):
    """The call only enqueues: captured once, replayed, the replays go on with the stream (history and position live on
    the device)."""
    D, T, n_in = 4, 24, 512
    h = b2.ddc_design(D, T)
    ch = b2.Channelizer(FS, D, h, (IRR,), n_in)
    rng = np.random.default_rng(12)
    pieces = [make_input(b2, rng, b2.FMT_C32, n_in) for _ in range(3)]
    u = np.concatenate([p[2] for p in pieces], axis=-1)
    d_x = torch.zeros(n_in, dtype=torch.complex64, device="cuda")
    d_y = torch.zeros(n_in, dtype=torch.complex64, device="cuda")
    ox = torch.zeros(n_in // D, dtype=torch.complex64, device="cuda")
    oy = torch.zeros(n_in // D, dtype=torch.complex64, device="cuda")
    st = torch.cuda.Stream()
    ch.reset(0, st.cuda_stream)
    st.synchronize()
    st.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):  # one stream, two kernel nodes in a chain: no parallel branches
        ch.process_dev(b2.FMT_C32, d_x.data_ptr(), d_y.data_ptr(), n_in, 1, n_in, ox.data_ptr(), oy.data_ptr(), n_in // D, n_in // D,
                       torch.cuda.current_stream().cuda_stream)
    gx, gy = [], []
    for rx, ry, _ in pieces:
        d_x.copy_(torch.from_numpy(rx))
        d_y.copy_(torch.from_numpy(ry))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        gx.append(ox.cpu().numpy())
        gy.append(oy.cpu().numpy())
    check_contract(b2, "graph replays", ch, h, u, 0, np.concatenate(gx)[None], np.concatenate(gy)[None])
    ch.close()


def test_chain_on_the_scene(b2, torch):
    """Both carriers of the scene in one call of two rows, then the ambiguity stage on each carrier's planes as they stand
    (FMT_C32): the maps within the cell-wise gate of the oracle's map of the restatement's planes, the peaks in place."""
    from gates import map_cell_gate
    x, y = S.scene()
    x32, y32 = x.astype(np.complex64), y.astype(np.complex64)
    h = S.taps()
    ch = b2.Channelizer(S.FS, S.D, h, S.CARRIERS, S.PIECE, max_rows=S.PIECES)
    n_out = S.N // S.D
    gx, gy, hx, hy = one_call(b2, torch, ch, b2.FMT_C32, x32, y32, S.PIECE, n_rows=S.PIECES)
    u = np.stack([x32, y32]).astype(np.complex128)
    check_contract(b2, "scene", ch, h, u, 0, gx, gy)
    d_px, d_py = dev(torch, hx), dev(torch, hy)
    amb = b2.Ambiguity(*S.AMB_ARGS)
    dims = amb.dims
    d_map = torch.zeros(dims.n_doppler_bins * dims.n_delay_bins, dtype=torch.complex64, device="cuda")
    d_met = torch.zeros(2, dtype=torch.float64, device="cuda")
    for c, (f, want) in enumerate(zip(S.CARRIERS, S.PEAKS)):
        amb.process_dev(b2.FMT_C32, d_px.data_ptr() + 8 * c * n_out, d_py.data_ptr() + 8 * c * n_out, 1, n_out, d_map.data_ptr(), d_met.data_ptr())
        torch.cuda.synchronize()
        got = d_map.cpu().numpy().reshape(dims.n_doppler_bins, dims.n_delay_bins)
        odims, ref = S.oracle_map(S.model_planes(u[0], u[1], f, g=ch.taps(c)))
        cell = map_cell_gate(got, ref)
        print(f"carrier {f}: {cell}")
        assert cell["ok"], cell
        (delay, dop), over = S.peak_off_zero(got, odims)
        assert delay == want[0] and abs(dop - want[1]) < 0.5 and over >= 20.0, (delay, dop, over)
    ch.close()
