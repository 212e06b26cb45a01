"""The digital down-converter on the device against crafted taps and streams (tests/ddc_crafted.py): every plan class of
ddc_plan, every segment seam, the carried history at every length the tail kernel treats differently.

Everything goes through Channelizer.process_dev with the taps read back from the handle; every case asserts that the
handle's tile is the Python plan's.  Bounds (tests/test_ddc_crafted_model.py derives the first and proves that each of the
wrong restatements it lists breaks these checks 1000-fold):

  census A, B, history   an output with one term: |v_dev - p g[t] a| <= 8 2^-24 |g[t]| |a|; one without: == 0
  census C, short rows   the contract of tests/test_ddc_gpu.py: |v_dev - v_oracle| <= (3 T + 8) 2^-24 sum_t |g[t]| |u[m D - t]|
  deliveries             one call, rows, calls and calls of n_in = D: the same bits

Each test prints its worst error as a fraction of its bound.  Measured on an MI355X (the worst case of each test):
census A 0.379 of the single-term bound (D = 3, T = 1024; 0.220 - 0.379 over the 28 cases), census B 0.403 (D = 24, T = 1024,
eight carriers, int16; 0.311 - 0.403 over the seven classes), the history 0.349 (H = 767; 0.268 - 0.349), every term-less
output exactly zero; census C 0.012 of the contract's bound (D = 26, T = 79; 0.000 - 0.002 at T >= 496), the four
deliveries 0.001 and the same bits in all seven classes, rows shorter than the history 0.009 (D = 33, T = 67) and the bits
of the one-row calls.  No gap lost its pattern, no canary reached a result.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ddc_crafted as K

OUT_X, OUT_Y = np.complex64(5 + 5j), np.complex64(6 - 6j)  # what the output buffers hold before a call
IN_BYTES = {"C32": 8, "I16": 8, "I8": 2}                    # per sample of a plane (int16: of the one plane of words)
CLASS_CASES = K.class_cases()


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


def handle(b2, D, h, offsets, calls):
    """A Channelizer that takes these calls, its tile checked against the Python plan."""
    ch = b2.Channelizer(K.FS, D, h, offsets, max(c.n_in for c in calls), max_rows=max(c.rows for c in calls))
    assert ch.tile == K.plan(D, len(h)).tile
    return ch


def run(b2, torch, ch, fmt, calls, out_gap=0, carrier_gap=0):
    """The calls in turn through process_dev, all enqueued before one wait: ([C][all outputs] x, y complex64 in stream
    order).  Rows of the output are n_out + out_gap apart, carriers a further carrier_gap; what no output owns must keep
    its pattern."""
    Cn, D, code = ch.n_carriers, ch.decim, getattr(b2, "FMT_" + fmt)
    raws = [K.encode(fmt, c.buf) for c in calls]
    d_x = dev(torch, np.concatenate([r[0] for r in raws]))
    d_y = dev(torch, np.concatenate([r[1] for r in raws])) if raws[0][1] is not None else None
    lay, total, at_in = [], 0, 0
    for c in calls:
        n_out = c.n_in // D
        out_stride = n_out + out_gap
        carrier_stride = (c.rows - 1) * out_stride + n_out + carrier_gap
        lay.append((at_in, total, n_out, out_stride, carrier_stride))
        total += (Cn - 1) * carrier_stride + (c.rows - 1) * out_stride + n_out + carrier_gap
        at_in += c.rows * c.stride
    ox, oy = dev(torch, np.full(total, OUT_X)), dev(torch, np.full(total, OUT_Y))
    before = ch.next_sample
    for c, (a_in, a_out, n_out, out_stride, carrier_stride) in zip(calls, lay):
        off = a_in * IN_BYTES[fmt]
        ch.process_dev(code, d_x.data_ptr() + off, d_y.data_ptr() + off if d_y is not None else None, c.n_in, c.rows, c.stride,
                       ox.data_ptr() + 8 * a_out, oy.data_ptr() + 8 * a_out, out_stride, carrier_stride)
    torch.cuda.synchronize()
    assert ch.next_sample == before + sum(c.rows * c.n_in for c in calls)
    hx, hy = ox.cpu().numpy().view(np.complex64), oy.cpu().numpy().view(np.complex64)
    owned = np.zeros(total, dtype=bool)
    gx, gy = [[] for _ in range(Cn)], [[] for _ in range(Cn)]
    for c, (_, a_out, n_out, out_stride, carrier_stride) in zip(calls, lay):
        for k in range(Cn):
            for r in range(c.rows):
                sl = slice(a_out + k * carrier_stride + r * out_stride, a_out + k * carrier_stride + r * out_stride + n_out)
                owned[sl] = True
                gx[k].append(hx[sl])
                gy[k].append(hy[sl])
    assert np.all(hx[~owned] == OUT_X) and np.all(hy[~owned] == OUT_Y)
    assert (~owned).sum() > 0 or (out_gap == 0 and carrier_gap == 0)
    return np.stack([np.concatenate(g) for g in gx]), np.stack([np.concatenate(g) for g in gy])


def worst_of(name, got, want, bound):
    """got [2][n] against want under bound, entry by entry (a NaN fails); where the bound is zero the output is == 0."""
    err = np.abs(got.astype(np.complex128) - want)
    bad = ~(err <= bound)
    assert not bad.any(), (name, [(int(k), int(m), complex(got[k, m]), complex(want[k, m]), float(bound[k, m])) for k, m in np.argwhere(bad)[:4]])
    zero = bound == 0
    assert np.all(got[zero] == 0), name
    return float(np.max(err[~zero] / bound[~zero])) if (~zero).any() else 0.0


def check_single(name, ch, cen, gx, gy, first):
    """Sparse streams: every carrier's outputs under the single-term bound, the others exactly zero."""
    worst = 0.0
    for c, f in enumerate(ch.offsets):
        v, bound = K.expect_single(cen, ch.taps(c), f, ch.decim, first)
        worst = max(worst, worst_of((name, c), np.stack([gx[c], gy[c]]), v, bound))
    return worst


def check_contract(b2, name, ch, u, gx, gy, first):
    worst, T = 0.0, ch.n_taps
    for c, f in enumerate(ch.offsets):
        v, _, S = b2.ddc(u, f, K.FS, ch.decim, None, first_sample=first, g=ch.taps(c), detail=True)
        worst = max(worst, worst_of((name, c), np.stack([gx[c], gy[c]]), v, (3 * T + 8) * K.CONTRACT * S))
    return worst


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_census_a_impulses_into_comparable_taps(b2, torch, case):
    """Every tap of every case is the one term of some output, in tiles and rows beyond the first."""
    D, T = case.D, case.T
    cen = K.census_a(D, T, K.plan(D, T).tile)
    calls = K.deliver(cen.u, [(cen.n_in, cen.rows)], gap=5, fill=K.canary(case.fmt))
    ch = handle(b2, D, K.comparable_taps(T), K.OFFSETS[case.C], calls)
    first = 12345 * D
    ch.reset(first)
    gx, gy = run(b2, torch, ch, case.fmt, calls)
    worst = check_single("census A " + K.case_id(case), ch, cen, gx, gy, first)
    print(f"census A {K.case_id(case)} tile {ch.tile}: worst error {worst:.3f} of the single-term bound")
    ch.close()


@pytest.mark.parametrize("case", CLASS_CASES, ids=K.case_id)
def test_census_b_one_tap_dense_input(b2, torch, case):
    """h = e_t0 for the window's ends, t0 around D, and both sides of every seam: each output is one product of a sample that
    lies in the tile, the lead-in, the row in front or the history; the canaries of the input gap reach nothing."""
    D, T = case.D, case.T
    fmt = case.fmt
    cuts, gap = K.dense_cuts(D, K.plan(D, T).tile)
    u = K.noise(np.random.default_rng(40 + D), fmt, sum(n * r for n, r in cuts), small=True)
    calls = K.deliver(u, cuts, gap, K.canary(fmt))
    first, worst = 7 * D, 0.0
    for t0 in K.census_b_taps(D, T):
        ch = handle(b2, D, K.unit_tap(T, t0), K.OFFSETS[case.C], calls)
        ch.reset(first)
        gx, gy = run(b2, torch, ch, fmt, calls)
        for c, f in enumerate(ch.offsets):
            g = ch.taps(c)
            assert np.count_nonzero(g) == 1 and g[t0] != 0
            v, bound = K.expect_one_tap(u, g, t0, f, D, first)
            worst = max(worst, worst_of((K.case_id(case), t0, c), np.stack([gx[c], gy[c]]), v, bound))
        ch.close()
    print(f"census B {K.case_id(case)} t0 in {K.census_b_taps(D, T)}: worst error {worst:.3f} of the single-term bound")


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_census_c_the_dense_sum(b2, torch, case):
    """The comparable taps under full-scale noise, two calls of two rows, gaps in the input (canaries), between the output's
    rows and between its carriers (patterns that stay)."""
    D, T = case.D, case.T
    cuts, gap = K.dense_cuts(D, K.plan(D, T).tile)
    u = K.noise(np.random.default_rng(50 + D + T), case.fmt, sum(n * r for n, r in cuts))
    calls = K.deliver(u, cuts, gap, K.canary(case.fmt))
    ch = handle(b2, D, K.comparable_taps(T), K.OFFSETS[case.C], calls)
    first = 999 * D
    ch.reset(first)
    gx, gy = run(b2, torch, ch, case.fmt, calls, out_gap=7, carrier_gap=11)
    worst = check_contract(b2, "census C " + K.case_id(case), ch, u, gx, gy, first)
    print(f"census C {K.case_id(case)} tile {ch.tile}: worst error {worst:.3f} of the bound")
    ch.close()


@pytest.mark.parametrize("case", CLASS_CASES, ids=K.case_id)
def test_deliveries_give_the_same_bits(b2, torch, case):
    """One call, four rows, four calls, calls of n_in = D (every one shorter than the history where T - 1 > D): the same
    bits in every plan class, the classes whose taps are split over two and four segments among them."""
    D, T = case.D, case.T
    n_out = (2 * K.plan(D, T).tile + 12) // 4 * 4
    N = n_out * D
    u = K.noise(np.random.default_rng(60 + D), case.fmt, N)
    ways = {"one call": [(N, 1)], "rows": [(N // 4, 4)], "calls": [(N // 4, 1)] * 4, "calls of D": [(D, 1)] * n_out}
    ch = handle(b2, D, K.comparable_taps(T), K.OFFSETS[min(case.C, 3)], [K.Call(None, N, 4, N)])
    first, ref = 31 * D, None
    for way, cuts in ways.items():
        ch.reset(first)
        gx, gy = run(b2, torch, ch, case.fmt, K.deliver(u, cuts))
        if ref is None:
            ref = (gx, gy)
            worst = check_contract(b2, "deliveries " + K.case_id(case), ch, u, gx, gy, first)
        assert np.array_equal(bits(gx), bits(ref[0])) and np.array_equal(bits(gy), bits(ref[1])), way
    print(f"deliveries {K.case_id(case)}: four ways bit for bit, worst error {worst:.3f} of the bound")
    ch.close()


AGES = (0, 255, 256, 511, 512, 767, 768, 1022)


@pytest.mark.parametrize("H", [255, 256, 257, 511, 512, 513, 767, 768, 769, 1023])
def test_history_at_length(b2, torch, H):
    """An impulse per channel at age a from call 1's end, then zeros: the second part's outputs are fed by the history alone,
    from every entry block e = tid + 256 k of the tail kernel.  The same with the zeros as calls of n_in = D (the in-place
    shift, until the impulse has left the history) and with both parts as rows shorter than the history in one call each
    (the tail kernel and ddc_load walk back over several rows, NaN in the gaps)."""
    D, T = 4, H + 1
    offsets, h, first, worst = K.OFFSETS[2], K.comparable_taps(T), 5 * D, 0.0
    ch = None
    for a in [a for a in AGES if a < H]:
        cen, n1, n2 = K.history_stream(D, T, a)
        unit = K.UNIT * D
        ways = {"calls": (K.deliver(cen.u, [(n1, 1), (n2, 1)]), True),
                "rows": (K.deliver(cen.u, [(unit, n1 // unit), (unit, n2 // unit)], 5, K.canary("C32")), True),
                "calls of D": (K.deliver(cen.u, [(n1, 1)] + [(D, 1)] * (n2 // D)), a == 0)}
        assert unit < H and n1 >= H and np.any(cen.tap[:, n1 // D:] >= 0) and np.all(cen.u[:, n1:] == 0)
        if ch is None:
            ch = b2.Channelizer(K.FS, D, h, offsets, n1, max_rows=n1 // unit)
            assert ch.tile == K.plan(D, T).tile
        for way, (calls, wanted) in ways.items():
            if not wanted:
                continue
            ch.reset(first)
            gx, gy = run(b2, torch, ch, "C32", calls)
            worst = max(worst, check_single(("history", H, a, way), ch, cen, gx, gy, first))
    print(f"history H = {H}: worst error {worst:.3f} of the single-term bound")
    ch.close()


@pytest.mark.parametrize("D, T, k, C, fmt", [(24, 1024, 11, 8, "I16"), (33, 67, 1, 2, "C32"), (64, 193, 2, 3, "I8"), (32, 1024, 5, 1, "C32")])
def test_rows_shorter_than_the_history_on_segmented_classes(b2, torch, D, T, k, C, fmt):
    """Rows of k D < T - 1 samples in one call, then again in a second call (its first rows read the history the first
    call's rows left): against the restatement, and bit for bit the stream delivered as one row per call."""
    p = K.plan(D, T)
    n_in = k * D
    rows = -(-(2 * p.tile + 9) // k)
    assert p.G > 1 and n_in < T - 1 and rows * n_in > 2 * (T - 1)
    u = K.noise(np.random.default_rng(70 + D), fmt, 2 * rows * n_in)
    ch = handle(b2, D, K.comparable_taps(T), K.OFFSETS[C], [K.Call(None, rows * n_in, rows, 0)])
    first = 3 * D
    ch.reset(first)
    ax, ay = run(b2, torch, ch, fmt, K.deliver(u, [(rows * n_in, 1)] * 2))
    worst = check_contract(b2, ("short rows", D, T), ch, u, ax, ay, first)
    ch.reset(first)
    bx, by = run(b2, torch, ch, fmt, K.deliver(u, [(n_in, rows)] * 2, 3, K.canary(fmt)), out_gap=2, carrier_gap=5)
    assert np.array_equal(bits(ax), bits(bx)) and np.array_equal(bits(ay), bits(by))
    print(f"short rows D{D} T{T} {rows} rows of {n_in}: worst error {worst:.3f} of the bound, rows and one row bit for bit")
    ch.close()
