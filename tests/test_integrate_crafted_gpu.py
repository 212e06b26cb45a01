"""GPU: nci_kernel<W> (blah2hip_nci_process_dev, MapIntegrator) on the crafted maps of tests/integrate_crafted.py, whose
cells all differ: every window W = 1 .. 16 (all five ring lengths), every schedule of calls, hops of a window and more,
several channels with weights, maps 8 bytes off a 16-byte boundary, the fused metrics on a moving peak, maps below 0 dB and
a window that sums to zero.  tests/test_integrate_crafted_model.py shows on the CPU what these cases reach and that the gates
used here would catch a wrong walk or a wrong epilogue.

No reference counterpart; the checks are
  * cells: ``|out - ref| <= (K W + 8) 2^-24 ref`` against the fp64 ``blah2_amd.integrate_maps`` of the whole stream (derived
    in tests/test_integrate_gpu.py), imaginary parts exactly 0;
  * cuts: however the stream is cut into calls, maps and metrics are the same bits;
  * metrics: 1e-3 dB (the project's gate) against fp64 Map::set_metrics of the device's own cells;
  * exact values where the arithmetic gives them: ``maxPower == -noisePower`` below 0 dB, +0 / -inf / +inf for a zero window.
Every output lies in an arena with guard words in front and behind; so does every input.

Measured on the MI355X (printed by the tests; integrate_crafted.FIGURES).  Largest error / bound per window, odd geometry,
K = 1, H = 1, one call: W = 1 .. 16: 0.179 0.187 0.198 0.178 0.186 0.168 0.159 0.134 0.142 0.165 0.143 0.136 0.128 0.134 0.134
0.120; even geometry, W = 5, 9, 13, 16: 0.174 0.169 0.126 0.120; with hops and channels 0.015 (W = 16, K = 8) .. 0.128 (W = 5,
K = 2).  Every other cut into calls, and every placement 8 bytes off, gave the bits of the one aligned call.  Metrics on the
moving peak, largest distance from fp64 set_metrics of the device's own cells (noisePower, maxPower), dB: W = 1: 1.89e-7,
4.28e-6; W = 4: 1.78e-7, 4.52e-6; W = 9: 1.64e-7, 4.59e-6.  No defect was found.
"""
import numpy as np
import pytest

import integrate_crafted as IC

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces
PAD = 64                       # guard words on either side; a multiple of four, so that the data keep the base's alignment
MAX_BATCH = 64
ODD = (-10, 100, -100, 100, 1_000_000, 100_000)    # 21 x 111: every other plane starts 8 bytes off, the last unit is one cell
EVEN = (-10, 101, -100, 100, 1_000_000, 100_000)   # 21 x 112: every plane shares the base's alignment
GEOMS = {"odd": ODD, "even": EVEN}


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


def handle(b2, name):
    if name not in _handles:
        _handles[name] = b2.Ambiguity(*GEOMS[name], True, max_batch=MAX_BATCH)
    return _handles[name]


def shape_of(amb):
    return amb.get_n_doppler_bins(), amb.get_n_delay_bins()


class Arena:
    """``words`` 32-bit words between two runs of guard words, the first of them on a 16-byte boundary or 8 bytes off it."""

    def __init__(self, torch, words, off8=False):
        self.front = PAD + (2 if off8 else 0)
        self.words = words
        self.whole = torch.full((self.front + words + PAD,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
        self.ptr = self.whole.data_ptr() + 4 * self.front
        assert self.whole.data_ptr() % 16 == 0 and self.ptr % 16 == (8 if off8 else 0)

    def fill(self, torch, host):
        raw = np.ascontiguousarray(host).view(np.int32).reshape(-1)
        assert raw.size == self.words
        self.whole[self.front:self.front + self.words].copy_(torch.from_numpy(raw))

    def read(self, used_words):
        """The first ``used_words`` of the data (uint32) after checking that nothing else was written: the guards in front
        and behind, and the data behind the used part."""
        host = self.whole.cpu().numpy().view(np.uint32)
        assert (host[:self.front] == GUARD).all(), "the guard in front was written"
        assert (host[self.front + self.words:] == GUARD).all(), "the guard behind was written"
        assert (host[self.front + used_words:self.front + self.words] == GUARD).all(), "written behind the output"
        return host[self.front:self.front + used_words].copy()


def call(torch, amb, integ, maps, w=None, in_off8=False, out_off8=False):
    """The next maps.shape[1] CPIs of ``integ``; outputs with room for one map per CPI -> (out complex64 [n_out, nD, nC],
    metrics [n_out, 2], first_end)."""
    nD, nC = shape_of(amb)
    cells = nD * nC
    n_cpi = maps.shape[1]
    src = Arena(torch, maps.size * 2, in_off8)
    src.fill(torch, maps)
    dst = Arena(torch, n_cpi * cells * 2, out_off8)
    met = Arena(torch, n_cpi * 4)
    want = integ.count(n_cpi)
    got = integ.process_dev(src.ptr, n_cpi, dst.ptr, met.ptr, n_cpi, w, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert got == want  # count() announces what the call reports
    n_out, first = got
    out = dst.read(n_out * cells * 2).view(np.complex64).reshape(n_out, nD, nC)
    metrics = met.read(n_out * 4).view(np.float64).reshape(n_out, 2)
    assert np.array_equal(src.read(src.words), np.ascontiguousarray(maps).view(np.uint32).reshape(-1))  # the input as it was
    return out, metrics, first


def run(b2, torch, amb, K, W, H, maps, cuts, w=None, in_off8=False, out_off8=False, integ=None):
    """A fresh integrator over the stream cut into ``cuts`` -> (out, metrics); every call's report is held to the plan."""
    own = integ is None
    integ = b2.MapIntegrator(amb, K, W, H) if own else integ
    outs, mets, at = [], [], 0
    try:
        for n, planned in zip(cuts, IC.plan(W, H, cuts)):
            o, m, first = call(torch, amb, integ, maps[:, at:at + n], w, in_off8, out_off8)
            if own:
                assert (o.shape[0], first) == (planned["n_out"], planned["first"]), (at, n)
            outs.append(o)
            mets.append(m)
            at += n
    finally:
        if own:
            integ.close()
    assert at == maps.shape[1]
    return np.concatenate(outs), np.concatenate(mets)


def cell_ratio(out, ref, K, W, tag):
    """Largest |out - ref| / bound; imaginary parts exactly 0, everything finite."""
    assert out.shape == ref.shape, (tag, out.shape, ref.shape)
    assert (out.imag == 0).all() and not np.signbit(out.imag).any(), tag
    assert np.isfinite(out.real).all(), tag
    bound = (K * W + 8) * 2.0 ** -24 * ref
    ratio = float((np.abs(out.real.astype(np.float64) - ref) / bound).max())
    print(f"{tag}: largest error / bound {ratio:.3f}")
    return ratio


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. every window, every schedule ----------------------------------------------------------------------------------------
EVERY = [("odd", W) for W in range(1, IC.MAX_WINDOW + 1)] + [("even", W) for W in (5, 9, 13, 16)]


@pytest.mark.parametrize("geom,W", EVERY, ids=[f"{g}-W{W}" for g, W in EVERY])
def test_every_window_under_every_schedule(b2, torch, geom, W):
    amb = handle(b2, geom)
    nD, nC = shape_of(amb)
    assert (nD * nC) % 2 == (1 if geom == "odd" else 0)
    N = IC.stream_length(W)
    maps = IC.maps(1, N, nD, nC, seed=2000 + 20 * W + (geom == "even"))
    ref = b2.integrate_maps(maps, None, W, 1)
    cuts = IC.schedules(W, N)
    whole, wmet = run(b2, torch, amb, 1, W, 1, maps, cuts["one-call"])
    assert cell_ratio(whole, ref, 1, W, f"nci W={W} R={IC.nci_ring(W)} {geom} N={N}") <= 1.0
    assert np.isfinite(wmet).all()
    for name in ("one-cpi", "short", "mixed"):
        out, met = run(b2, torch, amb, 1, W, 1, maps, cuts[name])
        assert same_bits(out, whole), (name, cuts[name])
        assert same_bits(met, wmet), (name, cuts[name])


# ---- 2. hops and channels ---------------------------------------------------------------------------------------------------
def weights_of(K, long_hop):
    if K == 3:
        return (0.0, 1.0, 0.0) if long_hop else (1.0, 0.25, 4.0)
    if K == 2:
        return (2.0, 0.5) if long_hop else None
    return None


HOPS = [(W, H, K) for W in (5, 9, 13, 16) for H in (W, W + 3) for K in (2, 3, 8)]


@pytest.mark.parametrize("W,H,K", HOPS, ids=[f"W{W}-H{H}-K{K}" for W, H, K in HOPS])
def test_hops_and_channels(b2, torch, W, H, K):
    amb = handle(b2, "odd")
    nD, nC = shape_of(amb)
    N = IC.stream_length(W)
    w = weights_of(K, H > W)
    maps = IC.maps(K, N, nD, nC, seed=3000 + 100 * K + 10 * W + H)
    ref = b2.integrate_maps(maps, w, W, H)
    limit = MAX_BATCH // K
    mixed, chunks = IC.clipped(IC.schedules(W, N)["mixed"], limit), IC.clipped([N], limit)
    assert mixed != chunks and max(mixed) * K <= MAX_BATCH
    out, met = run(b2, torch, amb, K, W, H, maps, mixed, w)
    assert out.shape[0] == len(b2.integrate_ends(N, W, H)) >= 2
    assert cell_ratio(out, ref, K, W, f"nci W={W} H={H} K={K} w={w}") <= 1.0
    out2, met2 = run(b2, torch, amb, K, W, H, maps, chunks, w)
    assert same_bits(out2, out) and same_bits(met2, met)


# ---- 3. alignment -----------------------------------------------------------------------------------------------------------
_aligned = {}


@pytest.mark.parametrize("geom", ["odd", "even"])
@pytest.mark.parametrize("in_off8,out_off8", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["aligned", "in+8", "out+8", "both+8"])
def test_maps_eight_bytes_off_give_the_aligned_bits(b2, torch, geom, in_off8, out_off8):
    K, W, N = 2, 3, 7
    amb = handle(b2, geom)
    nD, nC = shape_of(amb)
    maps = IC.maps(K, N, nD, nC, seed=77)
    if geom not in _aligned:
        _aligned[geom] = run(b2, torch, amb, K, W, 1, maps, [N])
        ref = b2.integrate_maps(maps, None, W, 1)
        assert cell_ratio(_aligned[geom][0], ref, K, W, f"nci aligned {geom}") <= 1.0
    want, wmet = _aligned[geom]
    for cuts in ([N], [1, 2, 4]):
        out, met = run(b2, torch, amb, K, W, 1, maps, cuts, None, in_off8, out_off8)  # (call() checks both guards)
        assert same_bits(out, want) and same_bits(met, wmet), cuts


# ---- 4. the metrics on a moving peak ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 4, 9])
def test_metrics_follow_the_moving_peak(b2, torch, W):
    K = 2
    amb = handle(b2, "odd")
    nD, nC = shape_of(amb)
    N = IC.scene_length(W, K, MAX_BATCH)
    maps, at = IC.planted(K, N, nD, nC, seed=900 + W)
    whole, wmet = run(b2, torch, amb, K, W, 1, maps, [N])
    ones, omet = run(b2, torch, amb, K, W, 1, maps, [1] * N)
    ends = b2.integrate_ends(N, W, 1)
    assert whole.shape[0] == len(ends)
    worst = [0.0, 0.0]
    for out, met in ((whole, wmet), (ones, omet)):
        for i, g in enumerate(ends):
            noise, peak = IC.set_metrics64(out[i])
            worst = [max(worst[0], abs(met[i, 0] - noise)), max(worst[1], abs(met[i, 1] - peak))]
            assert abs(met[i, 0] - noise) <= IC.DB_TOL, (g, met[i, 0], noise)
            assert abs(met[i, 1] - peak) <= IC.DB_TOL, (g, met[i, 1], peak)
            assert int(np.argmax(out[i].real)) == at[g - W + 1], g  # the window's oldest planted cell
    print(f"nci metrics on the moving peak W={W}: noisePower {worst[0]:.2e} dB, maxPower {worst[1]:.2e} dB from fp64 set_metrics")
    assert cell_ratio(whole, b2.integrate_maps(maps, None, W, 1), K, W, f"nci planted W={W}") <= 1.0
    assert same_bits(ones, whole) and same_bits(omet, wmet)


# ---- 5. below 0 dB ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 4, 9])
def test_below_0_db_the_running_max_stays_at_its_start(b2, torch, W):
    """The stream without planted cells, scaled by 1e-3: every cell lies below 0 dB (a planted cell of 1e4 would still stand
    at 10), so the maximum is the 0 the running max starts at and maxPower is -noisePower to the bit."""
    K = 2
    amb = handle(b2, "odd")
    nD, nC = shape_of(amb)
    N = IC.scene_length(W, K, MAX_BATCH)
    maps = (IC.maps(K, N, nD, nC, seed=900 + W) * np.complex64(1e-3)).astype(np.complex64)
    for cuts in ([N], [1] * N):
        out, met = run(b2, torch, amb, K, W, 1, maps, cuts)
        assert out.shape[0] == N - W + 1 and 0 < out.real.min() and out.real.max() < 1.0
        assert np.array_equal(met[:, 1].view(np.uint64), (-met[:, 0]).view(np.uint64)), cuts
        assert (met[:, 0] < -20).all()
        for i in range(out.shape[0]):
            assert abs(met[i, 0] - IC.set_metrics64(out[i])[0]) <= IC.DB_TOL
    assert cell_ratio(out, b2.integrate_maps(maps, None, W, 1), K, W, f"nci below 0 dB W={W}") <= 1.0


# ---- 6. a window that sums to zero ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["wave-seam", "last-cell"])
def test_a_zero_window_is_plus_zero_and_infinite_metrics(b2, torch, where):
    K, W, N = 2, 2, 10
    amb = handle(b2, "odd")
    nD, nC = shape_of(amb)
    cell = 127 if where == "wave-seam" else nD * nC - 1
    maps = IC.maps(K, N, nD, nC, seed=61)
    maps.reshape(K, N, -1)[:, 3:5, cell] = 0
    ref = b2.integrate_maps(maps, None, W, 1).reshape(N - 1, -1)
    integ = b2.MapIntegrator(amb, K, W, 1)
    try:
        with np.errstate(all="ignore"):
            out, met = run(b2, torch, amb, K, W, 1, maps[:, :6], [6], integ=integ)   # windows end at 1 .. 5
            later, lmet = run(b2, torch, amb, K, W, 1, maps[:, 6:], [4], integ=integ)  # ... and at 6 .. 9
    finally:
        integ.close()
    flat = out.reshape(5, -1)
    z = flat[3, cell]  # the window that ends at 4
    assert z.real == 0 and z.imag == 0 and not np.signbit(z.real) and not np.signbit(z.imag)
    assert met[3, 0] == -np.inf and met[3, 1] == np.inf
    keep = np.ones(flat.shape, dtype=bool)
    keep[3, cell] = False
    assert (flat.imag == 0).all() and np.isfinite(flat.real).all() and (flat.real[keep] > 0).all()
    bound = (K * W + 8) * 2.0 ** -24 * ref[:5]
    assert (np.abs(flat.real.astype(np.float64) - ref[:5]) <= bound)[keep].all()  # the maps ending at 3 and 5 among them
    assert ref[2, cell] > 0 and ref[4, cell] > 0 and ref[3, cell] == 0
    for i in (0, 1, 2, 4):
        noise, peak = IC.set_metrics64(out[i])
        assert np.isfinite(met[i]).all() and abs(met[i, 0] - noise) <= IC.DB_TOL and abs(met[i, 1] - peak) <= IC.DB_TOL
    # the next call on the same integrator: as if nothing had happened
    assert cell_ratio(later, ref[5:].reshape(later.shape), K, W, f"nci behind a zero window ({where})") <= 1.0
    for i in range(4):
        noise, peak = IC.set_metrics64(later[i])
        assert abs(lmet[i, 0] - noise) <= IC.DB_TOL and abs(lmet[i, 1] - peak) <= IC.DB_TOL
