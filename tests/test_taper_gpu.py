"""GPU: taper_kernel<P> (blah2hip_amb_taper_dev, Ambiguity.taper_dev) on maps whose cells all differ (tests/taper_scenes.py),
on the engine's own map and on the masking scene.  tests/test_taper_model.py shows on the CPU that the stencil is the window
and what the scene does without a GPU.

No reference counterpart; the checks are
  * cells: ``|out - ref| <= sqrt(2) (2P + 1) 2^-24 B``, ``B = sum_m |t_m| |M[j + m]|``, against the fp64 ``taper_maps`` of the
    device's own input with the fp32 taps -- the kernel's 2P + 1 roundings per component, each at most 2^-24 of B -- for every
    preset and generic taps of every half width, on four geometries, with segments of 1, 4, 5 and nD rows and the launch's
    own choice (seams, the wrap inside a segment and at a seam), 6 maps a call;
  * placement: input and output 8 bytes off a 16-byte boundary in every combination give the aligned call's bits;
  * cuts: one call of 6 maps against calls of 1, 2 and 3: maps and metrics bit for bit;
  * pass-through: n_side 0 with t_0 = 1 copies the cells; metrics within 1e-3 dB of the engine's own;
  * metrics: 1e-3 dB (the project's gate) against fp64 Map::set_metrics of the device's own output, a planted peak on the strip
    and segment seams;
  * NaN: one NaN cell makes exactly the 2P + 1 cells of its column that hold it NaN, that map's metrics NaN, nothing else;
  * refusals: every BLAH2HIP_ERR_INVALID case writes nothing;
  * chain: the engine's map of oracle.synth_iq, tapered, against the oracle of the windowed pulses by the triangle inequality
    ``|D'| <= sum_m |t_m| |D[j + m]| + sqrt(2) (2P + 1) 2^-24 B + 1e-12 peak`` (D, D': device minus oracle before and behind
    the taper; the oracle's window is the one the fp32 taps make, w[i] = t_0 + 2 sum_m t_m cos(2 pi m i / nD), so that no
    rounding of the taps enters); then the 1-D detector and the finisher on the tapered pair against the oracle's detector
    and the host's Centroid and Interpolate on the device's own tapered cells;
  * masking: the scene's three maps, tapered with Blackman on the device, through CfarDetector1D.process_dev: no stray, the
    weak echo present; untapered at least 80 strays.
Every output lies in an arena with guard words in front and behind; so does every input.

Measured on the MI355X (printed by the tests).  Cells, largest error / bound over the twelve stencils of a case: 0.655 .. 0.660
in all twenty (geometry, segment) cases.  Metrics on the planted peak, largest distance from fp64 set_metrics of the device's
own cells (noisePower, maxPower), dB: 1.00e-7, 4.40e-6 (thin, segments of 4); 9.53e-8, 4.57e-6 (odd, 5); 9.53e-8, 3.97e-6 (odd,
own choice).  Chain, largest |device - oracle| over its limit behind the taper: 0.945 (hamming), 0.911 (blackman), 0.788
(flattop), with the engine's map 9.55e-8 of the peak from the oracle in front of it.  Masking scene: 86, 86, 86 strays untapered,
0, 0, 0 with Blackman, the weak echo found in all six.  Every placement and every cut gave the bits of the one aligned call.
No defect was found.
"""
import ctypes as C

import numpy as np
import pytest

import taper_scenes as TS
from oracle import blah2_oracle as O
from oracle.gates import MARGIN_EPS_MIN, cfar1d_margins, detection_gate

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces
PAD = 64                       # guard words on either side; a multiple of four, so that the data keep the base's alignment
MAX_BATCH = 8
N_MAPS = 6
SEVEN = ((-10, 100, -30, 30, 1_000_000, 100_000), 0)  # 7 x 111: too few rows for n_side 4
GENERIC = {P: np.array([0.6, -0.31, 0.17, -0.09, 0.04][:P + 1], dtype=np.float32) for P in range(5)}


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
        limits, bins = SEVEN if name == "seven" else TS.GEOMS[name]
        _handles[name] = b2.Ambiguity(*limits, True, max_batch=MAX_BATCH, n_doppler_bins=bins)
        if name in TS.SHAPES:
            assert shape_of(_handles[name]) == TS.SHAPES[name]
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
        """The first ``used_words`` of the data (uint32) after checking that nothing else was written."""
        host = self.whole.cpu().numpy().view(np.uint32)
        assert (host[:self.front] == GUARD).all(), "the guard in front was written"
        assert (host[self.front + self.words:] == GUARD).all(), "the guard behind was written"
        assert (host[self.front + used_words:self.front + self.words] == GUARD).all(), "written behind the output"
        return host[self.front:self.front + used_words].copy()


def taper(torch, amb, maps, taps, seg=0, in_off8=False, out_off8=False):
    """One call over maps [n, nD, nC] -> (out complex64 [n, nD, nC], metrics [n, 2])."""
    n, nD, nC = maps.shape
    assert (nD, nC) == shape_of(amb)
    src = Arena(torch, maps.size * 2, in_off8)
    src.fill(torch, maps)
    dst = Arena(torch, maps.size * 2, out_off8)
    met = Arena(torch, n * 4)
    amb.set_taper_seg_rows(seg)
    amb.taper_dev(src.ptr, n, taps, dst.ptr, met.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    strips, rows = -(-nC // 256), min(seg, nD) if seg else min(32, nD)
    assert amb.info(amb_info("INFO_TAPER_GRID")) == strips * -(-nD // rows)
    out = dst.read(maps.size * 2).view(np.complex64).reshape(n, nD, nC)
    metrics = met.read(n * 4).view(np.float64).reshape(n, 2)
    assert np.array_equal(src.read(src.words), np.ascontiguousarray(maps).view(np.uint32).reshape(-1))  # the input as it was
    return out, metrics


def amb_info(name):
    from blah2_amd import _lib
    return getattr(_lib, name)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def f64_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def cell_ratio(b2, out, maps, taps, tag):
    """Largest |out - ref| / bound against the fp64 stencil of the same input with the same fp32 taps."""
    taps = np.asarray(taps, dtype=np.float32)
    ref = b2.taper_maps(maps, taps.astype(np.float64))
    err = np.abs(out.astype(np.complex128) - ref)
    ratio = float((err / TS.cell_bound(maps, taps)).max())
    assert np.isfinite(out.view(np.float32)).all(), tag
    return ratio


def all_taps(b2, nD):
    cases = [(name, b2.doppler_taper_f32(name)) for name in TS.PRESETS] + [("hamming:norm", b2.doppler_taper_f32("hamming", True))]
    cases += [(f"generic-P{P}", t) for P, t in GENERIC.items()]
    return [(k, t) for k, t in cases if nD >= 2 * len(t) - 1]


# ---- 1. cells ---------------------------------------------------------------------------------------------------------------
def seg_rows(name):
    nD = TS.SHAPES[name][0]
    return [1, 4, 5, nD, 0]


CELLS = [(g, s) for g in TS.SHAPES for s in seg_rows(g)]


@pytest.mark.parametrize("geom,seg", CELLS, ids=[f"{g}-seg{s}" for g, s in CELLS])
def test_cells_of_every_stencil(b2, torch, geom, seg):
    amb = handle(b2, geom)
    nD, nC = shape_of(amb)
    maps = TS.maps(N_MAPS, nD, nC, seed=400 + 7 * seg + len(geom))
    cases = all_taps(b2, nD)
    assert {len(t) - 1 for _, t in cases} == {0, 1, 2, 3, 4}
    worst = 0.0
    for name, taps in cases:
        out, met = taper(torch, amb, maps, taps, seg)
        r = cell_ratio(b2, out, maps, taps, (geom, seg, name))
        worst = max(worst, r)
        assert r <= 1.0, (geom, seg, name, r)
        for i in range(N_MAPS):
            noise, peak = TS.set_metrics64(out[i])
            assert abs(met[i, 0] - noise) <= TS.DB_TOL and abs(met[i, 1] - peak) <= TS.DB_TOL, (geom, seg, name, i)
    print(f"taper {geom} {nD} x {nC} seg {seg}: largest error / bound {worst:.3f} over {len(cases)} stencils")


# ---- 2. placement -----------------------------------------------------------------------------------------------------------
_aligned = {}


@pytest.mark.parametrize("geom", ["odd", "even", "thin"])
@pytest.mark.parametrize("in_off8,out_off8", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["aligned", "in+8", "out+8", "both+8"])
def test_maps_eight_bytes_off_give_the_aligned_bits(b2, torch, geom, in_off8, out_off8):
    amb = handle(b2, geom)
    nD, nC = shape_of(amb)
    maps = TS.maps(N_MAPS, nD, nC, seed=77)
    for name in ("hann", "flattop"):
        taps = b2.doppler_taper_f32(name)
        for seg in (0, 4):
            key = (geom, name, seg)
            if key not in _aligned:
                _aligned[key] = taper(torch, amb, maps, taps, seg)
                assert cell_ratio(b2, _aligned[key][0], maps, taps, key) <= 1.0
            out, met = taper(torch, amb, maps, taps, seg, in_off8, out_off8)  # (taper() checks both guards)
            assert same_bits(out, _aligned[key][0]) and f64_bits(met, _aligned[key][1]), key


# ---- 3. cuts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["odd", "thin"])
def test_cuts_into_calls_give_the_same_bits(b2, torch, geom):
    amb = handle(b2, geom)
    nD, nC = shape_of(amb)
    maps = TS.maps(N_MAPS, nD, nC, seed=91)
    taps = b2.doppler_taper_f32("blackmanharris")
    for seg in (0, 4):
        whole, wmet = taper(torch, amb, maps, taps, seg)
        outs, mets, at = [], [], 0
        for n in (1, 2, 3):
            o, m = taper(torch, amb, maps[at:at + n], taps, seg, in_off8=bool(at & 1))
            outs.append(o)
            mets.append(m)
            at += n
        assert at == N_MAPS
        assert same_bits(np.concatenate(outs), whole) and f64_bits(np.concatenate(mets), wmet), seg


# ---- 4. the metrics on a planted peak ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,seg", [("thin", 4), ("odd", 5), ("odd", 0)])
def test_metrics_follow_a_planted_peak(b2, torch, geom, seg):
    """One cell per map 80 dB above the rest, on the first and last column of a strip, of a wave, of a segment's first and
    last row: the map's maximum is found whichever workgroup and lane owns it."""
    amb = handle(b2, geom)
    nD, nC = shape_of(amb)
    rows = sorted({0, max(seg, 1) - 1, max(seg, 1) % nD, nD - 1, nD // 2, 1})
    cols = [c for c in (0, 63, 64, 255, 256, nC - 1) if c < nC]
    places = [(rows[i % len(rows)], cols[i % len(cols)]) for i in range(N_MAPS)] + \
             [(rows[(i + 1) % len(rows)], cols[-1 - i % len(cols)]) for i in range(N_MAPS)]
    taps = b2.doppler_taper_f32("blackman")
    worst = [0.0, 0.0]
    for half in (places[:N_MAPS], places[N_MAPS:]):
        maps = TS.maps(N_MAPS, nD, nC, seed=55)
        for i, (r, c) in enumerate(half):
            maps[i, r, c] *= np.float32(1e4)
        out, met = taper(torch, amb, maps, taps, seg)
        for i, (r, c) in enumerate(half):
            noise, peak = TS.set_metrics64(out[i])
            worst = [max(worst[0], abs(met[i, 0] - noise)), max(worst[1], abs(met[i, 1] - peak))]
            assert abs(met[i, 0] - noise) <= TS.DB_TOL and abs(met[i, 1] - peak) <= TS.DB_TOL, (i, r, c)
            assert np.unravel_index(int(np.argmax(np.abs(out[i]))), (nD, nC)) == (r, c)
            assert peak > 30.0
    print(f"taper metrics on a planted peak {geom} seg {seg}: noisePower {worst[0]:.2e} dB, maxPower {worst[1]:.2e} dB from fp64 set_metrics")


# ---- 5. NaN -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,name,row,col,seg", [("odd", "blackman", 0, 110, 4), ("odd", "flattop", 19, 0, 5),
                                                   ("thin", "flattop", 3, 256, 4), ("even16", "hann", 15, 64, 0),
                                                   ("odd", "none", 7, 31, 0)])
def test_a_nan_cell_spreads_over_its_stencil_only(b2, torch, geom, name, row, col, seg):
    amb = handle(b2, geom)
    nD, nC = shape_of(amb)
    taps = b2.doppler_taper_f32(name)
    P = len(taps) - 1
    maps = TS.maps(N_MAPS, nD, nC, seed=13)
    clean, cmet = taper(torch, amb, maps, taps, seg)
    bad = maps.copy()
    bad[2, row, col] = np.complex64(complex(np.nan, np.nan))
    out, met = taper(torch, amb, bad, taps, seg)  # (the guards are checked there)
    want = np.zeros((nD, nC), dtype=bool)
    want[[(row + k) % nD for k in range(-P, P + 1)], col] = True
    assert int(want.sum()) == 2 * P + 1
    assert np.array_equal(np.isnan(out[2]), want)
    assert same_bits(out[2][~want], clean[2][~want])
    assert np.isnan(met[2]).all()
    keep = [0, 1, 3, 4, 5]
    assert same_bits(out[keep], clean[keep]) and f64_bits(met[keep], cmet[keep])


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(b2, torch):
    from blah2_amd import _lib
    L = _lib.load()
    amb = handle(b2, "odd")
    nD, nC = shape_of(amb)
    cells = nD * nC
    n = 2
    src = Arena(torch, n * cells * 2)
    src.fill(torch, TS.maps(n, nD, nC, seed=3))
    dst = Arena(torch, n * cells * 2)
    met = Arena(torch, n * 4)
    st = torch.cuda.current_stream().cuda_stream
    good = np.array([0.5, -0.25], dtype=np.float32)
    five = np.zeros(6, dtype=np.float32)
    nan, inf = np.array([0.5, np.nan], dtype=np.float32), np.array([np.inf, 0.1], dtype=np.float32)

    def p(a):
        return a.ctypes.data_as(C.c_void_p)

    base = [amb._h, src.ptr, n, p(good), 1, dst.ptr, met.ptr, st]
    cases = {"n_side above 4": {3: p(five), 4: 5}, "n_maps 0": {2: 0}, "n_maps above max_batch": {2: MAX_BATCH + 1},
             "NULL taps": {3: None}, "NULL map": {5: None}, "NULL metrics": {6: None}, "a NaN tap": {3: p(nan)},
             "an infinite tap": {3: p(inf)}, "output = input": {5: src.ptr}, "output on the input's last cell": {5: src.ptr + 8 * (n * cells - 1)},
             "output ends on the input's first cell": {1: dst.ptr + 8 * (n * cells - 1)}, "metrics inside the input": {6: src.ptr + 16},
             "a map 4 bytes off": {5: dst.ptr + 4}, "NULL handle": {0: None}}
    for why, change in cases.items():
        args = list(base)
        for k, v in change.items():
            args[k] = v
        assert L.blah2hip_amb_taper_dev(*args) == _lib.ERR_INVALID, why
    # the handle's own map as the input (d_map NULL), and as the output of that
    own = C.c_void_p()
    ownmet = C.c_void_p()
    assert L.blah2hip_amb_result_ptrs(amb._h, C.byref(own), C.byref(ownmet)) == _lib.OK
    assert L.blah2hip_amb_taper_dev(amb._h, None, n, p(good), 1, own.value + 8 * cells, met.ptr, st) == _lib.ERR_INVALID
    # nD = 7: n_side 3 is the largest stencil
    seven = handle(b2, "seven")
    assert shape_of(seven) == (7, 111)
    t4 = b2.doppler_taper_f32("flattop")
    assert L.blah2hip_amb_taper_dev(seven._h, src.ptr, 1, p(t4), 4, dst.ptr, met.ptr, st) == _lib.ERR_INVALID
    assert b"Doppler bins" in L.blah2hip_last_error()
    with pytest.raises(b2.Blah2HipError):
        seven.taper_dev(src.ptr, 1, t4, dst.ptr, met.ptr, st)
    with pytest.raises(ValueError):
        amb.taper_dev(src.ptr, 1, [], dst.ptr, met.ptr, st)
    for bad in (-1, 65536):
        with pytest.raises(b2.Blah2HipError):
            amb.set_taper_seg_rows(bad)
    torch.cuda.synchronize()
    dst.read(0)
    met.read(0)
    # ... and the same buffers take the good call, and n_side 3 on the seven rows
    assert L.blah2hip_amb_taper_dev(*base) == _lib.OK
    t3 = b2.doppler_taper_f32("nuttall")
    m7 = TS.maps(1, 7, 111, seed=4)
    out, _ = taper(torch, seven, m7, t3, 0)
    assert cell_ratio(b2, out, m7, t3, "seven") <= 1.0


# ---- 7. the engine's map: pass-through, the chain's triangle inequality, the detector and the finisher -------------------------
@pytest.fixture(scope="module")
def engine(b2, torch):
    """(x, y, device map [1, nD, nC] complex64, metrics [1, 2]) of oracle.synth_iq through process_dev at the odd geometry."""
    limits, _ = TS.GEOMS["odd"]
    n, fs = limits[5], limits[4]
    x, y = O.synth_iq(n, targets=((37, -60.0, 0.05),), fs=fs)
    amb = handle(b2, "odd")
    nD, nC = shape_of(amb)
    d_x = torch.from_numpy(x.astype(np.complex64)).cuda()
    d_y = torch.from_numpy(y.astype(np.complex64)).cuda()
    d_map = torch.zeros((1, nD, nC), dtype=torch.complex64, device="cuda")
    d_met = torch.zeros((1, 2), dtype=torch.float64, device="cuda")
    amb.process_dev(b2.FMT_C32, d_x.data_ptr(), d_y.data_ptr(), 1, n, d_map.data_ptr(), d_met.data_ptr(),
                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return x, y, d_map.cpu().numpy(), d_met.cpu().numpy()


def test_pass_through_copies_the_cells(b2, torch, engine):
    _, _, m, met = engine
    amb = handle(b2, "odd")
    for seg in (0, 1, 5):
        for off in (False, True):
            out, tmet = taper(torch, amb, m, [1.0], seg, in_off8=off, out_off8=not off)
            assert same_bits(out, m)
            assert np.abs(tmet - met).max() <= TS.DB_TOL, (tmet, met)
    crafted = TS.maps(N_MAPS, *shape_of(amb), seed=8)
    crafted[1, 3, 5] = 0                       # +0 stays +0: its level is -inf
    crafted[4, 0, 0] = np.complex64(-0.0)
    with np.errstate(all="ignore"):
        out, tmet = taper(torch, amb, crafted, b2.doppler_taper_f32("none"), 4)
    assert same_bits(out, crafted)
    assert tmet[1, 0] == -np.inf and tmet[1, 1] == np.inf and np.isfinite(tmet[[0, 2, 3, 5]]).all()


@pytest.mark.parametrize("name", ["hamming", "blackman", "flattop"])
def test_chain_against_the_oracle_of_the_windowed_pulses(b2, torch, engine, name):
    x, y, m, met = engine
    limits, _ = TS.GEOMS["odd"]
    amb = handle(b2, "odd")
    dims = O.ambiguity_dims(*limits, True)
    nD = dims.n_doppler_bins
    taps = b2.doppler_taper_f32(name)
    t64 = taps.astype(np.float64)
    P = len(taps) - 1
    out, tmet = taper(torch, amb, m, taps, 0)
    # the window the fp32 taps make, on the pulses
    i = np.arange(nD)
    w = t64[0] + 2.0 * sum(t64[k] * np.cos(2.0 * np.pi * k * i / nD) for k in range(1, P + 1))
    assert np.abs(w - b2.doppler_window(name, nD)).max() < 1e-7
    pulse = np.minimum(np.arange(x.size) // dims.n_corr, nD - 1)
    plain = O.ambiguity_process(dims, x, y)
    windowed = O.ambiguity_process(dims, x, y * w[pulse])
    d0 = np.abs(m[0].astype(np.complex128) - plain)
    d1 = np.abs(out[0].astype(np.complex128) - windowed)
    spread = t64[0] * d0
    for k in range(1, P + 1):
        spread = spread + abs(t64[k]) * (np.roll(d0, k, axis=0) + np.roll(d0, -k, axis=0))
    limit = spread + TS.cell_bound(m[0], taps) + 1e-12 * np.abs(windowed).max()
    print(f"chain {name}: largest |device - oracle| / limit behind the taper {float((d1 / limit).max()):.3f}; "
          f"{float(d0.max() / np.abs(plain).max()):.2e} of the peak in front of it, {float(d1.max() / np.abs(windowed).max()):.2e} behind")
    assert (d1 <= limit).all()
    noise, peak = TS.set_metrics64(out[0])
    assert abs(tmet[0, 0] - noise) <= TS.DB_TOL and abs(tmet[0, 1] - peak) <= TS.DB_TOL

    # the detector and the finisher on the tapered pair, against the oracle's detector and the host's Centroid and
    # Interpolate on the device's own tapered cells
    pfa, ng, nt, md, mdop = 1e-3, 2, 6, 5, 15.0
    n, fs = limits[5], limits[4]
    cells = out[0].size
    st = torch.cuda.current_stream().cuda_stream
    d_map = torch.from_numpy(out.copy()).cuda()
    d_met = torch.from_numpy(tmet.copy()).cuda()
    d_hits = torch.zeros((1, cells, 2), dtype=torch.float64, device="cuda")
    d_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_out = torch.zeros((1, cells, 4), dtype=torch.float64, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
    det = b2.CfarDetector1D(pfa, ng, nt, md, mdop)
    det.process_dev(amb, 1, d_hits.data_ptr(), cells, d_cnt.data_ptr(), d_map.data_ptr(), d_met.data_ptr(), st)
    b2.DetectionFinisher(6, 6, 1 / (n / fs), True, True).process_dev(amb, 1, d_hits.data_ptr(), cells, d_cnt.data_ptr(), d_out.data_ptr(),
                                                                    cells, d_n.data_ptr(), d_map.data_ptr(), d_met.data_ptr(), st)
    torch.cuda.synchronize()
    k = int(d_cnt.cpu()[0])
    got = b2.hits_to_detection(amb, d_hits[0].cpu().numpy().view(b2.HIT_DTYPE).reshape(-1), k, cells)
    dl, dp, sn = O.cfar1d_fast(out[0], amb.delay, amb.doppler, tmet[0, 0], pfa, ng, nt, md, mdop)
    mg = cfar1d_margins(out[0], pfa, ng, nt)
    dg = detection_gate(zip(dl, dp), zip(got.get_delay(), got.get_doppler()), mg, amb.doppler, amb.delay[0], MARGIN_EPS_MIN)
    assert dg["ok"] and dg["n_ref"] > 0, dg
    step = float(amb.doppler[1] - amb.doppler[0])
    echo = (np.abs(got.get_delay() - 37) < 0.5) & (np.abs(got.get_doppler() + 60.0) < step)
    assert echo.any(), "the echo is missing from the tapered map's detections"
    host_map = b2.Map(amb, out[0], amb.delay, amb.doppler, float(tmet[0, 0]), float(tmet[0, 1]), 0)
    ref = b2.Interpolate(True, True).process(b2.Centroid(6, 6, 1 / (n / fs)).process(got), host_map)
    fin = b2.dets_to_detection(d_out[0].cpu().numpy().view(b2.DET_DTYPE).reshape(-1), int(d_n.cpu()[0]), cells)
    assert fin.get_nDetections() == ref.get_nDetections() > 0
    assert np.allclose(fin.get_delay(), ref.get_delay(), rtol=0, atol=1e-9)
    assert np.allclose(fin.get_doppler() / step, ref.get_doppler() / step, rtol=0, atol=1e-9)
    assert np.allclose(fin.get_snr(), ref.get_snr(), rtol=0, atol=1e-9)


# ---- 8. the masking scene on the device -------------------------------------------------------------------------------------
def test_masking_scene_on_the_device(b2, torch):
    nP, nB = TS.SCENE_PULSES, TS.SCENE_BINS
    amb = b2.Ambiguity(0, nB - 1, -50, 50, 1_000_000, 1_000_000, True, max_batch=len(TS.SCENE_SEEDS))
    try:
        assert shape_of(amb) == (nP, nB)
        maps = np.stack([TS.scene_map(s) for s in TS.SCENE_SEEDS]).astype(np.complex64)
        n = maps.shape[0]
        cells = nP * nB
        st = torch.cuda.current_stream().cuda_stream
        plain, pmet = taper(torch, amb, maps, [1.0], 0)  # (the metrics of the untapered maps)
        assert same_bits(plain, maps)
        tapered, tmet = taper(torch, amb, maps, b2.doppler_taper_f32("blackman"), 0)
        det = b2.CfarDetector1D(TS.SCENE_CFAR["pfa"], TS.SCENE_CFAR["n_guard"], TS.SCENE_CFAR["n_train"], 0, 0.0)
        verdicts = {}
        for tag, m, met in (("none", plain, pmet), ("blackman", tapered, tmet)):
            d_map, d_met = torch.from_numpy(m.copy()).cuda(), torch.from_numpy(met.copy()).cuda()
            d_hits = torch.zeros((n, cells, 2), dtype=torch.float64, device="cuda")
            d_cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
            det.process_dev(amb, n, d_hits.data_ptr(), cells, d_cnt.data_ptr(), d_map.data_ptr(), d_met.data_ptr(), st)
            torch.cuda.synchronize()
            for i in range(n):
                h = d_hits[i].cpu().numpy().view(b2.HIT_DTYPE).reshape(-1)[:int(d_cnt[i])]
                verdicts[tag, i] = TS.scene_verdict(h["col"], h["row"] - float((nP - 1) // 2))
        print("masking scene on the device (strays, weak echo):", verdicts)
        for i in range(n):
            assert verdicts["none", i][0] >= 80 and verdicts["none", i][1]
            assert verdicts["blackman", i] == (0, True)
    finally:
        amb.close()
