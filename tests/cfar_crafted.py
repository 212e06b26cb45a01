"""Crafted inputs for the detector kernels (csrc/cfar_kernels.hpp), shared by the CPU pin in test_oracle_properties.py
and by test_cfar_crafted_gpu.py: what the CPU test checks (no tested cell of any input within 1e-9 of its threshold, at
most 1 % of the hits inside the summed-area band) is what the GPU module runs.

A case is a map shape with its axes (the arguments of ``Ambiguity``), a window, the detector's parameters and a seeded
map flavour.  Maps never come from the ambiguity engine: the detectors' ``process_dev`` take any device map.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from oracle import blah2_oracle as O

# (nGd, nTd, nGf, nTf).  C2S_SHAPES in csrc/cfar_kernels.hpp lists the same nine as (nTd, nGd, nTf, nGf).
STREAM_SHAPES = [(2, 6, 1, 3), (2, 6, 0, 0), (2, 8, 1, 4), (1, 4, 1, 2), (1, 3, 1, 2), (0, 1, 0, 0), (0, 0, 0, 1),
                 (0, 2, 0, 1), (2, 5, 2, 6)]
TILE_NL3 = (6, 34, 2, 4)      # halo of 40 columns: three loads per row, the widest the tile kernel takes
TILE_NOLDS = (5, 27, 3, 21)   # 65 x 49 window: two loads per row, threshold table too long for the LDS
SAT_ONLY = (9, 40, 5, 20)     # halo 49 x 25: beyond the tile kernel
WINDOWS = STREAM_SHAPES + [TILE_NL3, TILE_NOLDS, SAT_ONLY]
BAND = 1e-9                   # additive kernels; fp64 bound for a sum of 81 x 49 non-negative terms: 4e-13
N_CORR = 1024


def stream_ring(w):
    """Rows per round of the stream kernel's unrolled loop (c2s_ring in csrc/cfar_kernels.hpp, C2S_V = 2)."""
    return (2 + w[3] + 2 * w[2] + 1 + 1) // 2 * 2


def kernels_for(w):
    """The forced kernels that take window ``w``; 'auto' runs besides."""
    out = []
    if w[2] + w[3] <= 24 and w[0] + w[1] <= 40:
        out.append("tile")
    if tuple(w) in STREAM_SHAPES:
        out.append("stream")
    return out + ["sat", "auto"]


def geom(nD, nC, delay_min=None, n_corr=N_CORR):
    """Ambiguity arguments of an nD x nC map on a symmetric 1 Hz axis (delayMin <= 1 and delayMax >= -1 are the
    engine's own limits)."""
    if delay_min is None:
        delay_min = -min(3, nC - 1)
    n = nD * n_corr
    return (delay_min, delay_min + nC - 1, -1000, 1000, n, n, nD)


ASYM = (-10, 100, -7, 30, 100_000, 100_000, 0)     # one-sided axis: -6.5 ... 29.5 Hz, 37 rows
MIRROR = (-10, 100, -30, 7, 100_000, 100_000, 0)
ASYM_EVEN = ASYM[:6] + (36,)
MIRROR_EVEN = MIRROR[:6] + (36,)


@dataclass(frozen=True)
class Case:
    name: str
    geom: tuple            # delayMin, delayMax, dopplerMin, dopplerMax, fs, n, n_doppler_bins (0 = the reference's rule)
    window: tuple          # (nGd, nTd, nGf, nTf), or (nGuard, nTrain) for the 1-D detector
    pfa: float = 0.02
    min_delay: int = -128
    min_doppler: float = 0.0
    B: int = 1
    kind: str = "floor"    # floor | range | zero | holes | nonfinite
    seg_rows: int = 0      # BLAH2HIP_OPT_CFAR2D_SEG_ROWS
    grid: int = 0          # BLAH2HIP_OPT_CFAR2D_GRID
    only: tuple = ()       # restrict the kernels

    @property
    def one_d(self):
        return len(self.window) == 2

    @property
    def w4(self):
        return tuple(self.window) if not self.one_d else (self.window[0], self.window[1], 0, 0)

    def kernels(self):
        if self.one_d:
            return ["1d"]
        k = kernels_for(self.window)
        return [x for x in k if x in self.only] if self.only else k


@lru_cache(maxsize=None)
def dims_of(g):
    return O.ambiguity_dims(g[0], g[1], g[2], g[3], g[4], g[5], False, g[6])


def _seams(n, steps):
    out = {0, 1, n - 2, n - 1, n // 2}
    for s in steps:
        if s > 0:
            for k in range(s, n + 2, s):
                out.update((k - 1, k, k + 1))
    return sorted(v for v in out if 0 <= v < n)


def make_maps(case):
    """(maps complex64 [B, nD, nC], metrics float64 [B, 2]): an exponential power floor, planted cells 10 - 60 dB (power) up
    at random places and on edges, corners, columns 0 / 1 and the seams of strips, tiles and segments."""
    d = dims_of(case.geom)
    nD, nC, B = d.n_doppler_bins, d.n_delay_bins, case.B
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    w = case.w4
    hC, hR = w[0] + w[1], w[2] + w[3]
    amp = np.sqrt(rng.exponential(1.0, (B, nD, nC)))
    if case.kind == "range":  # 1e-20 ... 1e18 in magnitude, rising along the map: an fp32 |z|^2 flushes at one end, its sums overflow at the other
        t = (np.arange(nD)[:, None] * nC + np.arange(nC)[None, :]) / max(nD * nC - 1, 1)
        amp = amp / amp.max() * 10.0 ** (-20.0 + 38.0 * t)[None]
    rows = _seams(nD, (8, 16, 64 - 2 * hR, case.seg_rows, stream_ring(w)))
    cols = _seams(nC, (64, 64 - 2 * hC if hC < 24 else 0))
    for c in range(B):
        k = min(40, max(nD * nC // 6, 1))
        ii = np.concatenate([rng.integers(0, nD, k), rng.choice(rows, k), rng.integers(0, nD, k)])
        jj = np.concatenate([rng.integers(0, nC, k), rng.integers(0, nC, k), rng.choice(cols, k)])
        gain = 10.0 ** (rng.uniform(10.0, 60.0, ii.size) / 20.0)
        if case.kind == "range":
            gain = np.minimum(gain, 1e18 / amp[c, ii, jj])
        amp[c, ii, jj] *= gain
    if case.kind == "range":
        amp[:, 0, 0], amp[:, -1, -1] = 1e-20, 1e18
    m = amp * np.exp(2j * np.pi * rng.uniform(0, 1, amp.shape))
    if case.kind == "zero":
        m[:] = 0
    if case.kind == "holes":  # isolated zero cells: no two are neighbours
        hole = rng.uniform(0, 1, amp.shape) < 0.3
        hole[:, ::2, :] = False
        hole[:, :, ::2] = False
        m[hole] = 0
    m = m.astype(np.complex64)
    if case.kind == "nonfinite":
        m[:, nD // 3, nC // 3] = np.complex64(complex(np.nan, 1.0))
        m[:, (2 * nD) // 3, (2 * nC) // 3] = np.complex64(complex(np.inf, 0.0))
    metrics = np.stack([3.0 + 7.5 * np.arange(B), 1.0 + np.arange(B)], axis=1).astype(np.float64)
    return m, metrics


@dataclass
class Expected:
    hits: list          # per CPI: {(row, col): snr}
    margin: list        # per CPI: |z|^2 / threshold, [nD, nC]
    tested: np.ndarray  # [nD, nC] cells the detector tests (minDelay, minDoppler)
    in_band: int        # tested cells within BAND of their threshold, all CPIs
    sat_band: list      # per CPI: the summed-area kernels' band per cell
    sat_share: float    # largest share of a CPI's hits inside its summed-area band


def expected(case, maps=None, metrics=None):
    """The oracle's answer for ``case`` and the two conditions on the input."""
    if maps is None:
        maps, metrics = make_maps(case)
    d = dims_of(case.geom)
    w = case.w4
    nD, nC = d.n_doppler_bins, d.n_delay_bins
    row_of = {f: i for i, f in enumerate(d.doppler)}
    assert len(row_of) == nD
    tested = (np.abs(d.doppler) >= case.min_doppler)[:, None] & (d.delay >= case.min_delay)[None, :]
    i = np.arange(nD)
    j = np.arange(nC)
    R1 = np.clip(i + w[2] + w[3] + 1, 0, nD)
    C1 = np.clip(j + w[0] + w[1] + 1, 0, nC)
    out = Expected([], [], tested, 0, [], 0.0)
    for c in range(maps.shape[0]):
        m = maps[c].astype(np.complex128)
        dl, dp, sn, mg = O.cfar2d_additive(m, d.delay, d.doppler, metrics[c, 0], case.pfa, *w, case.min_delay,
                                           case.min_doppler, return_margin=True)
        hits = {(row_of[f], int(a - d.delay[0])): s for a, f, s in zip(dl, dp, sn)}
        assert len(hits) == len(dl)
        if case.one_d and case.kind != "nonfinite":  # the reference's own loop gives the same list (its abs(z*z) makes an infinite cell NaN)
            dl1, dp1, sn1 = O.cfar1d(m, d.delay, d.doppler, metrics[c, 0], case.pfa, w[0], w[1], case.min_delay,
                                     case.min_doppler)
            assert np.array_equal(dl1, dl) and np.array_equal(dp1, dp)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            out.in_band += int(np.count_nonzero((np.abs(mg - 1.0) < BAND) & tested))
            # summed-area kernels: 8 ulp of the table's value at the window's far corner, relative to the window sum
            sq = m.real * m.real + m.imag * m.imag
            z = sq.copy()
            z[:, 0] = 0.0
            sat = np.zeros((nD + 1, nC + 1))
            sat[1:, 1:] = np.cumsum(np.cumsum(z, axis=0), axis=1)
            tot = O.cfar2d_window_sums(sq, *w)
            band = 8.0 * 2.0 ** -52 * sat[R1][:, C1] / tot
            inb = ~(np.abs(mg - 1.0) >= band)  # a NaN band (empty or all-zero window) counts as inside
        out.hits.append(hits)
        out.margin.append(mg)
        out.sat_band.append(inb)
        if hits:
            share = sum(1 for k in hits if inb[k]) / len(hits)
            out.sat_share = max(out.sat_share, share)
    return out


# ---------------------------------------------------------------------------------------------------- the cases --
def shape_cases(w):
    """Map shapes at the kernels' own boundaries for window ``w`` (a star: every nDelay at one nD, every nD at one
    nDelay, and the corners), all cells tested."""
    hC, hR = w[0] + w[1], w[2] + w[3]
    outw = 64 - 2 * hC
    rows_out = 64 - 2 * hR
    nC_list = {1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257}
    if outw >= 16:
        nC_list |= {outw - 1, outw, outw + 1}
    nD_list = {1, 2, hR, 2 * hR, 2 * hR + 1, 7, 8, 9, rows_out - 1, rows_out, rows_out + 1}
    shapes = [(11, c) for c in sorted(nC_list)] + [(r, 70) for r in sorted(nD_list) if r > 0]
    shapes += [(1, 1), (2, 2), (rows_out + 1, 129)]
    tag = "w" + "_".join(map(str, w))
    return [Case(f"shape-{tag}-{r}x{c}", geom(r, c), w) for r, c in shapes]


def seg_cases():
    out = []
    for w in ((2, 6, 1, 3), (2, 5, 2, 6)):
        hR, U, nD = w[2] + w[3], stream_ring(w), 70
        for B in (1, 3):
            out.append(Case(f"seg-w{w[1]}-auto-B{B}", geom(nD, 130), w, B=B))  # every kernel, batch of distinct maps
            for s in sorted({1, 2, hR, U - 1, U, U + 1, 8, 33, nD - 1, nD}):
                out.append(Case(f"seg-w{w[1]}-{s}-B{B}", geom(nD, 130), w, B=B, seg_rows=s, only=("stream",)))
    return out


def grid_cases():
    return [Case(f"grid-NL{nl}-B{B}", geom(170, 650), w, B=B, grid=8, only=("tile",), pfa=1e-3)
            for nl, w in ((2, (2, 6, 1, 3)), (3, TILE_NL3)) for B in (1, 2)]


def dead_row_cases():
    out = []
    for gname, g in (("asym", ASYM), ("mirror", MIRROR), ("asym-even", ASYM_EVEN), ("mirror-even", MIRROR_EVEN)):
        f = np.abs(dims_of(g).doppler)
        near = np.sort(f)
        values = {"zero": 0.0, "at-edge": float(f[0] if f[0] < f[-1] else f[-1]), "at-4": float(near[4]),
                  "between": float(0.5 * (near[6] + near[7])), "touching": float(0.5 * (near[12] + near[14])),
                  "above": float(f.max() + 1.0)}
        for vname, v in values.items():
            out.append(Case(f"dead-{gname}-{vname}", g, (2, 6, 1, 3), min_doppler=v, min_delay=-3))
            out.append(Case(f"dead1d-{gname}-{vname}", g, (2, 6), min_doppler=v, min_delay=-3))
        out.append(Case(f"dead-{gname}-w0001-at-4", g, (0, 0, 0, 1), min_doppler=float(near[4])))
    return out


def min_delay_cases():
    out = []
    for gname, g in (("neg", geom(21, 71, -10)), ("pos", geom(21, 70, 1))):
        dmin, dmax = g[0], g[1]
        for md in (dmin - 5, dmin, dmin + 30, dmax + 3, -128, 127):
            out.append(Case(f"mindelay-{gname}-{md}", g, (2, 6, 1, 3), min_delay=md))
            out.append(Case(f"mindelay-{gname}-w1412-{md}", g, (1, 4, 1, 2), min_delay=md))
            out.append(Case(f"mindelay1d-{gname}-{md}", g, (2, 6), min_delay=md))
    return out


def overflow_cases():
    g = geom(40, 100)
    return [Case("overflow-2d", g, (2, 6, 1, 3), B=3), Case("overflow-w2814", g, (2, 8, 1, 4), B=3),
            Case("overflow-1d", g, (2, 6), B=3)]


def value_cases():
    out = []
    for kind in ("range", "zero", "holes", "nonfinite"):
        g = geom(60, 140)
        out.append(Case(f"values-{kind}", g, (2, 6, 1, 3), kind=kind, B=2))
        out.append(Case(f"values-{kind}-w2526", g, (2, 5, 2, 6), kind=kind))
        out.append(Case(f"values-{kind}-nl3", g, TILE_NL3, kind=kind))
        out.append(Case(f"values-{kind}-1d", g, (2, 6), kind=kind, B=2))
    return out


PFAS = [10.0 ** -(1.0 + 0.25 * k) for k in range(13)]


def cache_cases():
    g = geom(40, 100)
    return [Case("cache-2d", g, (2, 6, 1, 3), pfa=PFAS[0]), Case("cache-1d", g, (2, 6), pfa=PFAS[0])]


def one_d_cases():
    out = [Case("1d-quirk-0-1", geom(9, 40), (0, 1)), Case("1d-quirk-2-6", geom(9, 40), (2, 6)),
           Case("1d-quirk-pos", geom(9, 40, 1), (1, 3)),
           Case("1d-wide-3-20", geom(5, 15), (3, 20)), Case("1d-wide-2-100", geom(5, 30), (2, 100)),
           Case("1d-wide-0-127", geom(3, 2), (0, 127)), Case("1d-one-column", geom(3, 1), (2, 6)),
           Case("1d-B3", geom(33, 257), (2, 6), B=3)]
    # either side of the longest row cfar1d_dev stages in LDS as fp64 (150 KB: 19 200 delay bins)
    for nC in (19200, 19201):
        out.append(Case(f"1d-lds-{nC}", geom(3, nC, -10, n_corr=16384), (2, 8), pfa=1e-4))
    return out


def all_cases():
    out = []
    for w in WINDOWS:
        out += shape_cases(w)
    out += seg_cases() + grid_cases() + dead_row_cases() + min_delay_cases() + overflow_cases() + value_cases()
    out += cache_cases() + one_d_cases()
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def groups():
    """name -> cases, the unit both test modules parametrise over."""
    g = {"shape-w" + "_".join(map(str, w)): shape_cases(w) for w in WINDOWS}
    g.update({"seg": seg_cases(), "grid": grid_cases(), "dead": dead_row_cases(), "mindelay": min_delay_cases(),
              "overflow": overflow_cases(), "values": value_cases(), "cache": cache_cases(), "1d": one_d_cases()})
    return g
