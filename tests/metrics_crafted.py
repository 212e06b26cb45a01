"""Crafted maps for the Map::set_metrics epilogues fused into the Doppler kernels (csrc/kernels.hpp).  Helpers only, no
tests; no GPU is touched at import.

Every Doppler kernel form carries its own copy of the epilogue: `ok` masks for the rows beyond nD and the columns of a
ragged last tile, wsum[] / wmax[] slots in LDS reused by every tile of a persistent workgroup, a partial slot
``cpi * tilesPerCpi + sub``, a running max that starts at 0, and a finish in metrics_kernel (or metrics_finish_256 behind a
ticket).  The suite's other scenes (oracle.synth_iq with direct = 0.8) put the map's maximum in ONE cell -- the zero-Doppler
cell of lag 0 -- at the same level in every CPI, so maxPower is right as long as that one cell reaches the fold, and a cell
lost or counted twice moves noisePower by 70 dB / cells, under the 1e-3 dB gate.

Here the direct path is off and ONE target is planted per CPI, exactly on a Doppler row and a lag column, at a cell that
moves from CPI to CPI over the places where an epilogue can lose it (``risky_cells``) and at an amplitude that falls by 0.7
per CPI (1.55 dB of 10 log10|z|; the mirrored batch rises).  The planted cell is the map's maximum in every CPI, so
maxPower is the dB value of that one cell: a mask that drops it, or a max carried over from the tile or the CPI before,
shows in maxPower by decibels.  noisePower is then held to ``WRITTEN_DB_GATE`` against ``written_metrics``: the oracle's
Map::set_metrics of the very map the device wrote, so that the transform's rounding is not in the comparison and one cell
of 60 .. 100 dB among 195 .. 53 274 is.

Measured with the oracle over every scene the GPU test runs (tests/test_metrics_crafted_model.py asserts it): the planted
cell is the maximum; on the ladder's top step it stands 19.8 (nD = 65) .. 27.3 dB (nD = 2049) above the mean and 13.6 dB or
more above the second cell; the target's own sidelobes make the floor there, so the margin does not depend on the
amplitude.  Further down the ladder the channel noise (30 against 300 a) makes the floor and each step costs its 1.55 dB:
on the last step (a = 0.5 x 0.7^8 .. 0.7^11) the margins are 14.4 dB and 8.5 dB at nD = 64 and larger at every other
length.
"""
from collections import namedtuple

import numpy as np

from oracle import blah2_oracle as O

# |noisePower - n'| and |maxPower - m'| against written_metrics(returned map), in dB: four times the worst figure measured on
# the MI355X over every case of tests/test_metrics_crafted_gpu.py, 1.22e-5 dB.  It may not exceed WRITTEN_DB_CAP, which is
# ten times under the least any mutant of tests/test_metrics_crafted_model.py has to move a metric.
# FIGURES: measured worst per form, (noisePower, maxPower).  noisePower is 3.7e-6 .. 4.1e-6 dB off in every form alike on
# maps of about 70 dB (2.0e-6 dB on the small-sample maps of about -50 dB): 5e-8 of the level, a third of an fp32 ulp of
# the logarithm.  The NumPy emulation of db_of with a correctly rounded log2 shows 9e-7 dB, so the rest is the device's
# log2f.  maxPower is one fp32 dB value of about 100 (half an ulp: 3.8e-6 dB) less that noisePower; it grows with the level
WRITTEN_DB_CAP = 5e-5
WRITTEN_DB_GATE = 4.9e-5
FIGURES = {"tile8": (4.05e-06, 8.15e-06), "tile8k": (3.95e-06, 8.14e-06), "tile16": (4.05e-06, 8.14e-06),
           "tile16wg": (3.81e-06, 8.15e-06), "sub4": (4.05e-06, 8.14e-06), "pfa513": (3.78e-06, 8.12e-06),
           "tilew": (3.79e-06, 1.22e-05), "tilew2": (3.82e-06, 1.09e-05), "tilew4": (3.79e-06, 1.10e-05),
           "tilem": (3.80e-06, 1.22e-05), "column": (3.81e-06, 1.22e-05), "direct": (3.85e-06, 1.22e-05)}

# What the GPU test needs of the margins: the planted cell stays the one maximum under the map gate (1e-5 of the peak: any
# margin above 1e-4 dB does), and a planted cell lost from the fold moves maxPower by the margin above the second cell, which
# has to be thousands of gates.  The floors asked of every CPI of every scene are a factor of four in |z| above the second
# cell and of sixteen above the mean; the top step is held to the figures above, rounded down
MARGIN_MEAN_DB = 12.0     # the planted cell above the mean of the dB values, every CPI of every scene
MARGIN_SECOND_DB = 6.0    # ... and above the second-largest cell
TOP_MARGIN_MEAN_DB = 19.5    # the same on the ladder's top step (a = 0.5)
TOP_MARGIN_SECOND_DB = 13.5
SMALL = 1e-6              # the small-sample scenes: x and y scaled by this, every cell of the map below 0 dB

WINDOWS = {"w25": (-7, 17), "w26": (-7, 18), "w3": (-1, 1)}
Geom = namedtuple("Geom", "nD window explicit")


def geom(nD, window="w25"):
    """nD = 64 is the explicit (even) bin count; every other length follows the reference's rule from fMax = nD // 2."""
    return Geom(nD, window, nD % 2 == 0)


def args_of(g):
    """Constructor arguments (delayMin, delayMax, dopplerMin, dopplerMax, fs, n): fs = n = 200 nD, a 1 s CPI of nD pulses
    of 200 samples, 1 Hz per Doppler row."""
    dmin, dmax = WINDOWS[g.window]
    n = 200 * g.nD
    return (dmin, dmax, -(g.nD // 2), g.nD // 2, n, n)


def dims_of(g):
    d = O.ambiguity_dims(*args_of(g), True, n_doppler_bins=g.nD if g.explicit else 0)
    assert (d.n_doppler_bins, d.n_corr) == (g.nD, 200)
    return d


def risky_cells(nD, nDelay, count=0):
    """(row, column) per CPI: two lists paired cyclically, as many CPIs as the longer list (or ``count``), so that every
    value occurs.  Rows: both ends, both sides of the 64-row register seams at either end, the zero-Doppler row nD // 2
    (where the kernels add nD r0 back) and its neighbours.  Columns: lag 0 of the -7 .. window (column 7), both sides of the
    4-, 8- and 16-column tile seams, the ragged tile's last live columns.

    The rows go from zero Doppler outwards.  A target at f Hz turns by f / nD of a cycle within a pulse of 200 samples, which
    costs its peak up to 1.96 dB of 10 log10|z| at the band's edge (sinc(1/2)), more than one step of the ladder; in this
    order the loss grows along the batch as the amplitude falls, so the peaks descend CPI by CPI until the row list wraps."""
    rows = sorted({min(max(v, 0), nD - 1) for v in (0, 1, 63, 64, nD // 2 - 1, nD // 2, nD // 2 + 1, nD - 65, nD - 64, nD - 2, nD - 1)},
                  key=lambda r: (abs(r - (nD - 1) // 2), r))
    cols = sorted({min(max(v, 0), nDelay - 1) for v in (0, 3, 4, 7, 8, 15, 16, nDelay - 2, nDelay - 1)})
    B = max(len(rows), len(cols), count)
    return [(rows[c % len(rows)], cols[c % len(cols)]) for c in range(B)]


def ladder(B, order="down"):
    a = [0.5 * 0.7 ** c for c in range(B)]
    return a if order == "down" else a[::-1]


def scene(g, cells, amps, seed, col_shift=0):
    """Per-CPI (x, y) complex128, int16-valued: CPI c is oracle.synth_iq(seed + c) with no direct path and one target of
    amplitude amps[c] at the lag of column cells[c][1] and the Doppler of row cells[c][0], both read off the oracle's axes.
    x depends on the seed alone, so two scenes of one seed are two surveillance channels of one reference."""
    d = dims_of(g)
    out = []
    for c, (r, k) in enumerate(cells):
        k = (k + col_shift) % d.n_delay_bins
        out.append(O.synth_iq(d.n_samples, seed + c, fs=d.fs, direct=0.0, quantise=True,
                              targets=((int(d.delay[k]), float(d.doppler[r]), float(amps[c])),)))
    return out


def db_values(m):
    """10 log10|z| in fp64, cell by cell (Map.cpp:187-206)."""
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(np.abs(np.asarray(m, dtype=np.complex128)))


def written_metrics(map_c64):
    """oracle.map_metrics of the map the device returned."""
    with np.errstate(divide="ignore"):
        return O.map_metrics(np.asarray(map_c64).astype(np.complex128))


def db_of_emulated(map_c64):
    """csrc/kernels.hpp db_of on complex64 cells: fp32 re^2 + im^2, fp32 log2, fp32 product with 5 log10(2); the sum of the
    values in fp64.  Returns (noisePower, maxPower)."""
    z = np.asarray(map_c64, dtype=np.complex64)
    re, im = z.real.astype(np.float32), z.imag.astype(np.float32)
    with np.errstate(divide="ignore"):
        db = np.float32(1.50514997831990597607) * np.log2(re * re + im * im, dtype=np.float32)
    assert db.dtype == np.float32
    noise = float(np.sum(db.astype(np.float64)) / db.size)
    return noise, float(max(np.float32(0.0), db.max())) - noise


# ---- mutants: wrong epilogues on the fp64 dB values, the divisor left at nD nDelay as the kernels have it -----------------
MUTANTS = ("dropped", "twice", "padding", "max-inf", "max-carried", "last-tile-stale")
TILE_WIDTHS = (4, 8, 16)


def _finish(total, peak, cells, floor=0.0):
    noise = total / cells
    return noise, max(floor, peak) - noise


def mutant(which, db, cell, db_prev=None, width=16):
    """(noisePower, maxPower) of a wrong epilogue.  ``db``: this CPI's dB values [nD, nDelay]; ``cell``: the planted cell;
    ``db_prev``: the CPI before; ``width``: the tile's columns.

    dropped          the planted cell masked out of sum and max       twice    ... counted twice
    padding          one padding column of the ragged last tile let into the sum: a copy of the previous tile's same column
                     (of this tile's, wrapped, where the window has fewer columns than a tile)
    max-inf          the running max started at -inf                  max-carried   the max of CPI c - 1 kept for CPI c
    last-tile-stale  the last tile's partial (sum, max) taken from the CPI before
    """
    nD, nC = db.shape
    total, peak = float(db.sum()), float(db.max())
    start = width * ((nC - 1) // width)  # first column of the last tile
    if which == "dropped":
        rest = db.copy()
        rest[cell] = -np.inf
        return _finish(total - db[cell], float(rest.max()), db.size)
    if which == "twice":
        return _finish(total + db[cell], peak, db.size)
    if which == "padding":
        live = nC - start
        assert live < width, "no ragged tile"
        src = start - width + live if start else live % nC
        return _finish(total + float(db[:, src].sum()), peak, db.size)
    if which == "max-inf":
        return _finish(total, peak, db.size, floor=-np.inf)
    if which == "max-carried":
        return _finish(total, max(peak, float(db_prev.max())), db.size)
    if which == "last-tile-stale":
        own = float(db[:, :start].max()) if start else -np.inf
        return _finish(total - float(db[:, start:].sum()) + float(db_prev[:, start:].sum()),
                       max(own, float(db_prev[:, start:].max())), db.size)
    raise ValueError(which)


# ---- the forms and the cases both test files run --------------------------------------------------------------------------
PERSISTENT = ("tile8", "tile8k", "tile16", "tile16wg", "pfa513", "tilew", "tilew2", "tilew4")
SMALL_ND = ("tile8", "tile8k", "tile16", "tile16wg", "sub4", "column", "direct")
FORMS = {65: SMALL_ND, 513: SMALL_ND + ("pfa513",), 64: ("tile8", "tile16", "sub4"),
         515: ("tilew", "tilem", "column", "direct"), 1025: ("tilew", "tilem", "column", "direct"),
         1027: ("tilew2", "tilew4", "tilem", "column", "direct"), 2049: ("tilew2", "tilew4", "tilem", "column", "direct")}
GRID_OF = {"w25": 3, "w26": 5, "w3": 3}  # workgroups of a persistent form: every one walks three tiles or more
SEED0 = 4100


def batch_size(nD):
    """CPIs of a batch: what risky_cells pairs (9 at nD = 64 / 65, 11 from 513 on), and 12 from nD = 1027 on, where
    doppler_tilew2_kernel's grid of 32 quarter-tile workgroups needs 96 quarter tiles for three each."""
    return 12 if nD > 1025 else 0


Case = namedtuple("Case", "kind form nD window grid order")


def case_id(c):
    return f"{c.kind}-{c.form}-{c.nD}-{c.window}" + (f"-g{c.grid}" if c.grid else "") + ("-up" if c.order == "up" else "")


def _grid(form, window):
    return GRID_OF[window] if form in PERSISTENT else 0


# 1. the descending ladder: every form at every Doppler length of its table row, the three windows
DESCENDING = tuple(Case("down", f, nD, w, _grid(f, w), "down") for nD in FORMS for f in FORMS[nD] for w in WINDOWS) + (
    Case("down", "pfa513", 513, "w25", 8, "down"),)  # eight workgroups: one per XCD of the XCD-local tile walk
# 2. the ascending ladder, 25 columns, one Doppler length per form (both instantiations of tilem, all three of column)
ASCENDING = tuple(Case("up", f, nD, "w25", _grid(f, "w25"), "up") for f, nD in (
    ("tile8", 65), ("tile8k", 513), ("tile16", 513), ("tile16wg", 65), ("sub4", 513), ("pfa513", 513), ("column", 65), ("direct", 513),
    ("tilew", 515), ("tilem", 1025), ("column", 1025), ("tilew2", 1027), ("tilew4", 2049), ("tilem", 2049), ("column", 2049), ("direct", 1027)))
# 3. / 4. small samples and the all-zero CPI: every form, one Doppler length per class
ONE_PER_CLASS = (64, 513, 1025, 2049)
SMALL_CASES = tuple(Case("small", f, nD, "w25", _grid(f, "w25"), "down") for nD in ONE_PER_CLASS for f in FORMS[nD])
ZERO_CASES = tuple(Case("zero", f, nD, "w25", _grid(f, "w25"), "down") for nD in ONE_PER_CLASS for f in FORMS[nD])
# 7. hot columns and leak compensation "always": one case per class
FEATURE_CASES = (Case("features", "tile8", 64, "w25", 3, "down"), Case("features", "pfa513", 513, "w25", 3, "down"),
                 Case("features", "tilew", 1025, "w25", 3, "down"), Case("features", "tilew2", 2049, "w25", 3, "down"))

_batches = {}


def batch(g, order="down", small=False, zero_cpi=None, channel=0, B=None):
    """{'d', 'cells', 'amps', 'xs', 'ys', 'refs'} of one batch: computed once, left unchanged.  ``small``: x and y scaled by
    SMALL and rounded to fp32, the oracle fed the rounded values.  ``zero_cpi``: that CPI's y is all zero, its map too.
    ``channel`` 1: a second surveillance channel on the same x, the cells' columns shifted by 5 and the batch mirrored."""
    key = (g, order, small, zero_cpi, channel, B)
    if key in _batches:
        return _batches[key]
    d = dims_of(g)
    cells = risky_cells(g.nD, d.n_delay_bins, batch_size(g.nD))
    if B is not None:
        cells = cells[:B]
    if channel:
        order = "up" if order == "down" else "down"
    amps = ladder(len(cells), order)
    if order == "up":  # the mirror: the same (cell, amplitude) pairs in the opposite order
        cells = cells[::-1]
    xy = scene(g, cells, amps, SEED0 + 100 * list(WINDOWS).index(g.window), col_shift=5 * channel)
    if channel:
        cells = [(r, (k + 5) % d.n_delay_bins) for r, k in cells]
    xs, ys = [v[0] for v in xy], [v[1] for v in xy]
    if small:
        xs = [(v * SMALL).astype(np.complex64).astype(np.complex128) for v in xs]
        ys = [(v * SMALL).astype(np.complex64).astype(np.complex128) for v in ys]
    if zero_cpi is not None:
        ys[zero_cpi] = np.zeros_like(ys[zero_cpi])
    refs = [np.zeros((d.n_doppler_bins, d.n_delay_bins), dtype=np.complex128) if c == zero_cpi
            else O.ambiguity_process(d, xs[c], ys[c]) for c in range(len(cells))]
    _batches[key] = {"d": d, "cells": cells, "amps": amps, "xs": xs, "ys": ys, "refs": refs}
    return _batches[key]


def batch_of(case):
    g = geom(case.nD, case.window)
    if case.kind == "small":
        return batch(g, small=True)
    if case.kind == "zero":
        return batch(g, zero_cpi=zero_cpi_of(g))
    return batch(g, case.order)


def zero_cpi_of(g):
    return len(risky_cells(g.nD, dims_of(g).n_delay_bins, batch_size(g.nD))) // 2


def scene_keys():
    """The (geometry, order, small) of every ordinary batch the GPU test hands to the device, for the model test."""
    keys = []
    for c in DESCENDING + ASCENDING + SMALL_CASES + FEATURE_CASES:
        k = (geom(c.nD, c.window), c.order, c.kind == "small")
        if k not in keys:
            keys.append(k)
    for nD in (513, 1027):  # the second channel of the multi-channel case
        keys.append((geom(nD), "down", False, 1))
    return keys
