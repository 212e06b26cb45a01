"""Crafted pulses for the range kernels (helpers only, no tests): a sparse "pair census" instead of a noise-like scene.

A census CPI is zero except for impulses planted in pairs: a reference sample x[i * nCorr + a] and, for every lag of a set of
delay columns, a surveillance sample y[i * nCorr + a + lag].  The positions a sit at the pulse's two ends and on both sides
of every segment seam of the plan, the columns at the seams of the range map (the 16-column tile, the 7-of-16-outputs form
at 448 lags, the window's two ends, lags -1, 0, +1).  Pairs whose surveillance sample falls into the neighbouring pulse are
planted too: they must count for nothing.  A sample lost, added or moved at such a place changes a cell of the map by a
planted product, tens of percent of the peak, where a noise-like scene moves it by about 1 / sqrt(nCorr) of itself.

The amplitudes are Gaussian integers with components in -7 .. 7 and modulus at least 3: exact as int8, int16, fp16 and
fp32, so one fp64 reference (oracle.blah2_oracle.ambiguity_process) serves every sample format.
"""
from collections import namedtuple

import numpy as np

from oracle import blah2_oracle as O

# longest run of lags one range launch takes on the 4096-point transform when the window needs more than one
# (blah2_amd/csrc/capi.hip, blah2hip_amb_create_ex: `lag_chunks(h, 2048)`); tests/test_range_crafted_model.py reads it back
LAG_CHUNK_CAP = 2048
TAIL = 4             # samples of every geometry behind nD * nCorr, never read by the range stage
GAP = 37             # samples between the CPIs of a plane
GAP_VALUE = 77       # what a read beyond a CPI would pick up
TAIL_X, TAIL_Y = 5 - 6j, -4 + 7j

Geom = namedtuple("Geom", "name fft_len delay_min delay_max n_corr n_seg seg_len pins")

# fs = n and Doppler limits -2 .. 2: nD = 5, n = 5 nCorr + 4.  (n_seg, seg_len) is what the engine's planner gives at the
# forced transform length; window = seg_len + nDelay - 1 samples of y' per segment.
GEOMS = (
    Geom("1k-449x1728", 1024, -10, 438, 1728, 3, 576, "REUSE without OUT7, window 1024 = the whole transform"),
    Geom("1k-449x1729", 1024, -10, 438, 1729, 4, 576, "carried registers into a one-sample last segment"),
    Geom("1k-449-positive", 1024, 1, 449, 1728, 3, 576, "one-sided window of positive lags at that shape"),
    Geom("1k-449-negative", 1024, -449, -1, 1728, 3, 576, "one-sided window of negative lags at that shape"),
    Geom("1k-448x1728", 1024, -10, 437, 1728, 3, 576, "REUSE with OUT7 at its limit, window 1023"),
    Geom("1k-448x1154", 1024, -10, 437, 1154, 2, 577, "first segment length outside SHORTX, window 1024"),
    Geom("1k-450x1725", 1024, -10, 439, 1725, 3, 575, "just outside REUSE, window 1024"),
    Geom("2k-257x3072", 2048, -6, 250, 3072, 2, 1536, "shortw with all three limits met, window 1792"),
    Geom("2k-258x3072", 2048, -6, 251, 3072, 2, 1536, "one past shortw, window 1793"),
    Geom("2k-411x3276", 2048, -10, 400, 3276, 2, 1638, "window 2048 = the whole transform, OUT7"),
    Geom("2k-449x3200", 2048, -10, 438, 3200, 2, 1600, "window 2048 = the whole transform, all 16 outputs"),
    Geom("4k-2049x4096", 4096, -24, 2024, 4096, 2, 2048, "half-zero x segments at their limit, window 4096"),
    Geom("4k-2050x4094", 4096, -24, 2025, 4094, 2, 2047, "one past it, window 4096"),
)
FIRST_ROW = {1024: "1k-449x1728", 2048: "2k-257x3072", 4096: "4k-2049x4096"}  # the rows that run all six formats
# tests/test_multi_surv_gpu.py's CHUNKS window (4431 delay bins, three launches) at nD = 5.  nCorr = 4500 (n = 22 504, the one
# CPI above the table's 20 484 samples): a window that reaches lag 4400 is one run of linear lags only while
# nfft - nCorr >= 4400, i.e. from nCorr = 4401 on.
CHUNKED = Geom("4k-chunks-4431x4500", 4096, -30, 4400, 4500, 3, 1500, "three lag chunks of at most 2048 lags")
GEOM_BY_NAME = {g.name: g for g in GEOMS + (CHUNKED,)}


def args_of(g):
    """Constructor arguments (delayMin, delayMax, dopplerMin, dopplerMax, fs, n) of a table row."""
    n = 5 * g.n_corr + TAIL
    return (g.delay_min, g.delay_max, -2, 2, n, n)


def dims_of(g):
    return O.ambiguity_dims(*args_of(g), True)


def chunk_seams(n_delay, cap=LAG_CHUNK_CAP):
    """First columns of the second and later chunks of a one-run window of ``n_delay`` lags (capi.hip lag_chunks)."""
    return list(range(cap, n_delay, cap)) if n_delay > 4081 else []


def extra_cols_of(g):
    """Census columns on both sides of each chunk seam."""
    n_delay = g.delay_max - g.delay_min + 1
    return [s + k for s in chunk_seams(n_delay) for k in (-2, -1, 0, 1)]


def plan(n_corr, n_delay, F):
    """(nSeg, segLen) of capi.hip's choose_plan at the forced transform length ``F`` for a longest chunk of ``n_delay``
    lags, or None where the window does not fit."""
    lmax = F - n_delay + 1
    if lmax < 16:
        return None
    n_seg = -(-n_corr // lmax)
    seg_len = -(-n_corr // n_seg)
    if F == 1024 and lmax >= 576 and -(-n_corr // 576) == n_seg:
        seg_len = 576
    return n_seg, seg_len


def plan_of(g):
    n_delay = g.delay_max - g.delay_min + 1
    return plan(g.n_corr, min(n_delay, LAG_CHUNK_CAP) if n_delay > 4081 else n_delay, g.fft_len)


def gaussian_integers(rng, count):
    """``count`` values a + bj, a, b in -7 .. 7, |a + bj| >= 3."""
    out = np.zeros(count, dtype=np.complex128)
    todo = np.arange(count)
    while todo.size:
        v = rng.integers(-7, 8, todo.size) + 1j * rng.integers(-7, 8, todo.size)
        good = np.abs(v) >= 3
        out[todo[good]] = v[good]
        todo = todo[~good]
    return out


def census_positions(n_corr, n_seg, seg_len):
    a = {0, 1, n_corr - 2, n_corr - 1}
    for s in range(1, n_seg):
        a |= {s * seg_len - 1, s * seg_len, s * seg_len + 1}
    return sorted(p for p in a if 0 <= p < n_corr)


def census_columns(delay_min, n_delay, extra=()):
    c = {0, 1, 15, 16, 17, 447, 448, 449, n_delay - 2, n_delay - 1, -1 - delay_min, -delay_min, 1 - delay_min}
    c |= set(int(e) for e in extra)
    return sorted(k for k in c if 0 <= k < n_delay)


def census(dims, n_seg, seg_len, seed, pulses=None, extra_cols=()):
    """(x, y): complex128 arrays of ``dims.n_samples``, zero except for the planted impulses and the tail behind
    nD * nCorr.  ``pulses``: the pulses that carry impulses ({0, 1, nD // 2, nD - 1} unless given; 0 and 1 are adjacent on
    purpose).  The window must be one run of linear lags (lag of column c = delayMin + c)."""
    nD, nC, n = dims.n_doppler_bins, dims.n_corr, dims.n_samples
    assert dims.nfft - nC >= max(abs(dims.delay_min), abs(dims.delay_max)), "the lag window aliases: not one run of linear lags"
    if pulses is None:
        pulses = sorted({0, 1, nD // 2, nD - 1})
    pos = np.array(census_positions(nC, n_seg, seg_len), dtype=np.int64)
    lags = dims.delay_min + np.array(census_columns(dims.delay_min, dims.n_delay_bins, extra_cols), dtype=np.int64)
    base = np.array(sorted(pulses), dtype=np.int64)[:, None] * nC + pos[None, :]
    ix = np.unique(base.ravel())
    iy = np.unique((base[:, :, None] + lags[None, None, :]).ravel())  # into the neighbouring pulses too
    iy = iy[(iy >= 0) & (iy < nD * nC)]
    rng = np.random.default_rng(seed)
    x = np.zeros(n, dtype=np.complex128)
    y = np.zeros(n, dtype=np.complex128)
    x[ix] = gaussian_integers(rng, ix.size)
    y[iy] = gaussian_integers(rng, iy.size)
    x[nD * nC:] = TAIL_X
    y[nD * nC:] = TAIL_Y
    return x, y


def smallest_product(dims, x, y):
    """Smallest |u v| over the planted reference samples u and surveillance samples v."""
    used = dims.n_doppler_bins * dims.n_corr
    ax, ay = np.abs(x[:used]), np.abs(y[:used])
    return float(ax[ax > 0].min() * ay[ay > 0].min())


def reference(dims, x, y):
    return O.ambiguity_process(dims, x, y)


# ---- planes in the six sample formats ---------------------------------------------------------------------------------
FORMATS = ("FMT_C32", "FMT_I8", "FMT_I16", "FMT_F16", "FMT_I16X_C32Y", "FMT_I8X_C32Y")


def _pairs(v):
    return np.stack([v.real, v.imag], axis=-1)


def _c32_plane(cpis, stride):
    host = np.full((len(cpis), stride), GAP_VALUE * (1 + 1j), dtype=np.complex64)
    for c, v in enumerate(cpis):
        host[c, :v.shape[0]] = v
    return host


def _pair_plane(cpis, stride, dtype):
    host = np.full((len(cpis), stride, 2), GAP_VALUE, dtype=dtype)
    for c, v in enumerate(cpis):
        host[c, :v.shape[0]] = _pairs(v)
    return host


def _word_plane(xs, ys, stride):
    """The int16 I1 Q1 I2 Q2 words; ``ys`` None: the second tuner's columns hold the gap value (a mixed format must not
    read them)."""
    host = np.full((len(xs), stride, 4), GAP_VALUE, dtype=np.int16)
    for c, v in enumerate(xs):
        host[c, :v.shape[0], 0:2] = _pairs(v)
        if ys is not None:
            host[c, :v.shape[0], 2:4] = _pairs(ys[c])
    return host


def host_planes(fmt_name, xs, ys, stride):
    """(x plane, y plane or None) as NumPy arrays for ``process_dev(fmt, ...)``: one row of ``stride`` samples per CPI, the
    gaps between and behind the CPIs filled with GAP_VALUE.  ``xs``, ``ys``: lists of complex128 CPIs with census values."""
    for v in list(xs) + list(ys):
        assert np.abs(_pairs(v)).max() <= 127 and np.array_equal(_pairs(v), np.rint(_pairs(v)))
    if fmt_name == "FMT_C32":
        return _c32_plane(xs, stride), _c32_plane(ys, stride)
    if fmt_name == "FMT_I8":
        return _pair_plane(xs, stride, np.int8), _pair_plane(ys, stride, np.int8)
    if fmt_name == "FMT_F16":
        return _pair_plane(xs, stride, np.float16), _pair_plane(ys, stride, np.float16)
    if fmt_name == "FMT_I16":
        return _word_plane(xs, ys, stride), None
    if fmt_name == "FMT_I16X_C32Y":
        return _word_plane(xs, None, stride), _c32_plane(ys, stride)
    if fmt_name == "FMT_I8X_C32Y":
        return _pair_plane(xs, stride, np.int8), _c32_plane(ys, stride)
    raise ValueError(fmt_name)


# ---- three deliberately wrong restatements of the correlation (fp64, for the sensitivity proof) -----------------------
def _doppler(dims, R):
    nD = dims.n_doppler_bins
    D = np.fft.fft(R, axis=0)
    return D[(np.arange(nD) + nD // 2 + 1) % nD, :]


def correlate(dims, x, y, n_seg, seg_len, mutant=None):
    """The map by the time-domain definition, segment by segment as the kernels walk a pulse, over the populated reference
    samples only.  ``mutant``: None (right), "leak" (y read across pulse boundaries), "first" (the pulse's first y sample
    read as zero) or "segend" (the last x sample of each segment dropped)."""
    nD, nC, nDelay = dims.n_doppler_bins, dims.n_corr, dims.n_delay_bins
    lags = dims.delay_min + np.arange(nDelay)
    R = np.zeros((nD, nDelay), dtype=np.complex128)
    used = nD * nC
    for i in range(nD):
        xs, lo = x[i * nC:(i + 1) * nC], i * nC
        for s in range(n_seg):
            a0, a1 = s * seg_len, min((s + 1) * seg_len, nC)
            if mutant == "segend":
                a1 -= 1
            for a in range(a0, a1):
                if xs[a] == 0:
                    continue
                m = a + lags
                if mutant == "leak":
                    ok = (lo + m >= 0) & (lo + m < used)
                else:
                    ok = (m >= 0) & (m < nC)
                if mutant == "first":
                    ok &= m != 0
                R[i, ok] += y[lo + m[ok]] * np.conj(xs[a])
    return _doppler(dims, R)
