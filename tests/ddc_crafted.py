"""Crafted taps and streams for the digital down-converter (ddc_kernel / ddc_tail_kernel, csrc/ddc_kernels.hpp).  Helpers
only, no tests; NumPy alone, no GPU and no library is touched at import.

The designed taps of ddc_design fall off towards both ends: with noise under them most taps of a long filter are smaller
than the contract's bound, and exactly the taps a kernel gets wrong -- the first and last of the window, those beside a
segment seam, those that read a tile's lead-in or the carried history -- can be lost without a test noticing.  Here the
taps are GIVEN and of comparable size, h[t] = +-(1 + t / T), or one tap alone, and the streams are

  census A   impulses a period P >= T apart, gcd(P, D) = 1: every output has no term or one, every tap is met;
  census B   h = e_t0 under dense noise: every output is one product, p g[t0] u[m D - t0];
  census C   the comparable taps under dense noise, under the contract of tests/test_ddc_gpu.py.

plan() restates ddc_plan with the kernel's segment bounds; CASES launches each of its seven classes at two (D, T) or more
and with 1, 2, 3 and 8 carriers.  Model is an fp64 restatement of the stream's delivery (calls, rows with a stride, tiles,
tap segments, the history the tail kernel leaves) that equals blah2_amd.ddc and takes a FAULT: the wrong restatements of
the sensitivity proof in tests/test_ddc_crafted_model.py.
"""
import math
from collections import namedtuple

import numpy as np

FS = 65536.0
IRR = FS / (2.0 * math.pi)        # no rational fraction of fs (tests/test_ddc_gpu.py)
IRR2 = -FS * (math.sqrt(2.0) - 1.0) / 3.0
C8 = (0.0, FS / 2, -FS / 2, FS / 3, IRR, IRR2, 1000.0, -FS / 3)
OFFSETS = {1: (IRR,), 2: (IRR2, -FS / 2), 3: (FS / 3, IRR, 0.0), 8: C8}  # block 1; 2; 4 with a padded carrier; 4 twice

LDS_SAMPLES, PART_SAMPLES = 5120, 768  # DDC_LDS_SAMPLES, DDC_PART_SAMPLES
MAX_D, MAX_T = 64, 1024

Plan = namedtuple("Plan", "tile threads TR R G Lp segs")


def plan(D, T):
    """ddc_plan(D, T) restated, with G = threads / TR and the kernel's (s0, s1) of every segment: kernel index s is tap
    T - 1 - s."""
    lead = (T - 1 + D - 1) // D
    fit = LDS_SAMPLES // D - lead - 1
    if fit >= 192:
        tile = 1024 if fit >= 1024 else 512 if fit >= 512 else 256 if fit >= 256 else 192
        while tile > 256 and (T - 1) * 16 <= (tile // 2) * D:
            tile //= 2
        threads = 256 if tile >= 256 else 192
        TR = threads
    else:
        fit = (LDS_SAMPLES - PART_SAMPLES) // D - lead - 1
        tile = 128 if fit >= 128 else 64 if fit >= 64 else fit
        threads = 256
        TR = 128 if tile > 64 else 64
    G = threads // TR
    Tseg = (T + G - 1) // G
    segs = tuple((min(T, k * Tseg), min(T, min(T, k * Tseg) + Tseg)) for k in range(G))
    return Plan(tile, threads, TR, (tile + TR - 1) // TR, G, (tile + lead) | 1, segs)


def plan_class(p):
    """(tile class, threads, TR, R, G): the tiles below 64 are one class, written 0."""
    return (p.tile if p.tile >= 64 else 0, p.threads, p.TR, p.R, p.G)


CLASSES = ((1024, 256, 256, 4, 1), (512, 256, 256, 2, 1), (256, 256, 256, 1, 1), (192, 192, 192, 1, 1), (128, 256, 128, 1, 2),
           (64, 256, 64, 1, 4), (0, 256, 64, 1, 4))

Case = namedtuple("Case", "D T C fmt")
# two (D, T) or more per class, one with T at or near 1024 and one near the class's edge; every class with 1, 2, 3 and 8
# carriers; D odd and D that divide no workgroup size (3, 5, 7, 9, 19, 24, 26, 33, 51, 63); int16 and int8 on segmented classes
CASES = (
    Case(1, 1024, 1, "C32"), Case(3, 1024, 2, "I16"), Case(1, 1024, 3, "I8"), Case(3, 1024, 8, "C32"),      # tile 1024, R = 4
    Case(5, 1024, 8, "I16"), Case(9, 496, 1, "C32"), Case(7, 1000, 2, "I8"), Case(9, 496, 3, "C32"),        # tile 512, R = 2
    Case(9, 1024, 3, "C32"), Case(19, 229, 8, "I16"), Case(9, 1024, 1, "I8"), Case(19, 229, 2, "C32"),      # tile 256
    Case(16, 1024, 2, "C32"), Case(26, 79, 3, "I16"), Case(16, 1024, 8, "I8"), Case(26, 79, 1, "C32"),      # tile 192, 192 threads
    Case(24, 1024, 8, "I16"), Case(33, 67, 1, "I8"), Case(24, 1024, 3, "C32"), Case(33, 67, 2, "C32"),      # tile 128, two segments
    Case(32, 1024, 1, "C32"), Case(64, 193, 8, "I8"), Case(33, 1024, 2, "I16"), Case(64, 193, 3, "C32"),    # tile 64, four segments
    Case(63, 1024, 3, "I16"), Case(64, 512, 2, "C32"), Case(51, 1022, 1, "I8"), Case(64, 1024, 8, "C32"),   # tiles below 64 (51 the least)
)


def case_id(c):
    return f"D{c.D}-T{c.T}-C{c.C}-{c.fmt}"


def class_cases():
    """The first case of the table in each plan class, in CLASSES' order."""
    first = {}
    for c in CASES:
        first.setdefault(plan_class(plan(c.D, c.T)), c)
    return tuple(first[k] for k in CLASSES)


def seam_taps(D, T):
    """The taps on either side of every segment seam of (D, T)'s class: kernel indices s1 - 1 and s1 of each segment but the last."""
    p = plan(D, T)
    out = []
    for s0, s1 in p.segs[:-1]:
        if 0 < s1 < T:
            out += [T - 1 - (s1 - 1), T - 1 - s1]
    return out


def census_b_taps(D, T):
    """t0 of census B: 0, 1, D - 1, D, T - 2, T - 1 and the taps beside every seam (those inside 0 ... T - 1, each once)."""
    return sorted({t for t in [0, 1, D - 1, D, T - 2, T - 1] + seam_taps(D, T) if 0 <= t < T})


def comparable_taps(T, seed=0):
    """h[t] = +-(1 + t / T), the signs from a seeded generator: no tap is small beside another."""
    sign = np.where(np.random.default_rng(1000 + seed).integers(0, 2, T) == 1, 1.0, -1.0)
    return sign * (1.0 + np.arange(T) / float(T))


def unit_tap(T, t0):
    h = np.zeros(T)
    h[t0] = 1.0
    return h


def phasor(f, D, m0, n):
    """exp(-2 pi i frac(r m)), r = f D / fs in fp64, m = m0 ... m0 + n - 1, the product taken exactly (integers)."""
    num, den = (float(f) * D / FS).as_integer_ratio()
    fr = np.array([((num * m) % den) / den for m in range(int(m0), int(m0) + int(n))], dtype=np.float64)
    fr = np.where(fr > 0.5, fr - 1.0, fr)
    return np.cos(2.0 * math.pi * fr) - 1j * np.sin(2.0 * math.pi * fr)


# ---------------------------------------------------------------------------------------------------------------- streams
def _coprime_from(p, D):
    while math.gcd(p, D) != 1:
        p += 1
    return p


def amplitude(ch, k):
    """A Gaussian integer that fits int8, distinct for every impulse k < 120 and channel."""
    return complex(1 + k, 120 - k) if ch == 0 else complex(-(2 + k), k - 100)


Sparse = namedtuple("Sparse", "u n_in rows tap imp amp where")


def sparse(u, D, T, n_in, rows):
    """A stream of impulses T apart or more with what each output is made of: tap[ch][m] / imp[ch][m], the tap and the
    impulse of output m (-1: no term), amp[ch][k] / where[ch][k] the impulses' amplitudes and places."""
    N = u.shape[1]
    tap = -np.ones((2, N // D), dtype=np.int64)
    imp = -np.ones((2, N // D), dtype=np.int64)
    amp, where = [], []
    for ch in range(2):
        at = np.flatnonzero(u[ch])
        assert at.shape[0] < 2 or np.min(np.diff(at)) >= T
        for k, n in enumerate(at):
            m = np.arange(-(-n // D), min(N // D, (n + T - 1) // D + 1))
            tap[ch, m] = m * D - n
            imp[ch, m] = k
        amp.append(u[ch, at])
        where.append(at)
    return Sparse(u, n_in, rows, tap, imp, amp, where)


def census_a(D, T, tile, rows=2):
    """Impulses at k P + off per channel (P >= T, gcd(P, D) = 1, another P and another offset for y), D + 1 of them or more,
    over `rows` rows of one and a half tiles or more."""
    n_min = tile + tile // 2 + 3
    Px = _coprime_from(max(T, rows * n_min * D // (D + 3)), D)  # (a short filter on a large tile: the period grows, not the count)
    P = (Px, _coprime_from(Px + 1, D))
    off = (1, 2)
    n_row = max(-(-((D + 1) * P[1] + off[1] + T) // (rows * D)), n_min)
    N = rows * n_row * D
    u = np.zeros((2, N), dtype=np.complex128)
    for ch in range(2):
        K = (N - off[ch] - 1) // P[ch] + 1
        assert D + 1 <= K <= 120
        u[ch, off[ch] + P[ch] * np.arange(K)] = [amplitude(ch, k) for k in range(K)]
    return sparse(u, D, T, n_row * D, rows)


def expect_single(cen, g, f, D, first=0):
    """Census A's outputs of one carrier with taps g: (v [2][n_out], bound [2][n_out]); an output without a term is exactly
    zero, one with a term p g[t] a within 8 2^-24 |g[t]| |a|."""
    n_out = cen.tap.shape[1]
    p = phasor(f, D, first // D, n_out)
    v = np.zeros((2, n_out), dtype=np.complex128)
    bound = np.zeros((2, n_out))
    g = np.asarray(g).astype(np.complex128)
    for ch in range(2):
        has = cen.tap[ch] >= 0
        term = g[cen.tap[ch][has]] * cen.amp[ch][cen.imp[ch][has]]
        v[ch, has] = p[has] * term
        bound[ch, has] = SINGLE * np.abs(term)
    return v, bound


def expect_one_tap(u, g, t0, f, D, first=0):
    """Census B's outputs of one carrier, h = e_t0 (zeros in front of the stream): (v [2][n_out], bound [2][n_out]), every
    output the one product p[m] g[t0] u[m D - t0]."""
    n_out = u.shape[1] // D
    at = np.arange(n_out) * D - t0
    term = complex(np.asarray(g)[t0]) * np.where(at >= 0, u[:, np.maximum(at, 0)], 0.0)
    return phasor(f, D, first // D, n_out)[None, :] * term, SINGLE * np.abs(term)


SINGLE = 8.0 * 2.0 ** -24  # the single-term bound's factor (derived in tests/test_ddc_crafted_model.py)
CONTRACT = 2.0 ** -24     # ... and the contract's: (3 T + 8) of these times sum_t |g[t]| |u[m D - t]|


def noise(rng, fmt, n, small=False):
    """[2][n] complex128 that the format holds exactly: fp32 normals, int16 at full scale (at most 100 when small, so that a
    full-scale canary stands out), int8 at full scale (at most 8 when small)."""
    if fmt == "C32":
        re, im = rng.standard_normal((2, n)).astype(np.float32), rng.standard_normal((2, n)).astype(np.float32)
        return re.astype(np.float64) + 1j * im.astype(np.float64)
    lim = {"I16": (100, 32767), "I8": (8, 127)}[fmt][0 if small else 1]
    w = rng.integers(-lim - (0 if small else 1), lim + 1, size=(2, 2, n)).astype(np.float64)
    if not small:
        w[:, :, ::7] = lim
        w[:, :, 3::11] = -lim - 1
    return w[0] + 1j * w[1]


def canary(fmt):
    """What an input-stride gap holds: NaN for fp32, full scale for the integer formats."""
    return {"C32": complex(np.nan, np.nan), "I16": complex(32767, -32768), "I8": complex(127, -128)}[fmt]


Call = namedtuple("Call", "buf n_in rows stride")  # buf [2][rows * stride] complex128: the rows, each followed by its gap


def deliver(u, cuts, gap=0, fill=0.0):
    """The stream u [2][N] as calls: cuts = [(n_in, rows), ...] in stream order, rows `n_in + gap` apart, the gaps filled."""
    calls, at = [], 0
    for n_in, rows in cuts:
        buf = np.full((2, rows, n_in + gap), fill, dtype=np.complex128)
        buf[:, :, :n_in] = u[:, at:at + rows * n_in].reshape(2, rows, n_in)
        calls.append(Call(buf.reshape(2, -1), n_in, rows, n_in + gap))
        at += rows * n_in
    assert at == u.shape[1]
    return calls


def encode(fmt, buf):
    """A call's buffer in the format's device layout: (x, y) complex64 planes, (int16 words [n][4], None), (x, y) int8 [n][2]."""
    if fmt == "C32":
        return buf[0].astype(np.complex64), buf[1].astype(np.complex64)
    if fmt == "I16":
        w = np.stack([buf[0].real, buf[0].imag, buf[1].real, buf[1].imag], axis=-1)
        assert np.all(w == np.rint(w)) and np.all(np.abs(w + 0.5) <= 32767.5)
        return w.astype(np.int16), None
    w = [np.stack([b.real, b.imag], axis=-1) for b in buf]
    assert all(np.all(a == np.rint(a)) and np.all(np.abs(a + 0.5) <= 127.5) for a in w)
    return w[0].astype(np.int8), w[1].astype(np.int8)


UNIT = 3  # outputs per row where a history stream is delivered as rows shorter than the history


def history_stream(D, T, a):
    """Call 1 (T - 1 + D samples or more) with one impulse per channel at age a from its end, then zeros for every output
    the impulse still reaches (output j of the zeros reads it under tap j D + 1 + a); both parts whole multiples of UNIT
    outputs.  Returns (the sparse stream, n1, n2), the samples of the two parts."""
    H = T - 1
    n1 = -(-(H + D) // (UNIT * D)) * UNIT * D
    n2 = -(-(H // D + 1) // UNIT) * UNIT * D
    u = np.zeros((2, n1 + n2), dtype=np.complex128)
    u[0, n1 - 1 - a], u[1, n1 - 1 - a] = amplitude(0, 5), amplitude(1, 7)
    return sparse(u, D, T, n1 + n2, 1), n1, n2


def dense_cuts(D, tile):
    """Census B's and C's delivery: two calls of two rows of tile + 5 outputs, an input gap of 13 samples."""
    return [((tile + 5) * D, 2)] * 2, 13


# ------------------------------------------------------------------------------------------------------------------ model
FAULTS = ("drop", "double", "tseg", "wrap", "leadin", "stale", "shift", "overwrite", "stride_walk", "pos_n_in", "swap_xy")


class Model:
    """The stream's delivery in fp64: calls of rows at a stride, tiles of the plan, tap segments, the history and position
    the tail kernel leaves.  Without a fault it equals blah2_amd.ddc on the concatenated stream.  fault = (name, value):
      drop t / double t   tap t left out / counted twice
      tseg                segment length floor(T / G) for ceil: the taps behind G floor(T / G) are nobody's
      wrap +-1            the phase row wraps at D +- 1 (window sample = entry D + row, walked from each segment's start)
      leadin              every tile but the stream's first reads its T - 1 lead-in samples one sample early
      stale               the tail writes entries e < 256 only
      shift               the tail takes the samples one earlier
      overwrite           a call shorter than the history leaves the old entries where they were instead of shifting them
      stride_walk         the walk back over rows divides by in_stride for n_in
      pos_n_in            the position advances by the call's samples, not its outputs
      swap_xy             the tail writes x into y's history and y into x's"""

    def __init__(self, D, g, offsets, first=0, fault=(None, 0)):
        self.g = np.atleast_2d(np.asarray(g)).astype(np.complex128)  # [C][T]
        self.D, self.T, self.H = D, self.g.shape[1], self.g.shape[1] - 1
        self.offsets, self.fault = tuple(offsets), fault
        self.plan = plan(D, self.T)
        self.hist = np.zeros((2, self.H), dtype=np.complex128)
        self.pos, self.first_tile = first // D, True
        T, name, val = self.T, fault[0], fault[1]
        assert name is None or name in FAULTS
        self.coef, self.wmap = np.ones(T), np.arange(T)
        if name == "drop":
            self.coef[T - 1 - val] = 0.0
        if name == "double":
            self.coef[T - 1 - val] = 2.0
        if name == "tseg":
            self.coef[self.plan.G * (T // self.plan.G):] = 0.0
        if name == "wrap":
            for s0, s1 in self.plan.segs:
                ph, q = s0 % D, s0 // D
                for s in range(s0, s1):
                    self.wmap[s] = q * D + ph
                    ph += 1
                    if ph == D + val:
                        ph, q = 0, q + 1

    def _load(self, c, row, i):
        """ddc_load: sample i of row `row` (negative: the rows in front, then the history), both channels."""
        Wd = c.stride if self.fault[0] == "stride_walk" else c.n_in
        out = np.zeros((2, i.shape[0]), dtype=np.complex128)
        pos = i >= 0
        out[:, pos] = c.buf[:, row * c.stride + i[pos]]
        j = row * Wd + i[~pos]
        h = np.zeros((2, j.shape[0]), dtype=np.complex128)
        inh = j < 0
        hi = self.H + j[inh]
        ok = hi >= 0
        hv = np.zeros((2, hi.shape[0]), dtype=np.complex128)
        hv[:, ok] = self.hist[:, hi[ok]]
        h[:, inh] = hv
        jj = j[~inh]
        h[:, ~inh] = c.buf[:, (jj // Wd) * c.stride + jj % Wd]
        out[:, ~pos] = h
        return out

    def call(self, c):
        """One call: (v [C][2][rows n_out], S [C][2][rows n_out]), S = sum_t |g[t]| |u[m D - t]| over the samples read."""
        D, T, H, p = self.D, self.T, self.H, self.plan
        n_out, Cn = c.n_in // D, self.g.shape[0]
        v = np.zeros((Cn, 2, c.rows * n_out), dtype=np.complex128)
        S = np.zeros((Cn, 2, c.rows * n_out))
        grev = self.g[:, ::-1].T  # [T][C]: entry s is g[T - 1 - s]
        for row in range(c.rows):
            for o0 in range(0, n_out, p.tile):
                nT = min(p.tile, n_out - o0)
                W = (nT - 1) * D + T
                i = o0 * D - (T - 1) + np.arange(W)
                if self.fault[0] == "leadin" and not self.first_tile:
                    i[:T - 1] -= 1
                self.first_tile = False
                win = np.zeros((2, W + T + 2 * D), dtype=np.complex128)  # (a wrong wrap walks beyond the window: zeros)
                win[:, :W] = self._load(c, row, i)
                idx = np.minimum(np.arange(nT)[:, None] * D + self.wmap[None, :], win.shape[1] - 1)
                gat = win[:, idx]  # [2][nT][T]
                acc = gat @ (self.coef[:, None] * grev)  # [2][nT][C]
                Sv = np.abs(gat) @ np.abs(grev)
                at = row * n_out + o0
                for k, f in enumerate(self.offsets):
                    ph = phasor(f, D, self.pos + at, nT)
                    v[k, :, at:at + nT] = ph[None, :] * acc[:, :, k]
                    S[k, :, at:at + nT] = Sv[:, :, k]
        # ddc_tail_kernel
        name = self.fault[0]
        total = c.rows * c.n_in
        e = np.arange(H)
        j = total - H + e - (1 if name == "shift" else 0)
        new = np.zeros((2, H), dtype=np.complex128)
        neg = j < 0
        src = (e if name == "overwrite" else H + j)[neg]
        ok = src >= 0
        hv = np.zeros((2, src.shape[0]), dtype=np.complex128)
        hv[:, ok] = self.hist[:, src[ok]]
        new[:, neg] = hv
        jp = j[~neg]
        new[:, ~neg] = c.buf[:, (jp // c.n_in) * c.stride + jp % c.n_in]
        if name == "stale":
            new[:, 256:] = self.hist[:, 256:]
        if name == "swap_xy":
            new = new[::-1].copy()
        self.hist = new
        self.pos += c.rows * (c.n_in if name == "pos_n_in" else n_out)
        return v, S

    def run(self, calls):
        """Every call in turn: (v, S) [C][2][all outputs], and the index of each call's first output."""
        parts = [self.call(c) for c in calls]
        starts = np.cumsum([0] + [pp[0].shape[2] for pp in parts])[:-1]
        return np.concatenate([pp[0] for pp in parts], axis=2), np.concatenate([pp[1] for pp in parts], axis=2), starts
