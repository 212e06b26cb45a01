"""Crafted geometries and inputs for the spectrum analyser (blah2_amd/csrc/spectrum.hip).  Helpers only, no tests; NumPy only, no
device is touched.

The stage keeps nS of the N bins of an N-point transform, spectrum[k] = FFT_N(x[:N])[(k D + N/2 + 1) mod N], and never forms
that transform: it folds the samples over j (x[p + nS j] W_D^(j c)), turns the folded sequence by W_N^(p c), takes an nS-point
DFT and rotates the bins by hq (N/2 + 1 = hq D + c).  Three evaluation paths (roots staged in LDS up to nS = 4096, the same sums
from L2 up to 65536, a chirp-z product beyond), four sample formats, a batch dimension.  ``GEOMS`` puts a row on every size at
which one of these changes its shape; the inputs are integer-valued (exact in every format they are sent in) and say which
term was wrong: an impulse has its spectrum in closed form with every bin's phase naming b_k s mod N, a tone on a kept bin
names the rotation, a tone off the comb is exactly where a wrong (j c) mod D walk leaks.

References, in order of authority: ``definition`` (the sum itself, term by term in long double, the phase reduced in
integers) on up to 64 chosen bins; ``reference`` (oracle.blah2_oracle.spectrum_process: an fp64 FFT) on all bins;
``folded_restatement`` (what the kernels compute, in plain fp64 NumPy, written from the header comment of spectrum.hip), which
sets the floor of the figure and takes planted defects.

Figure: err = max_k |got - ref| / sqrt(mean_k |ref|^2); A N in place of the rms where the expectation is zero (the tone off
the comb).  FLOOR is the worst figure of the restatement against the reference over every input of every row (chirp=True on
the rows the device runs as a chirp-z product), measured on the CPU and asserted by tests/test_spectrum_crafted_model.py;
GATE = 64 FLOOR: the device sums the same fp64 terms in another order (4 waves x nJ chunks, 8 slices, 2 x 18 or 19 radix-2
passes) and forms 2 pi m / nS in fp64 before the cosine -- a constant factor over the restatement's floor, not an order of
magnitude.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import blah2_oracle as O

FOLD_WAVES, DFT_SLICES, DFT_BINS = 4, 8, 32   # spectrum.hip
STAGED_MAX, DIRECT_MAX = 4096, 65536           # largest nS with the roots in LDS / evaluated directly
TAIL = 30000                                   # x[N:n], never read: +-TAIL, not zeros
# Measured: impulses 0.5e-15 .. 3.7e-15 on every row; tones and the noise's tone 1e-14 (nS = 683) .. 2.5e-14 (4096) direct and
# 2.6e-13 .. 3.3e-13 on the chirp-z rows, all of it at the tone's own bin, which stands sqrt(nS) above the rms: eps sqrt(nS).
# The reference itself is 2.5e-13 from the long-double definition there.  test_spectrum_crafted_model.py asserts the figure.
FLOOR = 3.5e-13
GATE = 64 * FLOOR
assert GATE <= 1e-9   # tests/test_spectrum_gpu.py's TOL

Geom = namedtuple("Geom", "name n bw D nS N c hq why")

#        name              n       bw       D     nS      N       c     hq
GEOMS = (
    Geom("one-bin",        1000,   1,       1000, 1,      1000,   501,  0,     "one bin, all of D in the fold"),
    Geom("n7",             7,      7,       1,    7,      7,      0,    4,     "nS < 8 slices, D = 1, c = 0, odd N"),
    Geom("n31",            31,     31,      1,    31,     31,     0,    16,    "one ragged DFT block"),
    Geom("n66",            66,     33,      2,    33,     66,     0,    17,    "32 + 1 bins, D = 2 with c = 0"),
    Geom("n193",           193,    64.4,    2,    96,     192,    1,    48,    "tail of 1 sample, D = 2 with c = 1"),
    Geom("n195",           195,    65,      3,    65,     195,    2,    32,    "64 + 1 lanes, D < FOLD_WAVES, c = 2"),
    Geom("n1285",          1285,   257,     5,    257,    1285,   3,    128,   "256 + 1 reduce threads"),
    Geom("n1293",          1293,   257.5,   5,    258,    1290,   1,    129,   "fractional bandwidth, tail of 3"),
    Geom("n2049",          2049,   600,     3,    683,    2049,   2,    341,   "odd N, p c passes nS"),
    Geom("n10030",         10030,  10,      1003, 10,     10030,  1,    5,     "nJ capped by CUs, ragged j chunks"),
    Geom("n70000",         70000,  33,      2121, 33,     69993,  1061, 16,    "large c, tail of 7"),
    Geom("d16",            48,     3,       16,   3,      48,     9,    1,     "D = 16, nS = 3: nJ = 4 chunks of 4, all full"),
    Geom("empty-chunk",    45012,  9,       5001, 9,      45009,  2501, 4,     "nJ capped below D / 4: the last chunks are empty"),
    Geom("staged-max",     8192,   4096,    2,    4096,   8192,   1,    2048,  "largest staged DFT"),
    Geom("staged-max-d3",  12288,  4096,    3,    4096,   12288,  1,    2048,  "the same with D = 3"),
    Geom("l2-first",       8194,   4097,    2,    4097,   8194,   0,    2049,  "first unstaged"),
    Geom("l2-c3",          20485,  4097,    5,    4097,   20485,  3,    2048,  "unstaged, c = 3"),
    Geom("l2-last",        65536,  65536,   1,    65536,  65536,  0,    32769, "last direct: 4.3e9 fp64 multiply-adds from L2"),
    Geom("cz-first",       65537,  65537,   1,    65537,  65537,  0,    32769, "first chirp-z, M = 262144"),
    Geom("cz-fold",        131074, 65537,   2,    65537,  131074, 0,    32769, "chirp-z behind a real fold"),
    Geom("cz-tail",        140005, 70001,   2,    70002,  140004, 1,    35001, "chirp-z, c = 1, tail of 1, M / 2 < 2 nS - 2"),
    Geom("cz-mid",         100003, 100003,  1,    100003, 100003, 0,    50002, "chirp-z, odd nS between two powers of two"),
    Geom("cz-tight",       131072, 131072,  1,    131072, 131072, 0,    65537, "M = 2 nS exactly"),
    Geom("cz-doubles",     131073, 131073,  1,    131073, 131073, 0,    65537, "M doubles to 524288"),
)
BY_NAME = {g.name: g for g in GEOMS}


def derive(n, bw):
    """(D, nS, N, c, hq) of a constructor call, from the oracle's dims."""
    D, nS, N = O.spectrum_dims(n, bw)
    h = N // 2 + 1
    return D, nS, N, h % D, h // D


def path_of(g):
    return "staged" if g.nS <= STAGED_MAX else "l2" if g.nS <= DIRECT_MAX else "chirpz"


def chirp_len(nS):
    M = 1
    while M < 2 * nS - 1:
        M <<= 1
    return M


def fold_chunks(g, cus):
    """(nJ, per) of spectrum_fold_kernel's grid on a device of ``cus`` compute units: blah2hip_spectrum_create restated."""
    bx = (g.nS + 63) // 64
    nJ = max(1, min((g.D + FOLD_WAVES - 1) // FOLD_WAVES, (4 * cus + bx - 1) // bx))
    return nJ, (g.D + nJ - 1) // nJ


def kept_bin(g, k):
    return (k * g.D + g.N // 2 + 1) % g.N


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _blank(g, tail):
    x = np.zeros(g.n, dtype=np.complex128)
    t = np.arange(g.n - g.N)
    x[g.N:] = tail * (1 - 2 * (t & 1)) + 1j * tail * (1 - 2 * ((t >> 1) & 1))
    return x


def impulse_positions(g):
    return sorted({s for s in (0, 1, g.nS - 1, g.nS, g.N - 1) if 0 <= s < g.N})


def impulse(g, s, A=3000 - 4000j, tail=TAIL):
    """One sample A at index s (s = None: none at all, only the ignored tail is non-zero) and its spectrum in closed form:
    A exp(-2 pi i ((b_k s) mod N) / N), exactly zero for s = None."""
    x = _blank(g, tail)
    if s is None:
        return x, np.zeros(g.nS, dtype=np.complex128)
    x[s] = A
    r = (kept_bin(g, np.arange(g.nS, dtype=np.int64)) * s) % g.N
    return x, A * np.exp(-2j * np.pi * r / g.N)


def tone_bins(g):
    return sorted({k % g.nS for k in (0, g.nS - 1, g.nS - g.hq - 1, g.nS - g.hq)})


def _tone(g, b, amp, tail):
    x = _blank(g, tail)
    r = (b * np.arange(g.N, dtype=np.int64)) % g.N
    t = amp * np.exp(2j * np.pi * r / g.N)
    x[:g.N] = np.rint(t.real) + 1j * np.rint(t.imag)
    return x


def tone_on_bin(g, k, amp=1000, tail=TAIL):
    return _tone(g, kept_bin(g, k), amp, tail)


def off_comb_bin(g):
    assert g.D > 1
    b = ((g.nS // 3) * g.D + g.c + 1) % g.N
    assert b % g.D != g.c
    return b


def tone_off_comb(g, amp=1000, tail=TAIL):
    """A tone on an FFT bin that no kept bin is congruent to modulo D: every kept bin holds rounding crumbs only."""
    return _tone(g, off_comb_bin(g), amp, tail)


def noise_plus_tone(g, seed, amp, tail=TAIL):
    """Uniform integer noise of +-amp/2 on a tone of amp/2 between two bins: |re|, |im| <= amp."""
    rng = np.random.default_rng(seed)
    h = int(amp) // 2
    t = 0.5 * amp * np.exp(2j * np.pi * 0.0613 * np.arange(g.N))
    x = _blank(g, min(tail, amp))
    x[:g.N] = (np.rint(t.real) + rng.integers(-h, h + 1, g.N)) + 1j * (np.rint(t.imag) + rng.integers(-h, h + 1, g.N))
    assert max(np.abs(x.real).max(), np.abs(x.imag).max()) <= amp
    return x


def quarters(g, seed):
    """fp16-exact non-integers: multiples of 0.25 up to 512 (fp16 carries quarter steps below 512), every eighth sample an
    integer up to 2048 (its last exact integer step)."""
    rng = np.random.default_rng(seed)
    v = rng.integers(-2048, 2049, (g.n, 2)) * 0.25
    v[::8] = rng.integers(-2048, 2049, (len(v[::8]), 2))
    return v[:, 0] + 1j * v[:, 1]


Case = namedtuple("Case", "tag x ref zero_ref")   # zero_ref: the expectation is (near) zero, the figure's denominator is A N


def _case(g, tag, x, zero):
    ref = reference(x, g)
    x.setflags(write=False)
    ref.setflags(write=False)
    return Case(tag, x, ref, zero)


@functools.lru_cache(maxsize=None)
def noise_case(name):
    """The ordinary case of a row, full int16 range (kept for the whole session: a few MB on the largest rows)."""
    g = BY_NAME[name]
    return _case(g, "noise", noise_plus_tone(g, 7, 32767), False)


@functools.lru_cache(maxsize=3)
def cases(name):
    """Every C32 input of a row with its reference, computed once; the arrays are read-only.  The noise comes last."""
    g = BY_NAME[name]
    out = []
    for s in impulse_positions(g):
        out.append(_case(g, f"impulse@{s}", impulse(g, s)[0], False))
    if g.n > g.N:
        out.append(_case(g, "impulse@tail", impulse(g, None)[0], True))
    for k in tone_bins(g):
        out.append(_case(g, f"tone@{k}", tone_on_bin(g, k), False))
    if g.D > 1:
        out.append(_case(g, "off-comb", tone_off_comb(g), True))
    out.append(noise_case(name))
    return tuple(out)


# ---- references ---------------------------------------------------------------------------------------------------------------
def reference(x, g):
    return O.spectrum_process(x, g.n, g.bw)[0]


def chosen_bins(g, most=64):
    ks = {0, g.nS - 1, (g.nS - g.hq - 1) % g.nS, (g.nS - g.hq) % g.nS}
    ks.update(int(k) for k in np.linspace(0, g.nS - 1, most - len(ks)).astype(np.int64))
    return sorted(ks)[:most]


def definition(x, g, ks):
    """spectrum[k] = sum_n x[n] exp(-2 pi i ((b_k n) mod N) / N), n < N, in long double; returns complex128."""
    ld = np.longdouble
    pi = 4 * np.arctan(ld(1))
    a = -2 * pi * np.arange(g.N, dtype=np.int64).astype(ld) / ld(g.N)
    wr, wi = np.cos(a), np.sin(a)
    xr, xi = x[:g.N].real.astype(ld), x[:g.N].imag.astype(ld)
    n = np.arange(g.N, dtype=np.int64)
    out = np.empty(len(ks), dtype=np.complex128)
    for i, k in enumerate(ks):
        r = (kept_bin(g, k) * n) % g.N
        c, s = wr[r], wi[r]
        out[i] = complex(float(np.sum(xr * c - xi * s)), float(np.sum(xr * s + xi * c)))
    return out


DEFECTS = ("stride", "walk", "tail", "phase", "rotation", "nowrap", "small-M")


def defect_applies(defect, g, chirp):
    """Whether the term that ``defect`` breaks exists on this row."""
    if defect in ("stride", "walk"):
        return g.D > 1
    if defect == "tail":
        return g.n > g.N
    if defect == "phase":        # some p c reaches nS (and N > nS)
        return g.D > 1 and (g.nS - 1) * g.c >= g.nS
    if defect == "rotation":
        return g.nS > 1
    if defect == "nowrap":
        return chirp and g.nS > 1
    if defect == "small-M":
        # lags +-(nS - 1) hold the same value, so 2 nS - 2 slots are still enough (nS = 65537, 131073); and the chirp of an
        # even nS has period nS, so a transform of exactly nS points is exact too (nS = 131072)
        half = chirp_len(g.nS) // 2
        return chirp and half < 2 * g.nS - 2 and not (g.nS % 2 == 0 and half == g.nS)
    raise ValueError(defect)


def folded_restatement(x, g, chirp=False, defect=None):
    """What spectrum.hip computes, in fp64 (its header comment):
         u[p] = W_N^(p c) sum_j x[p + nS j] W_D^(j c),  Xd = DFT_nS(u),  spectrum[k] = Xd[(k + hq) mod nS];
    chirp: the DFT as ch[m] sum_p (u[p] ch[p]) conj(ch[m - p]), ch[p] = exp(-i pi p^2 / nS), on M = 2^k >= 2 nS - 1 points
    with the conjugate chirp wrapped to M - p.  ``defect`` plants one wrong term (DEFECTS)."""
    assert defect is None or defect in DEFECTS
    D, nS, N, c, hq = g.D, g.nS, g.N, g.c, g.hq
    x = np.asarray(x, dtype=np.complex128)
    p = np.arange(nS, dtype=np.int64)
    rows = D
    if defect == "tail":
        rows = -(-g.n // nS)
        x = np.concatenate([x, np.zeros(rows * nS - len(x))])
    j = np.arange(rows, dtype=np.int64)
    cw = c + 1 if defect == "walk" else c
    wD = np.exp(-2j * np.pi * ((j * cw) % D) / D)
    stride = nS + 1 if defect == "stride" else nS
    idx = p[None, :] + stride * j[:, None]
    if defect == "stride":
        idx %= N
    fold = (x[idx] * wD[:, None]).sum(axis=0)
    ph = (p * c) % (nS if defect == "phase" else N)
    u = fold * np.exp(-2j * np.pi * ph / N)
    if not chirp:
        Xd = np.fft.fft(u)
    else:
        M = chirp_len(nS)
        if defect == "small-M":
            M //= 2
        ch = np.exp(-1j * np.pi * ((p * p) % (2 * nS)) / nS)
        assert M >= nS   # half of a power of two >= 2 nS - 1 still holds the sequence
        a = np.zeros(M, dtype=np.complex128)
        a[:nS] = u * ch
        kb = np.zeros(M, dtype=np.complex128)
        kb[p] = np.conj(ch)
        if defect != "nowrap":
            kb[M - p[1:]] = np.conj(ch[1:])
        conv = np.fft.ifft(np.fft.fft(a) * np.fft.fft(kb))
        Xd = conv[:nS] * ch
    rot = hq + 1 if defect == "rotation" else hq
    return Xd[(p + rot) % nS]


def err(got, ref, denom=None):
    """max_k |got - ref| over the rms of ref (``denom`` where the expectation is zero)."""
    d = np.sqrt(np.mean(np.abs(ref) ** 2)) if denom is None else denom
    return float(np.max(np.abs(got - ref)) / d)


def case_err(got, case, g):
    return err(got, case.ref, 1000.0 * g.N if case.zero_ref else None)
