"""Crafted taps and pulses for the fused FIR range kernel (range_fir_kernel, csrc/kernels.hpp).  Helpers only, no tests; no
GPU is touched at import, torch is imported inside the functions that need it.

The fused kernel filters the surveillance channel with given taps, y' = y - (w * xs), and correlates y' with x pulse by
pulse.  Estimated taps have ONE strong tap (lag 0) and noise-sized others, so a scene filtered with them cannot tell whether
the kernel's edge products -- the taps that look past a pulse's end (`tail`), the CPI's first |delayMin| samples that the
filter's stream does not hold (`head`), the history block in front of a pulse, the largest tap on its own path (`k0`) -- are
right.  Here the taps are GIVEN: a dozen Gaussian dyadics (multiples of 1/8) of modulus 0.375 .. 1 per CPI, exact in fp32 and
in fp64, with the largest wherever a test wants it; and the channels are a sparse census as in tests/range_crafted.py:
Gaussian-integer impulses at the places where those products arise, so that one product lost, added or misplaced moves a
cell of the map by parts in a hundred of the peak.

The reference is the oracle's own chain in fp64: the filter of oracle.blah2_oracle.wiener_hopf (its lines ":125-160", a
linear convolution with the shifted reference xs[i] = x[(i - delayMin) mod N], xs[m < 0] = 0) with the taps given instead of
solved for, then oracle.blah2_oracle.ambiguity_process.
"""
from collections import namedtuple

import numpy as np

import range_crafted as RC
from oracle import blah2_oracle as O

L = 2048          # samples of a filter block / a correlation segment of the kernel (half its 4096-point transform)
IN_GAP = 5        # input stride n + 5 (tests/clutter_crafted.py)
PAD = 64          # samples of poison in front of and behind a plane
POISON = 600 + 800j  # modulus 1000, fits int16: what a read beyond a CPI's N samples would pick up
SPARE_Y = -4 + 7j  # y behind nD nCorr: never read

Geom = namedtuple("Geom", "name delay_min delay_max f_max n_corr spare sb pins")

# fs = n: nD = 2 fMax + 1 pulses of nCorr = n // nD samples, n = nD nCorr + spare with |delayMin| <= spare < nD
GEOMS = (
    Geom("min-pulse", -8, 300, 10, 2056, 8, 2, "nCorr = 2048 - delayMin, the shortest accepted; spare exactly |delayMin|"),
    Geom("on-boundary", -8, 300, 10, 4096, 8, 3, "pulse ends on a block boundary; a third block of 8 samples"),
    Geom("past-5", -8, 300, 10, 4101, 8, 3, "pulse ends 5 samples past a boundary"),
    Geom("short-5", -8, 300, 10, 4091, 8, 3, "pulse ends 5 samples short of a boundary: two blocks hold its last 8 samples"),
    Geom("block-fits-4104", -8, 300, 10, 4104, 8, 3, "16 samples of the pulse in the third block"),
    Geom("block-fits-4088", -8, 300, 10, 4088, 8, 2, "nCorr - delayMin = 4096: the second block ends with the pulse, SB drops to 2"),
    Geom("long-walk", -8, 300, 10, 9523, 8, 5, "five blocks"),
    Geom("dmin0", 0, 2048, 5, 10000, 3, 5, "no anticipation; 2048 taps, 2049 delay bins"),
    Geom("dmin1", -1, 40, 2, 2049, 1, 2, "one anticipatory tap; nD = 5"),
    Geom("head-block1", -24, 2023, 15, 6149, 30, 4, "2047 taps: `head` reaches block 1 of pulse 0; 6 spare samples the filter never reads"),
    Geom("wide-dmin", -260, 100, 131, 2400, 260, 2, "`tail` span crosses a 256-lane register row; 263 pulses"),
)
GEOM_BY_NAME = {g.name: g for g in GEOMS}


def args_of(g):
    """Constructor arguments (delayMin, delayMax, dopplerMin, dopplerMax, fs, n) of a table row."""
    n = (2 * g.f_max + 1) * g.n_corr + g.spare
    return (g.delay_min, g.delay_max, -g.f_max, g.f_max, n, n)


def dims_of(g):
    return O.ambiguity_dims(*args_of(g), True)


def default_bins(g):
    """The clutter filter's length for the map's window: nDelay - 1 (WienerHopf.cpp:12)."""
    return g.delay_max - g.delay_min


def unfusable(dims, n_bins, fir_dmin):
    """capi.hip fir_unfusable()'s geometry conditions restated (the format and transform-length ones left out): None, or
    the condition that refuses."""
    A = -dims.delay_min
    if dims.doppler_min + dims.doppler_max != 0:
        return "symmetric Doppler limits"
    if n_bins < 1 or n_bins > L + 1 or dims.n_delay_bins > L + 1:
        return "at most 2049 taps and 2049 delay bins"
    if fir_dmin != dims.delay_min or dims.delay_min > 0:
        return "first lag"
    if n_bins < A:
        return "reach lag 0"
    if dims.n_corr < L + A:
        return "shorter"
    if dims.n_doppler_bins * dims.n_corr + A > dims.n_samples:
        return "look-ahead"
    return None


# ---- taps ---------------------------------------------------------------------------------------------------------------
def antic_indices(A):
    """Anticipatory tap indices (lags delayMin .. -1) that carry a tap: all of them up to 8, else both ends, the middle and
    the indices on both sides of a 256-lane register row."""
    if A <= 8:
        return list(range(A))
    return sorted({0, 1, A // 2, A - 2, A - 1} | {k for k in (255, 256) if k < A})


def late_indices(A, nb):
    """Tap indices from lag 0 on that carry a tap: lags 0 and 1, the window's last two, both sides of the register rows at
    256 and 2048, and (2047 taps at delayMin = -24) taps 2026 and 2040, which reach x[0 .. 24) from block 1 of pulse 0."""
    c = {A, A + 1, nb - 2, nb - 1, 255, 256, 2047, 2048}
    if nb > 2040:
        c |= {2026, 2040}
    return sorted(k for k in c if A <= k < nb)


def _small(rng, count):
    """Multiples of 1/8 with modulus in [0.375, 0.75]."""
    out = np.zeros(count, dtype=np.complex128)
    todo = np.arange(count)
    while todo.size:
        v = (rng.integers(-5, 6, todo.size) + 1j * rng.integers(-5, 6, todo.size)) / 8.0
        good = (np.abs(v) >= 0.375) & (np.abs(v) <= 0.75)
        out[todo[good]] = v[good]
        todo = todo[~good]
    return out


BIG = (1.0, 1j, -1.0, -1j, (7 + 4j) / 8, (-4 + 7j) / 8)  # modulus 1 .. 1.008: above every _small value
TAP_SETS = "abcdefgh"


def largest_index(cls, A, nb, c):
    """Where tap set ``cls`` puts CPI c's largest tap (None: no tap at all)."""
    if cls == "a":
        return A if A < nb else nb - 1
    if cls == "b":
        return 0
    if cls == "c":
        assert A >= 2, "no anticipatory index other than 0"
        return (A - 1, 1, A // 2)[c % 3]
    if cls == "d":
        return nb - 1
    if cls == "e":
        cand = [k for k in (255, 256, 2047, 2048) if k < nb]
        assert cand, "no tap beyond a lane row"
        return cand[c % len(cand)]
    if cls == "f":
        return A if A < nb else 0
    if cls == "g":
        return None
    if cls == "h":
        cand = sorted({min(A, nb - 1), 0, nb - 1})
        return cand[c % len(cand)]
    raise ValueError(cls)


def taps(g, cls, B, n_bins=None, seed=0):
    """[B][n_bins] complex128: tap set ``cls`` (a .. h of the table below, or "mixed": CPI c takes class "acde"[c % 4];
    b for c with a single anticipatory tap, d for e with 255 taps or fewer) for geometry row g, every CPI with values of its own.

    a: the largest tap at index -delayMin (lag 0), strong taps at every anticipatory index and at nBins - 1
    b: the largest at index 0                       c: the largest at an anticipatory index other than 0
    d: the largest at nBins - 1                     e: the largest at 255 / 256 / 2047 / 2048 (one per CPI)
    f: two taps of equal largest modulus (lag 0 and nBins - 1)
    g: all zero                                     h: one single non-zero tap
    """
    A = -g.delay_min
    nb = default_bins(g) if n_bins is None else n_bins
    w = np.zeros((B, nb), dtype=np.complex128)
    for c in range(B):
        rng = np.random.default_rng(9000 + 100 * seed + c)
        k = "acde"[c % 4] if cls == "mixed" else cls
        if cls == "mixed" and k == "e" and nb <= 255:
            k = "d"
        if cls == "mixed" and k == "c" and A < 2:
            k = "b"
        top = largest_index(k, A, nb, c)
        if top is None:
            continue
        big = BIG[int(rng.integers(len(BIG)))]
        if k == "h":
            w[c, top] = big
            continue
        idx = sorted(set(i for i in antic_indices(A) + late_indices(A, nb) if i < nb) | {top})
        w[c, idx] = _small(rng, len(idx))
        w[c, top] = big
        if k == "f":
            second = nb - 1 if nb - 1 != top else 0
            if second != top:
                w[c, second] = big * 1j  # the same modulus, exactly
    return w


def multipath_taps(g, B, seed=0):
    """12 taps per CPI of modulus 0.1 .. 0.6 (multiples of 1/64), spread over the window, anticipatory ones included."""
    A, nb = -g.delay_min, default_bins(g)
    w = np.zeros((B, nb), dtype=np.complex128)
    for c in range(B):
        rng = np.random.default_rng(9500 + 100 * seed + c)
        idx = np.unique(np.concatenate([[0, A - 1, A, nb - 1], rng.integers(0, nb, 8)]))
        v = np.zeros(idx.size, dtype=np.complex128)
        for j in range(idx.size):
            while not 0.1 <= abs(v[j]) <= 0.6:
                v[j] = (rng.integers(-38, 39) + 1j * rng.integers(-38, 39)) / 64.0
        w[c, idx] = v
    return w


def k0_of(w_row):
    """taps_spectrum_kernel's choice: the first tap of the largest modulus (squared moduli of dyadics: exact in fp32)."""
    return int(np.argmax(w_row.real ** 2 + w_row.imag ** 2))


# ---- the census ---------------------------------------------------------------------------------------------------------
def edge_offsets(A):
    """Offsets j in [0, |delayMin|) of the census samples behind a pulse's end and at the CPI's start."""
    if A <= 8:
        return list(range(A))
    return sorted({0, 1, 2, 3, A // 2, A - 2, A - 1})


def populated_pulses(nD):
    return sorted({0, 1, nD // 2, nD - 1})


def census_positions(g, n_bins=None):
    """(CPI indices of x, CPI indices of y) of the census of row g.  Per populated pulse (start p0, nC samples, A = |delayMin|):

    x  0, 1, nC - 2, nC - 1, nC - A - 1, nC - A            the correlation's anchors at both ends
       nC + j, j in edge_offsets(A)                         the NEXT pulse's / the spare region's first samples: `tail`
       -1, -2, -(kmax - A), -(kmax - A) + 1                 the previous pulse's last samples, down to the last tap's reach:
                                                            the history block (not for pulse 0)
       g L - 1, g L, g L - A - 1, g L - A + 1               both sides of every block seam and of every segment seam
       j in edge_offsets(A) on pulse 0                      the samples the filter's stream does not hold: `head`
       nD nC + A, n - 1 where spare > A                     spare samples no tap reaches
    y  0, 1, nC - 2, nC - 1, j and nC - A + j, g L - 1, g L, g L - A     where those products land
    """
    d = dims_of(g)
    nD, nC, n = d.n_doppler_bins, d.n_corr, d.n_samples
    A = -g.delay_min
    kmax = (default_bins(g) if n_bins is None else n_bins) - 1
    J = edge_offsets(A)
    seams = [s * L for s in range(1, g.sb + 1)]
    ix, iy = set(), set()
    for i in populated_pulses(nD):
        p0 = i * nC
        q = {0, 1, nC - 2, nC - 1, nC - A - 1, nC - A}
        for s in seams:
            q |= {s - 1, s, s - A - 1, s - A + 1}
        q = {v for v in q if 0 <= v < nC}
        q |= {nC + j for j in J}
        if i > 0:
            q |= {-h for h in (1, 2, kmax - A - 1, kmax - A) if 1 <= h <= L}
        if i == 0:
            q |= set(J)
        ix |= {p0 + v for v in q}
        r = {0, 1, nC - 2, nC - 1} | set(J) | {nC - A + j for j in J}
        for s in seams:
            r |= {s - 1, s, s - A}
        iy |= {p0 + v for v in r if 0 <= v < nC}
    used = nD * nC
    if g.spare > A:
        ix |= {used + A, n - 1}
    return np.array(sorted(v for v in ix if 0 <= v < n), dtype=np.int64), np.array(sorted(iy), dtype=np.int64)


def gaussian_integers(rng, count):
    """``count`` values a + bj with 5 <= |a + bj| <= 7: the upper half of tests/range_crafted.py's moduli.  With the largest
    tap at lag 0 the map's peak is about sum |x|^2 over the whole census, a hundred samples, so the smallest planted
    product, 0.375 x 5 x 5, needs the impulses' moduli close together to stay above 1e-3 of it."""
    out = np.zeros(count, dtype=np.complex128)
    todo = np.arange(count)
    while todo.size:
        v = rng.integers(-7, 8, todo.size) + 1j * rng.integers(-7, 8, todo.size)
        good = (np.abs(v) >= 5) & (np.abs(v) <= 7)
        out[todo[good]] = v[good]
        todo = todo[~good]
    return out


def census(g, seed, y_populated=True, n_bins=None):
    """(x, y) complex128 of dims.n_samples: Gaussian integers (gaussian_integers above) at census_positions, zero
    elsewhere; y all zero where ``y_populated`` is False (the map is the filter term alone), except behind nD nCorr, where
    no kernel reads it."""
    d = dims_of(g)
    ix, iy = census_positions(g, n_bins)
    rng = np.random.default_rng(seed)
    x = np.zeros(d.n_samples, dtype=np.complex128)
    y = np.zeros(d.n_samples, dtype=np.complex128)
    x[ix] = gaussian_integers(rng, ix.size)
    vy = gaussian_integers(rng, iy.size)
    if y_populated:
        y[iy] = vy
    y[d.n_doppler_bins * d.n_corr:] = SPARE_Y
    return x, y


def smallest_product(d, x, y, w):
    """The smallest planted product: |tap| |x| |x| over the filter term, |y| |x| over the plain one."""
    used = d.n_doppler_bins * d.n_corr
    ax, ay, aw = np.abs(x), np.abs(y[:used]), np.abs(w)
    out = []
    if aw.any():
        out.append(aw[aw > 0].min() * ax[ax > 0].min() ** 2)
    if ay.any():
        out.append(ay[ay > 0].min() * ax[ax > 0].min())
    return float(min(out)) if out else 0.0


# ---- the reference ------------------------------------------------------------------------------------------------------
def filtered(x, y, w, delay_min):
    """y - (w * xs)[0:N], xs[i] = x[(i - delayMin) mod N], linear (xs[m < 0] = 0): oracle.blah2_oracle.wiener_hopf's last
    step, tap by tap in fp64."""
    x = np.asarray(x, dtype=np.complex128)
    N = x.shape[0]
    xs = x[(np.arange(N) - delay_min) % N]
    f = np.zeros(N, dtype=np.complex128)
    for k in np.flatnonzero(w):
        f[k:] += w[k] * xs[:N - k]
    return np.asarray(y, dtype=np.complex128) - f


def reference(d, x, y, w, delay_min):
    return O.ambiguity_process(d, x, filtered(x, y, w, delay_min))


MUTANTS = ("notail", "nohead", "nohistory", "k0masked", "leak", "taps0", "stride")


def filter_sparse(d, x, y, w, delay_min, mutant=None, w_other=None, x_next=None):
    """The same map by the time-domain definition, pulse by pulse as the kernel sees a pulse, over the populated samples and
    the non-zero taps only: y'[n] = y[n] - sum_k w[k] s(p0 + n - delayMin - k) with the filter's stream s(u) = x[u] for
    u >= |delayMin|, zero in front; R[i][c] = sum_a y'[a + lag_c] conj(x[p0 + a]) over 0 <= a, a + lag_c < nCorr.

    ``mutant``: a deliberately wrong restatement --
      notail     the stream masked to the pulse at its end            nohead   pulse 0 sees x[0 .. |delayMin|)
      nohistory  the stream zero in front of every pulse              leak     x past the pulse's end enters the correlation
      k0masked   the largest tap on the pulse's masked window (neither the look-ahead nor the zero start)
      taps0      the taps of another CPI (``w_other``)                stride   the last pulse's look-ahead reads ``x_next``'s
                                                                               first samples instead of the spare ones
    """
    nD, nC, nDelay = d.n_doppler_bins, d.n_corr, d.n_delay_bins
    A, used = -delay_min, nD * nC
    x = np.asarray(x, dtype=np.complex128)
    if mutant == "taps0":
        w = w_other
    xf = x
    if mutant == "stride":
        xf = x.copy()
        xf[used:] = x_next[:x.size - used]
    kk = np.flatnonzero(w)
    k0 = k0_of(w)
    ux, uf = np.flatnonzero(x), np.flatnonzero(xf)
    lags = delay_min + np.arange(nDelay)
    R = np.zeros((nD, nDelay), dtype=np.complex128)
    for i in range(nD):
        p0 = i * nC
        xa = ux[(ux >= p0) & (ux < p0 + nC + (A if mutant == "leak" else 0))]
        if xa.size == 0:
            continue
        yp = y[p0:p0 + nC].astype(np.complex128)
        sel = uf[(uf >= p0 - len(w)) & (uf < p0 + nC + A)]
        if sel.size and kk.size:
            U, K = sel[:, None], kk[None, :]
            n = U - A + K - p0
            seen = np.broadcast_to(U >= (0 if mutant == "nohead" else A), n.shape).copy()
            if mutant == "notail":
                seen &= U < p0 + nC
            if mutant == "nohistory":
                seen &= U >= p0
            if mutant == "k0masked":
                seen[:, kk == k0] = ((U >= 0) & (U < p0 + nC))
            ok = seen & (n >= 0) & (n < nC)
            vals = w[kk][None, :] * xf[sel][:, None]
            np.subtract.at(yp, n[ok], vals[ok])
        for u in xa:
            m = u - p0 + lags
            okm = (m >= 0) & (m < nC)
            R[i, okm] += yp[m[okm]] * np.conj(x[u])
    return RC._doppler(d, R)


# ---- the dense complement -------------------------------------------------------------------------------------------------
def dense_scene(g, seed):
    """int16-valued noise x, and y = a weak echo of it in noise with no direct path (tests/test_fused_fir_gpu.py synth with
    direct = 0), as complex128."""
    from test_fused_fir_gpu import synth
    n = dims_of(g).n_samples
    x, y = synth(n, n, seed, direct=0.0)
    return x.astype(np.complex128) + 0.0, y.astype(np.complex128) + 0.0


# ---- planes -------------------------------------------------------------------------------------------------------------
def host_planes(fmt_name, xs, ys, stride):
    """(x plane, y plane or None, samples in front of CPI 0): rows of ``stride`` samples per CPI, PAD samples in front of the
    first and behind the last, every sample that is not a CPI's filled with POISON.  FMT_C32: two complex64 planes; FMT_I16:
    one plane of int16 words I1 Q1 I2 Q2 (tuner 1 = x, tuner 2 = y)."""
    B, n = len(xs), xs[0].shape[0]
    assert stride >= n
    total = 2 * PAD + B * stride
    if fmt_name == "FMT_C32":
        out = []
        for chans in (xs, ys):
            host = np.full(total, POISON, dtype=np.complex64)
            for c, v in enumerate(chans):
                host[PAD + c * stride:PAD + c * stride + n] = v
            out.append(host)
        return out[0], out[1], PAD
    if fmt_name == "FMT_I16":
        host = np.empty((total, 4), dtype=np.int16)
        host[:] = (POISON.real, POISON.imag, POISON.real, POISON.imag)
        for c in range(B):
            for v in (xs[c], ys[c]):
                assert np.abs(v.real).max() < 32768 and np.abs(v.imag).max() < 32768 and np.array_equal(v.real, np.rint(v.real))
            host[PAD + c * stride:PAD + c * stride + n] = np.stack([xs[c].real, xs[c].imag, ys[c].real, ys[c].imag], axis=-1)
        return host, None, PAD
    raise ValueError(fmt_name)


# ---- the cases both test files run ----------------------------------------------------------------------------------------
# (row, tap set, n_bins or None for nDelay - 1): every row with set a; sets b .. h on past-5; the far taps on the long rows;
# filters shorter and longer than the map's window, all-anticipatory, of one tap, of the 2049 taps the kernel takes at most
CASES = tuple((g.name, "a", None) for g in GEOMS) + tuple(("past-5", k, None) for k in "bcdefgh") + (
    ("dmin0", "d", None), ("dmin0", "e", None), ("head-block1", "d", None), ("head-block1", "e", None),
    ("past-5", "a", 8), ("past-5", "a", 208), ("past-5", "d", 600), ("dmin0", "a", 1), ("dmin0", "d", 2049),
    ("past-5", "mixed", None),
)
Y_ZERO_CPI = 1  # the CPI of every batch whose surveillance channel is all zero: its map is the filter term alone
# CPI c's census seed is SEED0 + c.  With these seeds the first spare sample of every CPI differs from the next CPI's first
# sample by a modulus of 8 or more on the row with ONE anticipatory tap, so the `stride` mutant has a product to get wrong
# there (tests/test_fir_crafted_model.py computes it)
SEED0 = 50
_batches = {}


def case_id(case):
    return "-".join(str(v) for v in case if v is not None)


def batch(g, cls, n_bins=None, B=3):
    """{'d', 'xs', 'ys', 'w', 'refs'} of B distinct census CPIs of row g with tap set ``cls``: computed once, left unchanged."""
    key = (g, cls, n_bins, B)
    if key not in _batches:
        d = dims_of(g)
        w = taps(g, cls, B, n_bins)
        xy = [census(g, SEED0 + c, y_populated=c != Y_ZERO_CPI, n_bins=n_bins) for c in range(B)]
        xs, ys = [v[0] for v in xy], [v[1] for v in xy]
        refs = [reference(d, xs[c], ys[c], w[c], g.delay_min) for c in range(B)]
        _batches[key] = {"d": d, "xs": xs, "ys": ys, "w": w, "refs": refs}
    return _batches[key]
