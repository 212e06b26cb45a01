"""Crafted maps and a cell-by-cell statement of the greatest-of / smallest-of rule (include/blah2hip.h) for
test_gocfar_model.py and test_gocfar_gpu.py.

``rule`` walks the cells in plain Python loops, straight from the definition, and takes a ``variant`` that names one
deliberate mistake; the model test shows that the crafted maps tell every one of them from the rule, the GPU test compares
the device with ``gocfar_hits``, which the model test has compared with ``rule``."""
import zlib

import numpy as np

import cfar_crafted as X

GO, SO = 1, 2
G2_ROWS, G2_COLS = 16, 64          # gocfar_kernels.hpp: the cells of a 2-D tile
MAX_HR, MAX_HC = 24, 40            # the halo limits
VARIANTS = ("halves_swapped", "shared_count", "ca_factor", "and_or_exchanged", "column0_trains", "leading_k_ge_0",
            "guard_plus_one", "guard_minus_one", "rows_plus_one", "rows_minus_one")


def window3(window):
    w = tuple(int(v) for v in window)
    return w if len(w) == 3 else (w[0], w[1], 0)


def rule(m, delay, doppler, noise_power, alpha, kind, window, min_delay=-128, min_doppler=0.0, variant=None):
    """{(row, col): snr} of one map by the definition, one cell at a time.  ``alpha(a, b)``: the factor of a pair; ``variant``:
    None or one of VARIANTS."""
    assert variant is None or variant in VARIANTS
    g, t, hR = window3(window)
    if variant == "guard_plus_one":
        g += 1
    if variant == "guard_minus_one":
        g = max(g - 1, 0)
    if variant == "rows_plus_one":
        hR += 1
    if variant == "rows_minus_one":
        hR = max(hR - 1, 0)
    m = np.asarray(m)
    re, im = m.real.astype(np.float64), m.imag.astype(np.float64)
    p = re * re + im * im
    nD, nC = p.shape
    first = 0 if variant in ("column0_trains", "leading_k_ge_0") else 1
    out = {}
    with np.errstate(all="ignore"):
        for i in range(nD):
            if abs(float(doppler[i])) < min_doppler:
                continue
            rows = [ii for ii in range(i - hR, i + hR + 1) if 0 <= ii < nD]
            for j in range(nC):
                if int(delay[j]) < min_delay:
                    continue
                A = [k for k in range(j - g - t, j - g) if first <= k < nC]
                B = [k for k in range(j + g + 1, j + g + t + 1) if 0 <= k < nC]
                a, b = len(rows) * len(A), len(rows) * len(B)

                def total(cols):
                    s = np.float64(0.0)
                    for k in cols:
                        c = np.float64(0.0)
                        for ii in rows:
                            c = c + p[ii, k]
                        s = s + c
                    return s

                SA, SB, pc = total(A), total(B), p[i, j]
                if variant == "halves_swapped":  # each sum with the other half's count (the rule itself is symmetric)
                    SA, SB = SB, SA
                if a == 0 and b == 0:
                    continue
                if a == 0 or b == 0:
                    hit = pc > np.float64(alpha(a, b)) * ((SA if a else SB) / np.float64(a + b))
                else:
                    al = np.float64(alpha(a, b))
                    if variant == "ca_factor":
                        n = a + b
                        al = np.float64(n * (pow_pfa(alpha) ** (-1.0 / n) - 1))
                    if variant == "shared_count":
                        hA, hB = pc > al * (SA / np.float64((a + b) / 2.0)), pc > al * (SB / np.float64((a + b) / 2.0))
                    else:
                        hA, hB = pc > al * (SA / np.float64(a)), pc > al * (SB / np.float64(b))
                    use_and = (kind == GO) != (variant == "and_or_exchanged")
                    hit = (hA and hB) if use_and else (hA or hB)
                if hit:
                    out[(i, j)] = float(5.0 * np.log10(pc) - noise_power)
    return out


def pow_pfa(alpha):
    """The pfa an ``alpha`` callable made by :func:`factors` was built for."""
    return alpha.pfa


def factors(b2, pfa, kind):
    """``alpha(a, b)`` from the pure-Python restatement, remembered per pair."""
    memo = {}

    def alpha(a, b):
        if (a, b) not in memo:
            memo[(a, b)] = b2.gocfar_alpha(pfa, kind, a, b)
        return memo[(a, b)]

    alpha.pfa = pfa
    return alpha


def hits_dict(rcs):
    r, c, s = rcs
    return {(int(i), int(j)): float(v) for i, j, v in zip(r, c, s)}


def noise_map(name, nD, nC, B=1, plant=40, column0=1e15, nonfinite=False):
    """complex64 [B, nD, nC]: an exponential power floor, ``plant`` cells 10 - 50 dB up at random places, on the edges and
    either side of the 2-D tile's seams, a huge cell in every row of delay column 0 (it trains nowhere), and with
    ``nonfinite`` a NaN and a +Inf cell inside the map -- each a training cell of its neighbours and a cell under test."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    amp = np.sqrt(rng.exponential(1.0, (B, nD, nC)))
    rows = sorted({r for r in (0, 1, nD - 2, nD - 1, G2_ROWS - 1, G2_ROWS, 2 * G2_ROWS - 1, 2 * G2_ROWS) if 0 <= r < nD})
    cols = sorted({c for c in (0, 1, 2, nC - 2, nC - 1, G2_COLS - 1, G2_COLS, 2 * G2_COLS - 1, 2 * G2_COLS) if 0 <= c < nC})
    for c in range(B):
        k = min(plant, max(nD * nC // 8, 1))
        ii = np.concatenate([rng.integers(0, nD, k), rng.choice(rows, k), rng.integers(0, nD, k)])
        jj = np.concatenate([rng.integers(0, nC, k), rng.integers(0, nC, k), rng.choice(cols, k)])
        amp[c, ii, jj] *= 10.0 ** (rng.uniform(10.0, 50.0, ii.size) / 20.0)
    m = (amp * np.exp(2j * np.pi * rng.uniform(0, 1, amp.shape))).astype(np.complex64)
    if column0:
        m[:, :, 0] = np.float32(np.sqrt(column0))
    if nonfinite and nC > 6 and nD > 2:
        m[:, nD // 3, nC // 3] = np.complex64(complex(np.nan, 1.0))
        m[:, (2 * nD) // 3, (2 * nC) // 3] = np.complex64(complex(np.inf, 0.0))
    return m


def flat_col(window):
    """The column whose leading half is delay column 1 alone."""
    return window3(window)[0] + 2


def flat_map(b2, pfa, kind, window, nD, nC):
    """A floor of power 1 with two cells planted in column ``flat_col``, where the leading half is one column and the lagging
    half at least four (b >= 4 a), in rows 1 and nD - 2.  With a flat floor both half means are 1, so the cell's power against the factors decides:
    row 1 holds 1.25 alpha (greatest-of: a hit, lost as soon as a sum is divided by another count than its own) or
    0.75 alpha (smallest-of: no hit, gained by the same mistakes); row nD - 2 holds the middle between alpha and the
    averaging factor of a + b cells (a hit for greatest-of and none for smallest-of, the other way round under that factor).
    Cells of one column never train each other."""
    m = np.ones((nD, nC), dtype=np.complex64)
    a, b = b2.gocfar_counts(nD, nC, window)
    col = flat_col(window)
    for r, which in ((1, "count"), (nD - 2, "factor")):
        x, y = int(a[r, col]), int(b[r, col])
        assert 0 < 4 * x <= y
        al = b2.gocfar_alpha(pfa, kind, x, y)
        ca = b2.cfar_alpha(pfa, 1, x + y)[x + y]
        power = (1.25 if kind == GO else 0.75) * al if which == "count" else 0.5 * (al + ca)
        m[r, col] = np.float32(np.sqrt(power))
    return m


def metrics_for(B):
    return np.stack([3.0 + 7.5 * np.arange(B), 1.0 + np.arange(B)], axis=1).astype(np.float64)


def step_scene(rng, nD=256, nC=128, step=64, db=20.0):
    """Complex Gaussian noise of unit power with a power step of ``db`` from column ``step`` on."""
    z = (rng.standard_normal((nD, nC)) + 1j * rng.standard_normal((nD, nC))) / np.sqrt(2.0)
    z[:, step:] *= 10.0 ** (db / 20.0)
    return z.astype(np.complex64)


def pair_scene(rng, nD=256, nC=128, cols=(60, 65), db=17.0):
    """Unit-power noise with two echoes of ``db`` over noise in every row, random phases, added to the noise."""
    z = (rng.standard_normal((nD, nC)) + 1j * rng.standard_normal((nD, nC))) / np.sqrt(2.0)
    for c in cols:
        z[:, c] += 10.0 ** (db / 20.0) * np.exp(2j * np.pi * rng.uniform(0, 1, nD))
    return z.astype(np.complex64)


def ca_hits(b2, m, window, pfa):
    """The averaging detector's cells on one map, by the same walk: a set of (row, col)."""
    g, t = window
    p = np.asarray(m).real.astype(np.float64) ** 2 + np.asarray(m).imag.astype(np.float64) ** 2
    nD, nC = p.shape
    al = b2.cfar_alpha(pfa, 1, 2 * t)
    out = set()
    for j in range(nC):
        ks = [k for k in range(j - g - t, j - g) if 0 < k < nC] + [k for k in range(j + g + 1, j + g + t + 1) if k < nC]
        if not ks:
            continue
        tot = np.zeros(nD)
        for k in ks:
            tot = tot + p[:, k]
        out.update((int(i), j) for i in np.flatnonzero(p[:, j] > al[len(ks)] * (tot / len(ks))))
    return out


geom, dims_of = X.geom, X.dims_of
