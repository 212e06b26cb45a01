"""Scenes and a NumPy fp32 emulation for the multi-carrier integration (csrc/carrier_kernels.hpp carrier_sum_kernel,
csrc/carriers.hip).  Helpers only, no tests; no GPU is touched at import.  The stage has no reference counterpart: the
oracle is the fp64 restatement ``blah2_amd.carrier_table`` / ``blah2_amd.fuse_carriers``.

``noise_scene``: maps of 65 x 48 cells of unit-power complex Gaussian noise for four carriers with the ratios (1, 1.25, 0.8,
1.1) on the axis -32 .. 32, and an echo of power 8 in every carrier at row ``32 + rint(16 ratio)``, column 20: one target of
one range rate, 16 rows from the centre in the reference carrier.  Summed along the right table the echo's cell holds four
looks of the echo; summed row by row (every ratio taken as 1) it holds one.

``emulate``: the kernel's arithmetic in fp32 NumPy on the flat input ``[C][n_cpi][cells]`` as the kernel addresses it -- p_lo =
fma(re, re, im im), q = a_lo p_lo, q = fma(a_hi, p_hi, q) where a_hi != 0, S = fma(w_c, q, S), sqrt(scale S) -- with every
fused multiply-add evaluated in fp64 and rounded once (the 48-bit product is exact there).  ``MUTANTS`` are the mistakes a
gather of this kind invites.

``capture``: the synthetic wideband int16 capture of the replay tests (see there).
"""
import numpy as np

RATIOS = (1.0, 1.25, 0.8, 1.1)
SCENE_ROWS, SCENE_COLS, SCENE_ECHO_ROW, SCENE_ECHO_COL, SCENE_ECHO_POWER = 65, 48, 16, 20, 8.0
SCENE_SEED = 20261021

MUTANTS = ("row-off-one", "weights-swapped", "clamped-zero", "no-weights", "no-scale", "carrier-stride")


def scene_axis():
    return np.arange(SCENE_ROWS, dtype=np.float64) - SCENE_ROWS // 2


def noise_scene(seed=SCENE_SEED, n_cpi=1):
    """(maps complex128 [4, n_cpi, 65, 48], the echo's output cell (row, col))."""
    rng = np.random.default_rng(seed)
    shape = (len(RATIOS), n_cpi, SCENE_ROWS, SCENE_COLS)
    m = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
    for c, r in enumerate(RATIOS):
        row = SCENE_ROWS // 2 + int(np.rint(SCENE_ECHO_ROW * r))
        phase = rng.uniform(0, 2 * np.pi, n_cpi)
        m[c, :, row, SCENE_ECHO_COL] += np.sqrt(SCENE_ECHO_POWER) * np.exp(1j * phase)
    return m, (SCENE_ROWS // 2 + SCENE_ECHO_ROW, SCENE_ECHO_COL)


def _fma(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 is exact in fp64; one rounding of the sum to fp64, one to fp32."""
    return (np.asarray(a, dtype=np.float32).astype(np.float64) * np.asarray(b, dtype=np.float32).astype(np.float64)
            + np.asarray(c, dtype=np.float32).astype(np.float64)).astype(np.float32)


def emulate(maps, table, w=None, mutant=None, out_of_axis=None):
    """carrier_sum_kernel over ``maps`` complex64 [C, n_cpi, nD, nC] -> fp32 [n_cpi, nD, nC] (the real parts).
    ``out_of_axis``: :func:`uncovered`'s mask, for the mutant that reads the clamped rows as zero."""
    assert mutant is None or mutant in MUTANTS
    m = np.ascontiguousarray(maps, dtype=np.complex64)
    C_, n_cpi, nD, nC = m.shape
    cells = nD * nC
    flat = m.reshape(C_ * n_cpi, nD, nC)
    stride = 1 if mutant == "carrier-stride" else n_cpi  # maps from one carrier to the next
    wc = np.ones(C_, dtype=np.float32) if w is None else np.asarray(w, dtype=np.float32)
    scale = np.float32(1.0 / wc.astype(np.float64).sum())
    if mutant == "no-weights":
        wc = np.ones(C_, dtype=np.float32)
    if mutant == "no-scale":
        scale = np.float32(1.0)
    row, a_lo, a_hi = (np.asarray(table[k]).copy() for k in ("row", "a_lo", "a_hi"))
    if mutant == "weights-swapped":
        a_lo, a_hi = a_hi, a_lo
    zero = np.zeros((C_, nD), dtype=bool)
    if mutant == "clamped-zero":  # a row the carrier does not cover contributes nothing
        zero = np.asarray(out_of_axis, dtype=bool)
        assert zero.shape == (C_, nD)
    if mutant == "row-off-one":
        row = np.minimum(row + 1, nD - 1)
    re, im = flat.real.astype(np.float32), flat.imag.astype(np.float32)
    p = _fma(re, re, im * im)  # [C n_cpi, nD, nC]
    out = np.zeros((n_cpi, nD, nC), dtype=np.float32)
    for i in range(n_cpi):
        S = np.zeros((nD, nC), dtype=np.float32)
        for c in range(C_):
            pc = p[c * stride + i]
            q = a_lo[c][:, None].astype(np.float32) * pc[row[c]]
            assert q.dtype == np.float32
            hi = a_hi[c] != 0
            if hi.any():
                q[hi] = _fma(a_hi[c][hi, None], pc[np.minimum(row[c][hi] + 1, nD - 1)], q[hi])
            q[zero[c]] = 0
            S = _fma(wc[c], q, S)
        out[i] = np.sqrt(scale * S)
        assert out.dtype == np.float32
    assert cells == out[0].size
    return out


def uncovered(axis, ratio):
    """bool [C, nD]: the rows a carrier does not cover, from the definition: ratio[c] doppler[j] lies outside the axis (by
    more than the table's snap of 1e-9 rows)."""
    axis, ratio = np.asarray(axis, dtype=np.float64), np.asarray(ratio, dtype=np.float64)
    nD = axis.size
    u = (ratio[:, None] * axis[None, :] - axis[0]) / ((axis[-1] - axis[0]) / (nD - 1))
    return (u < -1e-9) | (u > nD - 1 + 1e-9)


def bound(C_, ref):
    """The derived cell bound: at most 4 roundings up to q, one per carrier in S, one for the scale -- C + 5 relative errors
    of 2^-24 on non-negative terms, halved by the square root -- plus at most 2 units for sqrtf: below (C + 8) 2^-24 ref."""
    return (C_ + 8) * 2.0 ** -24 * np.asarray(ref, dtype=np.float64)


# ---- the wideband capture of the replay tests ---------------------------------------------------------------------------------
# fs = 65 536 Hz, CPIs of one second, two carriers at -16 384 Hz (carrier 0, the reference axis) and +16 384 Hz carrying
# independent noise-like programmes, band-limited to |nu| <= 0.08 cycles per sample and of unit power.  capture.fc = 655 360 Hz:
# the ratio is 671 744 / 638 976 = 1.0513.  x is the programmes' sum; y is 0.2 x, ONE target in both carriers -- each programme
# delayed by 24 samples, at 40 Hz in carrier 0 and 40 x ratio = 42.05 Hz in carrier 1, amplitude ECHO -- and noise of 0.01 per
# component -- and a strong echo of carrier 0's programme alone (delay 40 samples, 62 Hz, amplitude 0.03), which carrier 1
# does not cover: 62 x ratio lies beyond the axis' 64 Hz.  Down-converted by D = 4 with 64 taps each carrier is a 16 384-sample CPI at 16 384 Hz: 1 Hz Doppler bins, the
# echo at delay 6, row 40 Hz of carrier 0's map and row 42 Hz of carrier 1's, two rows apart.
FS, N, D, T = 65536, 65536, 4, 64
FC = 655360.0
OFFSETS = (-16384.0, 16384.0)
RATIO = (FC + OFFSETS[1]) / (FC + OFFSETS[0])
AMB_ARGS = (-4, 20, -64, 64, FS // D, N // D)
ECHO_DELAY, ECHO_DOPPLER = 24, 40.0
PEAK = (6, 40.0)  # (delay, Doppler) of the fused map's cell, on carrier 0's axis
ECHO = 0.0087     # the target's amplitude (tests/test_carriers_replay_gpu.py says how it was chosen)
EDGE_DELAY, EDGE_DOPPLER, EDGE_ECHO = 40, 62.0, 0.03  # a strong echo in carrier 0 alone, on a row carrier 1 does not cover
EDGE_PEAK = (10, 62.0)
CAPTURE_SEED, CAPTURE_CPIS = 20261022, 3


def _band_limited(rng, n, band):
    w = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    W = np.fft.fft(w)
    W[np.abs(np.fft.fftfreq(n)) > band] = 0
    x = np.fft.ifft(W)
    return x / np.sqrt(np.mean(np.abs(x) ** 2))


def stream(echo=ECHO, n_cpi=CAPTURE_CPIS, seed=CAPTURE_SEED):
    """(x, y) complex128 of n_cpi N samples: one continuous stream."""
    rng = np.random.default_rng(seed)
    n = n_cpi * N
    t = np.arange(n) / FS
    ill = [_band_limited(rng, n, 0.08) * np.exp(2j * np.pi * f * t) for f in OFFSETS]
    x = ill[0] + ill[1]
    y = 0.2 * x
    for s, f in zip(ill, (ECHO_DOPPLER, ECHO_DOPPLER * RATIO)):
        e = np.zeros(n, dtype=np.complex128)
        e[ECHO_DELAY:] = s[:n - ECHO_DELAY]
        y = y + echo * e * np.exp(2j * np.pi * f * t)
    e = np.zeros(n, dtype=np.complex128)
    e[EDGE_DELAY:] = ill[0][:n - EDGE_DELAY]
    y = y + EDGE_ECHO * e * np.exp(2j * np.pi * EDGE_DOPPLER * t)
    y = y + 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x, y


def quantise(x, y, full=30000.0):
    """The stream as the int16 words of a .rspduo capture [n, 4] and as the complex128 integers [2, n] they hold."""
    out = []
    for v in (x, y):
        s = full / max(np.max(np.abs(v.real)), np.max(np.abs(v.imag)))
        out += [np.rint(v.real * s), np.rint(v.imag * s)]
    return np.stack(out, axis=1).astype(np.int16), np.stack([out[0] + 1j * out[1], out[2] + 1j * out[3]])


def carrier_maps(u, n_cpi=CAPTURE_CPIS):
    """The fp64 restatement chain in front of the sum: blah2_amd.ddc of the whole stream ``u`` [2, n] per carrier, then the
    oracle's ambiguity stage per CPI -> (dims, complex128 [2, n_cpi, nD, nC])."""
    import blah2_amd
    from oracle import blah2_oracle as O
    dims = O.ambiguity_dims(*AMB_ARGS)
    h = blah2_amd.ddc_design(D, T, 0.8, 8.0)
    n = N // D
    maps = []
    for f in OFFSETS:
        v, _ = blah2_amd.ddc(u, f, FS, D, h)
        maps.append([O.ambiguity_process(dims, v[0, c * n:(c + 1) * n], v[1, c * n:(c + 1) * n]) for c in range(n_cpi)])
    return dims, np.array(maps)


def margins(level, pfa, n_guard, n_train, looks):
    """|z|^2 / threshold per cell (fp64) of the cell-averaging detector made for ``looks`` looks on the real map ``level``
    [nD, nC] (CfarDetector1D.cpp:55-83 with blah2_amd.cfar_alpha's factors; training cells k > 0 on the left, as there)."""
    import blah2_amd
    sq = np.asarray(level, dtype=np.float64) ** 2
    nD, nC = sq.shape
    alpha = np.asarray(blah2_amd.cfar_alpha_table(pfa, looks, 2 * n_train))
    out = np.zeros(sq.shape)
    for j in range(nC):
        idx = [k for k in range(j - n_guard - n_train, j - n_guard) if 0 < k < nC]
        idx += [k for k in range(j + n_guard + 1, j + n_guard + n_train + 1) if 0 <= k < nC]
        out[:, j] = sq[:, j] / (alpha[len(idx)] * sq[:, idx].mean(axis=1)) if idx else 0.0
    return out
