"""CPU: what the correlation census of tests/corr_crafted.py can see.

fp64 NumPy models of the two decompositions as the kernels do them (csrc/clutter_kernels.hpp):

  windowed     per segment g of seg_len samples the transform of x' (the window [g S, g S + F) of xs, cut to the segment and
               to the CPI) against the transforms of the whole windows of xs and of every y_c (wrapWin's indices), the
               segments dealt to the workgroups by seg_walk, one partial per workgroup, the partials summed;
  half-window  segments of L = F/2 samples, X_g + (-1)^m X_{g-1}, runs of `per` segments with the transform of the segment
               in front of a run, the short last segment, and the wrap product W_F^(tau m) of the last workgroup.

Asserted: on every geometry and grid that the GPU file runs both models equal the direct sums over impulse pairs, and those
the oracle, to 1e-12 of the normaliser; every planted product is at least 1e-3 of its normaliser (a hundred gates); the
census is exact in int8; the restated index map is the oracle's; and each of thirteen mutants of the models moves r or some
b_c by at least 100 gates at some lag on the geometry named in MUTANTS, which the GPU file runs at that grid.

The gates are those of the GPU file: |r - r_ref| <= 1e-5 r_ref[0], |b_c - b_ref| <= 1e-5 sqrt(r_ref[0] sum |y_c|^2)."""
import numpy as np
import pytest

import corr_crafted as CC
from oracle import blah2_oracle as O

TIE = 1e-12
FILL = CC.FILL * (1 + 1j)


def ext(v, lo, hi):
    """v[lo:hi] where what lies behind the CPI is the filler of the gap."""
    out = np.full(hi - lo, FILL, dtype=np.complex128)
    n = max(0, min(hi, v.shape[0]) - lo)
    out[:n] = v[lo:lo + n]
    return out


def pad(v, F):
    out = np.zeros(F, dtype=np.complex128)
    out[:v.shape[0]] = v
    return out


def model_window(g, grid, xs, ys, mut):
    N, F, nb, S = g.N, g.F, g.n_bins, CC.seg_len_of(g)
    n_seg = CC.cdiv(N, S)
    s8 = CC.cdiv(n_seg, 8)
    m = np.arange(F)
    r = np.zeros(nb, dtype=np.complex128)
    b = np.zeros((len(ys), nb), dtype=np.complex128)
    for walk in CC.window_walks(n_seg, grid):
        accR = np.zeros(F, dtype=np.complex128)
        accB = np.zeros((len(ys), F), dtype=np.complex128)
        for it, s in enumerate(walk):
            if mut == 8 and it == 1:
                continue
            if mut == 9 and s > 0 and s % s8 == 0 and it == 0:
                continue
            n0 = s * S
            idx = np.minimum(n0 + m, 2 * N - 1)  # wrapWin
            idx = np.where(idx >= N, idx - N, idx)
            live = np.ones(F) if mut != 6 else (m < F - 1)
            wx = xs[idx] * live
            cut = (n0 + m < N) if mut == 7 else ((m < S) & (n0 + m < N))
            V = np.fft.fft(np.where(cut, xs[idx], 0))
            accR += np.fft.fft(wx) * np.conj(V)
            for c, y in enumerate(ys):
                accB[c] += np.fft.fft(y[idx] * live) * np.conj(V)
        r += np.fft.ifft(accR)[:nb]  # one partial per workgroup
        b += np.fft.ifft(accB, axis=1)[:, :nb]
    return r, b


def model_half(g, grid, xs, ys, mut):
    N, F, nb = g.N, g.F, g.n_bins
    L, tau = F // 2, nb - 1
    sgn = np.where(np.arange(F) & 1, -1.0, 1.0) if mut != 4 else np.ones(F)
    per, runs = CC.half_walks(N, F, grid)
    r = np.zeros(nb, dtype=np.complex128)
    b = np.zeros((len(ys), nb), dtype=np.complex128)
    for job, run in enumerate(runs):
        accR = np.zeros(F, dtype=np.complex128)
        accB = np.zeros((len(ys), F), dtype=np.complex128)
        prev = np.zeros(F, dtype=np.complex128)
        if run and run[0] > 0 and mut != 2:  # the segment in front of the run (a full one)
            prev = np.fft.fft(pad(xs[(run[0] - 1) * L:run[0] * L], F))
        for s in run:
            n0 = s * L
            ln = L if mut == 5 else min(L, N - n0)
            X = np.fft.fft(pad(ext(xs, n0, n0 + ln), F))
            z = X + sgn * prev
            accR += X * np.conj(z)
            for c, y in enumerate(ys):
                accB[c] += np.fft.fft(pad(ext(y, n0, n0 + ln), F)) * np.conj(z)
            if mut != 3:
                prev = X
        wrap = job == grid - 1 and nb > 1 and mut != 1 and not (mut == 13 and not run)
        if wrap:
            ph = np.exp(-2j * np.pi * ((np.arange(F) * tau) % F) / F)  # W_F^(tau m)
            z = np.fft.fft(pad(xs[N - tau:], F)) * np.conj(ph)
            accR += np.fft.fft(pad(xs[:tau], F)) * np.conj(z)
            for c, y in enumerate(ys):
                accB[c] += np.fft.fft(pad(y[:tau], F)) * np.conj(z)
        r += np.fft.ifft(accR)[:nb]
        b += np.fft.ifft(accB, axis=1)[:, :nb]
    return r, b


def model(g, grid, c, mut=0):
    """r [nBins], b [4][nBins] of CPI c as the kernels' passes form them: r and b_0, then (b_1, b_2) in one NB = 2 pass, then b_3."""
    cs = CC.census_for(g)
    xs = cs.x[c][CC.xs_indices(g.N, g.dmin, off_by_one=(mut == 12))]
    ys = [cs.ys[c, k] for k in range(CC.MAX_SURV)]
    if mut == 11:
        ys[2] = ys[1]  # the pass's second plane read as its first
    r, b = (model_half if g.form == "half" else model_window)(g, grid, xs, ys, mut)
    if mut == 10:
        b[[1, 2]] = b[[2, 1]]
    return r, b


_direct = {}


def direct(g, c):
    if (g.name, c) not in _direct:
        cs = CC.census_for(g)
        rb = [CC.direct_sums(cs.x[c], cs.ys[c, k], g.dmin, g.n_bins) for k in range(CC.MAX_SURV)]
        _direct[(g.name, c)] = (rb[0][0], np.stack([v[1] for v in rb]))
    return _direct[(g.name, c)]


def gates_moved(g, c, r, b):
    """max over lags of |difference| / normaliser, in units of the 1e-5 gate: (r, worst b_c)."""
    r_ref, b_ref = direct(g, c)
    er = np.max(np.abs(r - r_ref)) / CC.normalisers(g, c, 0)[0] / CC.R_TOL
    eb = max(np.max(np.abs(b[k] - b_ref[k])) / CC.normalisers(g, c, k)[1] / CC.B_TOL for k in range(CC.MAX_SURV))
    return er, eb


def grids_of(g):
    """The geometry's grids, the planner's as an MI355X (256 CUs) chooses it for the geometry's batch."""
    return [gr or CC.planner_grid(g, 256, CC.BATCH_CPIS if g is CC.BATCH_GEOM else g.B) for gr in g.grids]


@pytest.mark.parametrize("g", CC.GEOMS + [CC.BATCH_GEOM], ids=lambda g: g.name)
def test_models_equal_direct_sums_and_census_is_sound(g):
    cs = CC.census_for(g)
    assert np.array_equal(CC.xs_indices(g.N, g.dmin), CC.oracle_indices(g.N, g.dmin)), "xs_index restated != the oracle's line"
    # exact in int8, distinct values, distinct CPIs, about 50 impulses per CPI and channel
    allv = np.concatenate([cs.x.ravel(), cs.ys.ravel()])
    nz = allv[allv != 0]
    assert np.array_equal(nz.real, np.rint(nz.real)) and np.array_equal(nz.imag, np.rint(nz.imag))
    assert np.abs(nz.real).max() <= 127 and np.abs(nz.imag).max() <= 127
    assert len(set(nz.tolist())) == nz.size, "census values repeat"
    mod = np.abs(nz)
    assert mod.max() / mod.min() <= 3
    for c in range(g.B):
        assert 0 < np.count_nonzero(cs.x[c]) <= 64 and all(0 < np.count_nonzero(cs.ys[c, k]) <= 80 for k in range(CC.MAX_SURV))
        assert all(not np.array_equal(cs.x[c], cs.x[d]) for d in range(c))
    # every planted product against its normaliser
    idx = CC.oracle_indices(g.N, g.dmin)
    least = np.inf
    for c, n, k in cs.planted:
        xs = cs.x[c][idx]
        r0, _ = CC.normalisers(g, c, 0)
        least = min(least, abs(xs[(n + k) % g.N] * np.conj(xs[n])) / r0)
        for ch in range(CC.MAX_SURV):
            least = min(least, abs(cs.ys[c, ch, (n + k) % g.N] * np.conj(xs[n])) / CC.normalisers(g, c, ch)[1])
    assert least >= 1e-3, least
    # the oracle, the direct sums and the models
    for c in range(g.B):
        r_d, b_d = direct(g, c)
        for ch in range(CC.MAX_SURV):
            r_o, b_o = CC.oracle_rb(g, c, ch)
            if ch == (c + g.n_bins) % CC.MAX_SURV:  # the whole oracle on one channel per CPI: the same bits
                full = O.wiener_hopf(cs.x[c], cs.ys[c, ch], g.dmin, g.dmin + g.n_bins, return_filter=True)
                assert np.array_equal(full[3], r_o) and np.array_equal(full[4], b_o)
            r0, bn = CC.normalisers(g, c, ch)
            assert abs(r_o[0].real - r0) <= TIE * r0
            assert np.max(np.abs(r_o - r_d)) <= TIE * r0, (c, ch)
            assert np.max(np.abs(b_o - b_d[ch])) <= TIE * bn, (c, ch)
        for grid in grids_of(g):
            er, eb = gates_moved(g, c, *model(g, grid, c))
            assert max(er, eb) * CC.R_TOL <= TIE, (grid, c, er, eb)
    print(f"\n[corr census {g.name}] {len(cs.planted)} planted lags, least product / normaliser {least:.2e}")


# mutant -> (what is wrong, the geometry and grid of the GPU file that sees it)
MUTANTS = {
    1: ("the wrap product is dropped", "half1024_33taps_39L3", 8),
    2: ("prevX is zero at a run front", "half2048_33taps_39L3", 8),
    3: ("prevX is not carried inside a run", "half4096_33taps_39L3", 8),
    4: ("the (-1)^m sign is dropped", "half2048_tauL_41L", 8),
    5: ("the short last segment is read as L samples", "half1024_33taps_40L3", 8),
    6: ("the window's last sample is dropped", "win2048_410taps_40seg", 8),
    7: ("x' is not cut at segLen", "win1024_110taps_43seg", 16),
    8: ("a workgroup's second segment is not accumulated", "win4096_2100taps_40seg", 16),
    9: ("an XCD eighth's first segment is skipped", "win1024_110taps_10seg", 8),
    10: ("rows row0 and row0 + 1 are swapped in an NB = 2 pass", "win2048_410taps_43seg", 8),
    11: ("y1 is read as y0", "half4096_tauL_41L", 8),
    12: ("the xs shift is off by one at thresh", "win1024_110taps_40seg", 8),
    13: ("the empty last job does not do the wrap", "half1024_tauL_41L", 8),
}


@pytest.mark.parametrize("mut", sorted(MUTANTS), ids=lambda m: f"mutant{m}")
def test_every_mutant_moves_the_correlations_a_hundred_gates(mut):
    what, name, grid = MUTANTS[mut]
    g = CC.BY_NAME[name]
    assert grid in g.grids
    worst = max(max(gates_moved(g, c, *model(g, grid, c, mut))) for c in range(g.B))
    print(f"\n[corr mutant {mut}: {what}] {name} grid {grid}: {worst:.0f} gates")
    assert worst >= 100, (what, worst)


def test_every_mutant_is_seen_wherever_its_code_runs():
    """Beyond the one geometry each mutant names: the half-window mutants on every half-window geometry with runs, the
    windowed ones on every windowed geometry with walks (printed; asserted: no such geometry is blind to all CPIs)."""
    for mut, (what, name, _) in MUTANTS.items():
        form = CC.BY_NAME[name].form
        for g in CC.GEOMS:
            if g.form != form or not g.walk or mut in (10, 11, 12, 13, 7, 9):
                continue
            if g.F == 4096:
                continue  # the same arithmetic at a larger transform: kept out for the suite's time
            if mut == 5 and g.N % (g.F // 2) == 0:
                continue  # no short last segment there
            worst = max(max(gates_moved(g, c, *model(g, g.grids[0], c, mut))) for c in range(g.B))
            assert worst >= 100, (mut, what, g.name, worst)


def test_walks_restated():
    """seg_walk and half.per by hand at the sizes the GPU file relies on."""
    w = CC.window_walks(10, 8)  # s8 = 2: XCDs 0 ... 4 own two segments each, 5 ... 7 none
    assert w == [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9], [], [], []]
    w = CC.window_walks(43, 16)  # s8 = 6, step 2; XCD 7 owns segment 42 alone
    assert w[0] == [0, 2, 4] and w[8] == [1, 3, 5] and w[7] == [42] and w[15] == []
    assert sorted(s for walk in w for s in walk) == list(range(43))
    assert max(map(len, CC.window_walks(40, 8))) == 5 and max(map(len, CC.window_walks(43, 8))) == 6
    per, runs = CC.half_walks(41 * 512, 1024, 8)
    assert per == 6 and runs[6] == [36, 37, 38, 39, 40] and runs[7] == []
    per, runs = CC.half_walks(39 * 512 + 3, 1024, 8)
    assert per == 5 and all(len(r) == 5 for r in runs)
    for g in CC.GEOMS:
        if g.walk:
            assert max(map(len, CC.walks_of(g, g.grids[0]))) == g.walk, g.name
    g = CC.BY_NAME["half1024_33taps_39L3"]
    assert CC.planner_grid(CC.BATCH_GEOM, 256, CC.BATCH_CPIS) == 32 and CC.half_walks(CC.BATCH_GEOM.N, 1024, 32)[0] == 4
    assert CC.plan_jobs(g, 256) == 24 and CC.planner_grid(g, 256, 3) == 24 and CC.planner_grid(g, 256, 256) == 8
