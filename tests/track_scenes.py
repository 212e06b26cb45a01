"""Shared by tests/test_tracks_model.py (CPU), tests/test_tracks_gpu.py and tests/test_tracks_replay_gpu.py: the walk tables,
the banks, the shared crafted input, an fp32 emulation of track_power_kernel / track_sum_kernel with its wrong variants, and
the walking-echo scene of the tests of integration along tracks.  No test in here, no GPU, no library call.

The shared input: integrate_crafted.maps on 21 x 111 cells (every cell differs), one channel, W = 4, 6 CPIs, the bank
(0, 1, -1) and the ``alternating`` table -- walk 0.9 cells per CPI with the sign of the row's parity, 0 in the first and the
last row.  That table is chosen so that NO TWO HYPOTHESES CAN COINCIDE in any cell: the rates +-1 reach rows j -+ a, whose
walks cancel the row's own (or, next to the ends, round to a shift of 0), so their age-1 term is inside the map at every
column; in the first row +1 has that term alone left out, in the last row -1 has, and the rate 0 keeps all its terms there
(walk 0); elsewhere the rate 0 may be down to its newest term at the column ends, where the other two are not.  With any
table that walks in the end rows, or a bank with two rates of one sign, whole hypotheses are equal at the edges (each is
down to the cell itself) and "the device's index" is not defined there.
"""
import numpy as np

import integrate_crafted as IC

MAX_RATES = 16  # BLAH2HIP_MAX_RATES
SHARED = dict(nD=21, nC=111, K=1, W=4, H=1, n_cpi=6, seed=4242, q=(0.0, 1.0, -1.0))
MUTANTS = ("walk-sign", "age-from-oldest", "j-plus-r", "walk-j-alone", "floor", "wrap-rows", "wrap-cols", "drop-oldest")


def bound(n_surv, W):
    """The integrator's derived cell bound, relative: (n_surv W + 8) 2^-24."""
    return (n_surv * W + 8) * 2.0 ** -24


def alternating(nD, c=0.9):
    walk = c * np.where(np.arange(nD) % 2 == 0, 1.0, -1.0)
    walk[0] = walk[-1] = 0.0
    return walk


def tables(nD, nC):
    """{name: walk [nD]} -- the tables of the GPU cases."""
    j = np.arange(nD, dtype=np.float64)
    rng = np.random.default_rng(77)
    return {
        "zero": np.zeros(nD),
        "physical": np.linspace(1.95, -1.95, nD),  # configs[1]'s -1.95 cells per CPI at its highest Doppler, scaled to nD rows
        # shifts up to 7 x 9.3 = 65 cells at W = 8, 140 at W = 16: past the wave's 64 columns and the workgroup's strip
        "seams": np.where(j % 3 == 0, 9.3, np.where(j % 3 == 1, -9.3, 4.65)),
        "beyond": np.where(j % 2 == 0, 2.0, 3.0) * nC,  # every older term leaves the map: the cell's own CPI is left
        "jagged": rng.uniform(-3.0, 3.0, nD),
        "alternating": alternating(nD),
    }


def shared_input():
    """(maps complex64 [1, 6, 21, 111], walk, q) of the shared input."""
    s = SHARED
    return IC.maps(s["K"], s["n_cpi"], s["nD"], s["nC"], s["seed"]), alternating(s["nD"]), np.array(s["q"])


def closest_pair(sums):
    """The smallest |S_a - S_b| / max(S_a, S_b) over every output map, cell and pair of hypotheses of ``sums [K, ...]``."""
    worst = np.inf
    for a in range(sums.shape[0]):
        for b in range(a + 1, sums.shape[0]):
            worst = min(worst, float((np.abs(sums[a] - sums[b]) / np.maximum(sums[a], sums[b])).min()))
    return worst


def scalar_tables(walk, q, W, mutant=None):
    """(jr, s) int64 [K, W, nD] by a scalar loop over (k, a, j): blah2hip_nci_set_tracks' definition, or a wrong variant."""
    walk = np.asarray(walk, dtype=np.float64)
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    nD = walk.size
    rnd = np.floor if mutant == "floor" else np.rint
    jr = np.full((q.size, W, nD), -1, dtype=np.int64)
    s = np.zeros((q.size, W, nD), dtype=np.int64)
    for k in range(q.size):
        for a in range(W):
            r = int(rnd(q[k] * float(a)))
            for j in range(nD):
                src = j + r if mutant == "j-plus-r" else j - r
                if mutant == "wrap-rows":
                    src %= nD
                if not 0 <= src < nD:
                    continue
                mean2 = 2.0 * walk[j] if mutant == "walk-j-alone" else walk[j] + walk[src]
                sh = -0.5 * float(a) * mean2
                jr[k, a, j] = src
                s[k, a, j] = int(rnd(-sh if mutant == "walk-sign" else sh))
    return jr, s


def emulate(maps, walk, q, W, H=1, w=None, mutant=None):
    """The device's arithmetic in fp32 for a fresh integrator: nci_power's p, the window sums along the tracks added oldest
    first from +0, the first of the largest, sqrt(scale S).  Returns (out fp32 [n_out, nD, nC], index uint8)."""
    m = np.asarray(maps, dtype=np.complex64)
    K, n_cpi, nD, nC = m.shape
    wk = np.ones(K, dtype=np.float32) if w is None else np.asarray(w, dtype=np.float32)
    p, _ = IC._power(m.reshape(K, n_cpi, nD * nC), wk, 0, None)
    p = p.reshape(n_cpi, nD, nC)
    jr, s = scalar_tables(walk, q, W, mutant)
    scale = np.float32(1.0 / (W * wk.astype(np.float64).sum()))
    ends = [g for g in range(n_cpi) if g >= W - 1 and (g - (W - 1)) % H == 0]
    out = np.zeros((len(ends), nD, nC), dtype=np.float32)
    index = np.zeros((len(ends), nD, nC), dtype=np.uint8)
    d = np.arange(nC)
    ages = range(W - 2, -1, -1) if mutant == "drop-oldest" else range(W - 1, -1, -1)
    for o, g in enumerate(ends):
        best = None
        for k in range(jr.shape[0]):
            S = np.zeros((nD, nC), dtype=np.float32)
            for a in ages:
                col = d[None, :] + s[k, a][:, None]
                if mutant == "wrap-cols":
                    col = col % nC
                ok = (jr[k, a] >= 0)[:, None] & (col >= 0) & (col < nC)
                plane = p[g - (W - 1 - a) if mutant == "age-from-oldest" else g - a]
                v = plane[np.clip(jr[k, a], 0, nD - 1)[:, None], np.clip(col, 0, nC - 1)]
                S = (S + np.where(ok, v, np.float32(0))).astype(np.float32)
            if best is None:
                best = S
            else:
                win = S > best
                best = np.where(win, S, best)
                index[o][win] = k
        out[o] = np.sqrt((scale * best).astype(np.float32))
    return out, index


def named_error(out, index, sums, scale):
    """|out - sqrt(scale S_k)| / sqrt(scale S_k) per cell, k the hypothesis ``index`` names, against the fp64 ``sums``
    [K, n_out, nD, nC] of integrate_tracks; 0 where both are 0."""
    ref = np.sqrt(scale * np.take_along_axis(sums, index[None].astype(np.int64), axis=0)[0])
    err = np.abs(out.astype(np.float64) - ref)
    return np.where(ref > 0, err / np.where(ref > 0, ref, 1.0), np.where(err > 0, np.inf, 0.0)), ref


# ---- the scene: an echo that walks 2 cells and 1 row per CPI through W = 8 maps of noise --------------------------------
SCENE = dict(nD=21, nC=111, W=8, seed=3, walk=2.0, rate=1.0, q=(-2.0, -1.0, 0.0, 1.0, 2.0), row=14, col=60, snr=8.0)


def scene(seed=None):
    """(maps complex64 [1, 8, 21, 111], walk [21], q, (row, col) of the echo in the newest CPI, index of the true rate).
    Complex Gaussian noise of mean power 1 per cell; the echo a complex Gaussian of mean power 8 (9 dB per look) drawn per
    look, added at (row - a, col - 2 a) in the CPI of age a."""
    c = SCENE
    rng = np.random.default_rng(c["seed"] if seed is None else seed)
    W, nD, nC = c["W"], c["nD"], c["nC"]
    m = (rng.standard_normal((1, W, nD, nC)) + 1j * rng.standard_normal((1, W, nD, nC))) / np.sqrt(2.0)
    echo = np.sqrt(c["snr"] / 2.0) * (rng.standard_normal(W) + 1j * rng.standard_normal(W))
    for a in range(W):
        m[0, W - 1 - a, c["row"] - int(c["rate"]) * a, c["col"] - int(c["walk"]) * a] += echo[a]
    q = np.array(c["q"])
    return m.astype(np.complex64), np.full(nD, c["walk"]), q, (c["row"], c["col"]), int(np.nonzero(q == c["rate"])[0][0])
