"""Crafted maps, call schedules and a NumPy fp32 emulation for the non-coherent integrator (csrc/integrate_kernels.hpp
nci_kernel<W>, csrc/integrate.hip).  Helpers only, no tests; no GPU is touched at import.  The integrator has no reference
counterpart: everything here restates the project's own kernel.

``maps``: cell (k, c, i) of channel k, CPI c and cell i has the magnitude ``level(k, c) u`` with ``level = 1 + 0.25 ((3 k +
5 c) mod 7)`` and ``u`` uniform in [0.7, 1.4], drawn per (k, c, cell), under a uniform phase.  The kernel uses |M|^2 alone,
so it is ``u`` that tells the cells of a plane apart: a wrong cell, the two cells of a unit swapped, a plane read or a history
plane written one cell off, z0 stored for z1 -- each moves a cell by per cent, against a bound of (K W + 8) 2^-24.  ``level``
alone has period 7 in c and the same value in every cell.  The dynamic range of a sum's terms is (2.5 x 1.4 / 0.7)^2 = 25, so
the derived bound, which is relative to the sum, stays meaningful for every term.

``schedules``: the cuts of a stream into calls -- one call, calls of one CPI (every history plane moves on every call),
calls of max(W - 2, 1) CPIs (shorter than the history from W = 4 on: some planes move up, some are stored), and
``[1, W - 1, W, R + 1, rest]`` (a lone CPI, the window still filling, the first full call, one past a ring length).

``planted``: a scene for the metrics.  One cell per input CPI c, in every channel, carries ``PLANT_TOP x PLANT_RATIO^c``:
the largest term of the window that ends at g is the cell planted at CPI g - W + 1, the window's oldest, so the maximum moves
from one output map to the next, over the seams of the thread mapping (``seams``).

``emulate``: the kernel's walk in fp32 NumPy as the kernel does it -- the ring of R = nci_ring(W) slots, the history planes
with their move-up, groups of four CPIs, every window summed oldest first, |M|^2 and p by fused multiply-adds (evaluated in
fp64 and rounded once: the 48-bit product is exact there), the metrics per thread, wave (the butterfly), workgroup (two LDS
sets in turn) and map (metrics_kernel's tree).  It carries the CPI count of every ring slot and history plane, so that it
can say which windows a mutant touches: those whose summed CPIs are not g - W + 1 .. g, or hold a plane the mutant altered.

Measured on the MI355X (tests/test_integrate_crafted_gpu.py prints them; FIGURES): the cells' largest error / bound is 0.20
(W = 3) falling to 0.12 (W = 16), as in the emulation here; on the planted scenes noisePower lies within 1.9e-7 dB and
maxPower within 4.6e-6 dB of fp64 set_metrics of the device's own cells (half an fp32 ulp of a dB value of 37), against the
gate of 1e-3 dB.
"""
import numpy as np

GROUP = 4
MAX_WINDOW = 16
DB_TOL = 1e-3  # the project's gate for noisePower and maxPower, dB
PLANT_TOP, PLANT_RATIO = 1e4, 0.97
DB_FACTOR = np.float32(1.50514997831990597607)  # metrics_core.hpp db_of: 5 log10(2)

# Worst figures on the MI355X.  "cells": largest |out - ref| / bound per window W, odd geometry, K = 1, H = 1, one call.
# "metrics": largest |noisePower - n'| and |maxPower - m'| in dB on the planted scenes, per W.
FIGURES = {
    "cells": {1: 0.179, 2: 0.187, 3: 0.198, 4: 0.178, 5: 0.186, 6: 0.168, 7: 0.159, 8: 0.134, 9: 0.142, 10: 0.165, 11: 0.143,
              12: 0.136, 13: 0.128, 14: 0.134, 15: 0.134, 16: 0.120},
    "metrics": {1: (1.89e-07, 4.28e-06), 4: (1.78e-07, 4.52e-06), 9: (1.64e-07, 4.59e-06)},
}


def nci_ring(W):
    """integrate_kernels.hpp nci_ring: W - 1 older CPIs and a group of new ones, in whole groups."""
    return (W - 1 + GROUP + GROUP - 1) // GROUP * GROUP


def stream_length(W):
    """CPIs of the streams the tests cut: past two ring lengths with a window and a ragged group on top."""
    return 2 * nci_ring(W) + W + 3


def scene_length(W, K, max_batch=64):
    """CPIs of the planted scenes: the stream's length, or what one call of K channels may hold if that is less."""
    return min(stream_length(W), max_batch // K)


def level(K, n_cpi):
    k, c = np.arange(K)[:, None], np.arange(n_cpi)[None, :]
    return 1.0 + 0.25 * ((3 * k + 5 * c) % 7)


def maps(K, n_cpi, nD, nC, seed):
    """complex64 [K, n_cpi, nD, nC]: |M| = level(k, c) u, u uniform in [0.7, 1.4] per (k, c, cell), uniform phase."""
    rng = np.random.default_rng(seed)
    shape = (K, n_cpi, nD, nC)
    phase = rng.uniform(0, 1, shape)
    u = rng.uniform(0.7, 1.4, shape)
    z = (level(K, n_cpi)[:, :, None, None] * u) * np.exp(2j * np.pi * phase)
    return z.astype(np.complex64)


def schedules(W, N):
    """{name: [CPIs per call]} -- every list adds up to N."""
    R = nci_ring(W)

    def chunks(n):
        return [n] * (N // n) + ([N % n] if N % n else [])

    mixed, left = [], N
    for n in (1, W - 1, W, R + 1):
        n = min(n, left)
        if n > 0:
            mixed.append(n)
            left -= n
    if left:
        mixed.append(left)
    out = {"one-call": [N], "one-cpi": [1] * N, "short": chunks(max(W - 2, 1)), "mixed": mixed}
    assert all(sum(v) == N and min(v) > 0 for v in out.values())
    return out


def clipped(cuts, limit):
    """The same cuts with every call longer than ``limit`` CPIs split into calls of ``limit`` and a rest."""
    out = []
    for n in cuts:
        while n > limit:
            out.append(limit)
            n -= limit
        out.append(n)
    return out


def seams(nD, nC):
    """Cell indices where the thread mapping has a seam: a thread owns cells 2u and 2u + 1, a wave 128 cells, a workgroup
    512; the last cell of an odd map is a unit of one cell."""
    cells = nD * nC
    G = ((cells + 1) // 2 + 255) // 256
    return [0, 1, 126, 127, 128, 510, 511, 512, 512 * (G - 1), cells - 1]


def planted(K, n_cpi, nD, nC, seed):
    """(maps with one planted cell per CPI, in every channel; the cell index per CPI).  The planted magnitude descends with
    the CPI, the positions go round ``seams``: no window of up to ten CPIs holds a position twice."""
    m = maps(K, n_cpi, nD, nC, seed)
    pos = seams(nD, nC)
    assert len(set(pos)) == len(pos) and max(pos) < nD * nC
    at = [pos[c % len(pos)] for c in range(n_cpi)]
    flat = m.reshape(K, n_cpi, nD * nC)
    for c, i in enumerate(at):
        z = flat[:, c, i].astype(np.complex128)
        flat[:, c, i] = (z / np.abs(z) * (PLANT_TOP * PLANT_RATIO ** c)).astype(np.complex64)
    return m, at


def set_metrics64(z):
    """Map::set_metrics (Map.cpp:187-206) in fp64: (noisePower, maxPower) of one map."""
    with np.errstate(divide="ignore"):
        db = 10.0 * np.log10(np.abs(np.asarray(z).astype(np.complex128)))
    noise = db.mean()
    return noise, max(0.0, db.max()) - noise


# ---- the walk: what a call does, from the counters alone ------------------------------------------------------------------
def plan(W, H, cuts):
    """One dict per call of an integrator that starts at count 0: ``g0``, ``n_cpi``, ``n_out``, ``first`` (as
    blah2hip_nci_count reports them), ``hist_valid``, ``stay`` (nci_kernel's: W - n_cpi, or 0) and ``groups``: per group of
    four CPIs the windows that end in it as (c in the call, newest slot, oldest slot)."""
    R, g, calls = nci_ring(W), 0, []
    for n in cuts:
        w1 = W - 1
        f = w1 if g <= w1 else w1 + (g - w1 + H - 1) // H * H
        n_out = (g + n - 1 - f) // H + 1 if f < g + n else 0
        nxt, hop = (f - g if n_out else n), min(H, n)
        groups = []
        for c0 in range(0, n, GROUP):
            wins = []
            for c in range(c0, min(c0 + GROUP, n)):
                if c == nxt:
                    wins.append((c, c % R, (c % R + R - W + 1) % R))
                    nxt += hop
            groups.append(wins)
        assert sum(len(v) for v in groups) == n_out
        calls.append({"g0": g, "n_cpi": n, "n_out": n_out, "first": f, "hist_valid": min(g, w1), "stay": max(W - n, 0),
                      "groups": groups})
        g += n
    return calls


# ---- the emulation ----------------------------------------------------------------------------------------------------------
CELL_MUTANTS = ("swap", "shift8", "stale-slot", "hist-reversed", "no-moveup", "hist-off-one", "dropped-channel", "wrong-weights")
METRIC_MUTANTS = ("lost", "twice", "wave-max-0", "wave-max-1", "wave-max-2", "wave-max-3", "max-carried", "absent-cell")


def _fma(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 is exact in fp64; one rounding of the sum to fp64, one to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _power(m, w, in_off, mutant):
    """p [n, cells] fp32 of a call's maps m [K, n, cells]: |M|^2 = fma(re, re, im im), p = fma(w_k, |M_k|^2, p) from 0 in
    the order k = 0 .. K - 1.  Returns (p, the CPIs of the call whose planes the mutant altered)."""
    K, n, cells = m.shape
    p = np.zeros((n, cells), dtype=np.float32)
    altered = set()
    if mutant == "wrong-weights":
        altered = set(range(n)) if not np.array_equal(w, np.roll(w, 1)) else set()
        w = np.roll(w, 1)
    for k in range(K):
        if mutant == "dropped-channel" and k == K - 1:
            altered = set(range(n))
            continue
        plane = m[k]
        if mutant == "shift8":  # the planes that start 8 bytes off a 16-byte boundary read one cell further
            off = (in_off + (k * n + np.arange(n)) * cells * 8) % 16 == 8
            plane = np.where(off[:, None], np.roll(plane, -1, axis=1), plane)
            altered |= set(np.nonzero(off)[0].tolist())
        re, im = plane.real.astype(np.float32), plane.imag.astype(np.float32)
        p = _fma(np.full_like(re, w[k]), _fma(re, re, im * im), p)
    return p, altered


def _butterfly(v):
    """metrics_core.hpp wave_sum_max's sum over the last axis (64 lanes): lane 0's result."""
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ off]
    return v[..., 0]


def _metrics(z, lds, st, t, mutant, plant):
    """The epilogue of one window: z [cells] fp32 as written -> (noisePower, maxPower).  ``lds``: wmax [2][GROUP][G][4] of
    the call, ``st`` its current set."""
    cells = z.size
    units = (cells + 1) // 2
    G = (units + 255) // 256
    assert G <= 256
    with np.errstate(divide="ignore"):
        db = DB_FACTOR * np.log2(z * z + np.float32(0.0) * np.float32(0.0))
    assert db.dtype == np.float32
    d = np.zeros(G * 512, dtype=np.float32)
    live = np.zeros(G * 512, dtype=bool)
    d[:cells] = db
    live[:cells] = True
    if mutant == "lost" and plant is not None:
        live[plant] = False
    d64 = np.where(live, d.astype(np.float64), 0.0)
    if mutant == "twice" and plant is not None:
        d64[plant] *= 2.0
    if mutant == "absent-cell" and cells % 2:  # the single-cell unit's second cell: a copy of its first
        d64[cells] = d64[cells - 1]
    lsum = d64[0::2] + d64[1::2]
    dm = np.where(live, d, np.float32(0.0))
    lmax = np.fmax(np.float32(0.0), np.fmax(dm[0::2], dm[1::2]))
    wsum = _butterfly(lsum.reshape(G, 4, 64))
    wmax = lmax.reshape(G, 4, 64).max(axis=2)
    stale = lds[st ^ 1][t].copy()
    lds[st][t] = wmax
    psum = np.zeros(G)
    pmax = np.zeros(G, dtype=np.float32)  # Map.cpp:193: the running max starts at 0
    for wv in range(4):
        psum = psum + wsum[:, wv]
        if mutant == f"wave-max-{wv}":
            continue
        pmax = np.fmax(pmax, wmax[:, wv])
        if mutant == "max-carried":
            pmax = np.fmax(pmax, stale[:, wv])
    # metrics_kernel: thread i holds partial i (G <= 256), then the tree over 256 slots
    ssum, smax = np.zeros(256), np.zeros(256, dtype=np.float32)
    ssum[:G], smax[:G] = 0.0 + psum, np.fmax(np.float32(0.0), pmax)
    off = 128
    while off:
        ssum[:off] = ssum[:off] + ssum[off:2 * off]
        smax[:off] = np.fmax(smax[:off], smax[off:2 * off])
        off //= 2
    with np.errstate(invalid="ignore"):
        noise = ssum[0] / float(cells)
        return noise, float(smax[0]) - noise


def emulate(m, W, H, cuts, w=None, mutant=None, in_off=0, plants=None, metrics=True):
    """nci_kernel<W> over the stream m [K, N, nD, nC] cut into the calls ``cuts``.  ``plants``: the planted cell per CPI, for
    the metrics mutants.  Returns {'out' fp32 [n_out, cells], 'met' fp64 [n_out, 2], 'ends', 'calls' [(n_out, first)],
    'touched' bool [n_out]}."""
    assert mutant is None or mutant in CELL_MUTANTS + METRIC_MUTANTS
    K, N = m.shape[:2]
    cells = m.shape[2] * m.shape[3]
    m = m.reshape(K, N, cells)
    R = nci_ring(W)
    wk = np.ones(K, dtype=np.float32) if w is None else np.asarray(w, dtype=np.float32)
    scale = np.float32(1.0 / (W * wk.astype(np.float64).sum()))
    G = ((cells + 1) // 2 + 255) // 256
    hist = np.zeros((max(W - 1, 0), cells), dtype=np.float32)
    hist_id = [None] * max(W - 1, 0)  # the CPI count a plane holds
    altered = set()  # CPI counts whose p the mutant altered
    out, met, ends, reports, touched = [], [], [], [], []
    assert sum(cuts) == N
    for call in plan(W, H, cuts):
        g0, n, stay, hist_valid = call["g0"], call["n_cpi"], call["stay"], call["hist_valid"]
        ring = np.zeros((R, cells), dtype=np.float32)
        ring_id = [None] * R
        # history plane i: the CPI W - i in front of the call, slot R - W + i; the planes that stay move up by n
        hq = 0
        for i in range(1, W):
            if W - i <= hist_valid:
                src = W - i if mutant == "hist-reversed" else i
                ring[R - W + i], ring_id[R - W + i] = hist[src - 1].copy(), hist_id[src - 1]
                if W - i < stay and mutant != "no-moveup":
                    hist[hq], hist_id[hq] = ring[R - W + i].copy(), ring_id[R - W + i]
            if W - i < stay:
                hq += 1
        hst = (W - 1 - n if W - 1 > n else 0) + (1 if mutant == "hist-off-one" else 0)
        p, alt = _power(m[:, g0:g0 + n], wk, in_off, mutant)
        altered |= {g0 + c for c in alt}
        lds = np.zeros((2, GROUP, G, 4), dtype=np.float32)
        st = 0
        wins = {c: (new, old) for grp in call["groups"] for c, new, old in grp}
        for c0 in range(0, n, GROUP):
            any_win = False
            for t in range(min(GROUP, n - c0)):
                c = c0 + t
                slot = c % R
                before, before_id = ring[slot].copy(), ring_id[slot]
                ring[slot], ring_id[slot] = p[c], g0 + c
                if W > 1 and c + W > n:  # one of the call's last W - 1 CPIs: into the history
                    if hst < W - 1:
                        hist[hst], hist_id[hst] = p[c].copy(), g0 + c
                    hst += 1
                if c not in wins:
                    continue
                new, old = wins[c]
                assert new == slot
                order = [(slot + R - q) % R for q in range(W - 1, -1, -1)]
                assert order[0] == old
                terms = [ring[s_] for s_ in order]
                ids = [ring_id[s_] for s_ in order]
                if mutant == "stale-slot":  # the newest term read before the walk wrote it
                    terms[-1], ids[-1] = before, before_id
                s = terms[0].copy()
                for term in terms[1:]:
                    s = s + term
                assert s.dtype == np.float32
                z = np.sqrt(scale * s)
                if mutant == "swap":
                    pairs = cells // 2
                    z[:2 * pairs] = z[:2 * pairs].reshape(pairs, 2)[:, ::-1].reshape(-1)
                g = g0 + c
                # touched: the CPIs summed are not the window's (in any order), or one of them is a plane the mutant altered
                touched.append(sorted(-1 if i is None else i for i in ids) != list(range(g - W + 1, g + 1))
                               or bool(altered & set(ids)) or mutant == "swap")
                out.append(z)
                ends.append(g)
                if metrics:
                    plant = plants[g - W + 1] if plants is not None else None
                    met.append(_metrics(z, lds, st, t, mutant, plant))
                any_win = True
            if any_win:
                st ^= 1
        reports.append((call["n_out"], call["first"]))
    return {"out": np.stack(out) if out else np.zeros((0, cells), dtype=np.float32),
            "met": np.array(met, dtype=np.float64).reshape(-1, 2), "ends": ends, "calls": reports,
            "touched": np.array(touched, dtype=bool)}
