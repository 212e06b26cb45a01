"""Crafted pulses for the clutter filter's FFT correlations (clutter_corr_kernel, clutter_corr_half_kernel): a sparse PAIR
CENSUS for the circular correlations

    r[k]   = sum_n xs[(n + k) mod N] conj(xs[n]),      b_c[k] = sum_n y_c[(n + k) mod N] conj(xs[n]),      0 <= k < nBins,

xs the shifted reference as oracle.blah2_oracle.wiener_hopf forms it (the uint32 evaluation for delayMin > 0 included).

Used by tests/test_corr_crafted_model.py (CPU: fp64 models of both kernel forms, the mutants) and
tests/test_corr_crafted_gpu.py.  Here: the geometries, the restatement of the plan and of the two segment walks
(seg_walk / half.per of csrc/clutter_kernels.hpp), the census, its exact references (the oracle, and a direct sum over impulse pairs)
and the device planes.  No GPU is touched at import.

The census.  A `place` is an EARLIER sample n (an index of xs).  A full place plants xs at n, n + 1, n + nBins - 1 and every
y_c at n, n + 1, n + nBins - 1 and at one lag of its own, n + 2 + c (all mod N): products at lags 0, 1, nBins - 2, nBins - 1
in r and in every b_c, the y impulses of a place that lie in front of one of its x impulses (they must reach no lag), and per
channel an impulse no other channel has.  Values are Gaussian integers with |re|, |im| <= 127 and moduli in [75, 170], all
distinct over a census, so exact as int8 planes, int16 words and fp32 planes.  The places of a geometry are dealt out over
its CPIs: every CPI differs and none holds more than 48 impulses in xs or 65 in a y_c; the least planted product is 8.1e-3
of its normaliser (the model file asserts 1e-3, a hundred gates, for what is actually planted)."""
from collections import namedtuple

import numpy as np

from oracle import blah2_oracle as O

R_TOL = B_TOL = 1e-5  # tests/clutter_crafted.py, and the range and FIR census gates
IN_GAP = 37           # input stride N + 37
FILL = 77             # the gaps between CPIs and the rows around the planes, in every format
MAX_SURV = 4
GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces

# form: the correlation form forced on the handle; grids: forced grids, 0 = the planner's; carry: the plan that shares
# seg_len = F/2 with the FIR; walk: the least number of segments some workgroup must walk at the FIRST grid
Geom = namedtuple("Geom", "name form F n_bins dmin N grids carry B walk")


def _geoms():
    out = []
    # half-window, 33 taps: 40 segments on 8 workgroups are runs of per = 5 with carried prevX and 7 run fronts, the last
    # segment has 3 samples; 40 L + 3 samples are 41 segments: per = 6, the last run is short, workgroup 7 has the wrap alone.
    # L + 1 taps: the maximal lag nBins - 1 = L across every seam, tau = L, the last segment is full, workgroup 7 is empty
    for F, d1, d2, d3 in ((1024, -7, 5, 0), (2048, 0, -7, 5), (4096, 5, 0, -7)):
        L = F // 2
        big = 2 if F == 4096 else 3
        out.append(Geom(f"half{F}_33taps_39L3", "half", F, 33, d1, 39 * L + 3, (8, 0), False, 3, 5))
        out.append(Geom(f"half{F}_33taps_40L3", "half", F, 33, d2, 40 * L + 3, (8, 0), False, 3, 6))
        out.append(Geom(f"half{F}_tauL_41L", "half", F, L + 1, d3, 41 * L, (8, 0), False, big, 6))
    # one or two segments: nearly everything is in the wrap product
    out.append(Geom("half1024_33taps_L1", "half", 1024, 33, -7, 513, (0,), False, 2, 0))
    out.append(Geom("half1024_33taps_short", "half", 1024, 33, 5, 100, (0,), False, 2, 0))
    # windowed: 10 segments (XCDs 5 ... 7 have none), 40 and 43 segments on 8 and 16 workgroups (step 1 and 2)
    for F, nb, d1, d2, d3 in ((1024, 110, 5, -7, 0), (2048, 410, -7, 0, 5), (4096, 2100, 0, 5, None)):
        S = F - nb + 1
        big = 2 if F == 4096 else 3
        if d3 is not None:
            out.append(Geom(f"win{F}_{nb}taps_10seg", "window", F, nb, d3, 9 * S + 2, (8, 0), False, big, 0))
        out.append(Geom(f"win{F}_{nb}taps_40seg", "window", F, nb, d1, 39 * S + 3, (8, 16), False, big, 5))
        out.append(Geom(f"win{F}_{nb}taps_43seg", "window", F, nb, d2, 42 * S + 1, (8, 16), False, big, 6))
    out.append(Geom("win4096_2047taps_carry", "window", 4096, 2047, -7, 12 * 2048 + 5, (8, 0), True, 2, 0))
    out.append(Geom("win1024_100taps_n300", "window", 1024, 100, -7, 300, (0,), False, 2, 0))  # 2N - 1 < F: wrapWin's clamp
    return out


GEOMS = _geoms()
BY_NAME = {g.name: g for g in GEOMS}
# the planner's own path: BATCH_CPIS CPIs per launch (three census CPIs and a fourth that fills the batch), 100 half-window
# segments each; on 256 CUs clutter_grids leaves 32 workgroups per CPI, runs of 4 segments: the census is built for those
BATCH_CPIS = 64
BATCH_GEOM = Geom("half1024_33taps_batch64", "half", 1024, 33, -7, 99 * 512 + 7, (0,), False, 4, 0)
CENSUS_GRID = {BATCH_GEOM.name: 32}


# ---- the plan and the walks, restated (csrc/clutter.hip: clutter_plan, clutter_grids, corr_args; clutter_kernels.hpp: seg_walk)
def up8(v):
    return max(8, (v + 7) & ~7)


def cdiv(a, b):
    return -(-a // b)


def seg_len_of(g):
    return g.F // 2 if g.carry else g.F - g.n_bins + 1


def plan_jobs(g, num_cu):
    """nJobs of the plan: the workgroups per CPI of a lone CPI, and the upper bound of a forced grid."""
    return up8(min(cdiv(g.N, seg_len_of(g)), 2 * num_cu))


def planner_grid(g, num_cu, n_cpi):
    """clutter_grids: two resident generations (4 workgroups per CU) over the launch's CPIs."""
    return min(plan_jobs(g, num_cu), up8(cdiv(8 * num_cu, n_cpi)))


def window_walks(n_seg, grid):
    """seg_walk: per workgroup the segments it takes, in order.  XCD x = workgroup & 7 owns the eighth
    [x s8, x s8 + count); its grid / 8 workgroups take every (grid / 8)-th segment of it."""
    assert grid % 8 == 0 and grid >= 8
    s8, gx = cdiv(n_seg, 8), grid // 8
    walks = []
    for wg in range(grid):
        xcd, first = wg & 7, wg >> 3
        base = xcd * s8
        count = min(s8, n_seg - base)  # <= 0 for the last XCDs of a short CPI
        walks.append([base + r for r in range(first, max(count, 0), gx)])
    return walks


def half_walks(N, F, grid):
    """clutter_corr_half_kernel: runs of per segments of L = F/2 samples; the LAST workgroup also does the wrap product."""
    L = F // 2
    n_seg = cdiv(N, L)
    per = cdiv(n_seg, grid)
    return per, [list(range(j * per, min((j + 1) * per, n_seg))) for j in range(grid)]


def walks_of(g, grid):
    if g.form == "half":
        return half_walks(g.N, g.F, grid)[1]
    return window_walks(cdiv(g.N, seg_len_of(g)), grid)


def xs_indices(N, dmin, off_by_one=False):
    """xs_index / xs_map of csrc/clutter_kernels.hpp: xs[i] = x[j[i]], without a division.  off_by_one: the mutant whose branch
    changes at thresh + 1."""
    thresh = max(dmin, 0)
    wrap_c = ((1 << 32) - thresh) % N
    i = np.arange(N, dtype=np.int64)
    j = np.where(i >= thresh + (1 if off_by_one else 0), i - dmin, i + wrap_c)
    return np.where(j >= N, j - N, j)


def oracle_indices(N, dmin):
    """oracle.blah2_oracle.wiener_hopf's own line: (i - delayMin) in uint32, then mod N."""
    i = np.arange(N, dtype=np.uint64)
    return (((i - np.uint64(dmin & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)) % np.uint64(N)).astype(np.int64)


# ---- the census -----------------------------------------------------------------------------------------------------------
def places_of(g, grid):
    """[(n, kind)]: kind 'full' (see the module docstring), 'x' / 'y' (one impulse in xs / in every y_c: the sentinels)."""
    N, nb, F = g.N, g.n_bins, g.F
    tau = nb - 1
    P = []

    def full(n):
        if 0 <= n < N:
            P.append((n, "full"))

    if g.form == "window":
        S = seg_len_of(g)
        n_seg, walks = cdiv(N, S), window_walks(cdiv(N, S), grid)
        s8 = cdiv(n_seg, 8)
        longest = max(walks, key=len)
        gs = {1, n_seg - 1} | set(longest[1:3]) | {j * s8 for j in range(1, 8)}
        for s in sorted(gs):
            if 0 < s < n_seg:
                full(s * S - 1)  # the pair across the seam belongs to segment s - 1, its later samples lie in window s - 1's tail
                full(s * S)
        inner = longest[1] if len(longest) > 1 else 0
        full(inner * S + S - 1)  # with lag nBins - 1 the later sample is the window's last, inner S + F - 1 (carry plan: F - 3)
        full(N - nb)             # the later sample at exactly N - 1
    else:
        L = F // 2
        per, runs = half_walks(N, F, grid)
        n_seg = cdiv(N, L)
        busy = [r for r in runs if r]
        fronts = [r[0] for r in busy[1:]]
        gs = set()
        if fronts:
            gs |= {fronts[0], fronts[len(fronts) // 2], fronts[-1]}
        for r in (busy[0], busy[len(busy) // 2], busy[-1]):  # run interiors: prevX carried
            gs |= set(r[1:2]) | set(r[-1:])
        gs.add(n_seg - 1)
        for s in sorted(gs):
            if 0 < s < n_seg:
                for n in (s * L - 1, s * L - tau, s * L + 1 - tau, s * L):  # later sample at s L and s L + 1, earlier in s - 1
                    full(n)
        full((n_seg // 2) * L + 5)  # both samples in one segment (33 taps)
        full(N - tau)               # (N - tau -> 0)
        P.append(((N - tau - 1) % N, "x"))  # at distance nBins from sample 0: must reach no kept lag
    full(0)
    full(N - 1)  # later samples wrapped to 0 and to tau - 1
    full(N - 2)  # later sample at exactly N - 1 and, wrapped, at tau - 2
    if g.dmin > 0:
        full(g.dmin - 1)
        full(g.dmin)
    # sentinels in the middle of the CPI: a lone x impulse, a y impulse 3 samples in front of it, a pair at distance nBins
    mid = (N // 2 + 11) % N
    P += [(mid, "x"), ((mid - 3) % N, "y"), ((mid + 3 * nb) % N, "x"), ((mid + 4 * nb) % N, "x"), ((mid + 4 * nb) % N, "y")]
    seen, out = set(), []
    for p in P:
        if p not in seen:
            seen.add(p)
            out.append(p)
    return out


def _value_pool(seed):
    re, im = np.meshgrid(np.arange(-127, 128), np.arange(-127, 128))
    m = np.hypot(re, im)
    keep = (m >= 75) & (m <= 170)
    v = (re[keep] + 1j * im[keep]).astype(np.complex128)
    np.random.default_rng(seed).shuffle(v)
    return v


Census = namedtuple("Census", "g grid x ys planted")  # x [B][N], ys [B][MAX_SURV][N] complex128; planted: [(cpi, n, k)]

_census = {}


def census_for(g):
    """The census of a geometry, built for its FIRST grid (the seams of that grid's walks) and used at every grid."""
    if g.name in _census:
        return _census[g.name]
    grid = CENSUS_GRID.get(g.name) or g.grids[0] or 8
    N, nb = g.N, g.n_bins
    pool = iter(_value_pool(sum(map(ord, g.name))))
    idx = oracle_indices(N, g.dmin)
    x = np.zeros((g.B, N), dtype=np.complex128)
    ys = np.zeros((g.B, MAX_SURV, N), dtype=np.complex128)
    planted = []
    lags = sorted({0, 1 % nb, nb - 1})
    for i, (n, kind) in enumerate(places_of(g, grid)):
        c = i % g.B
        xpos = [(n + k) % N for k in lags] if kind == "full" else ([n] if kind == "x" else [])
        ypos = [(n + k) % N for k in lags] if kind == "full" else ([n] if kind == "y" else [])
        for p in xpos:
            if x[c, idx[p]] == 0:
                x[c, idx[p]] = next(pool)
        for ch in range(MAX_SURV):
            own = [(n + 2 + ch) % N] if kind == "full" and nb > 2 + ch else []
            for p in ypos + own:
                if ys[c, ch, p] == 0:
                    ys[c, ch, p] = next(pool)
        if kind == "full":
            planted += [(c, n, k) for k in lags]
    for c in range(g.B):  # positive delayMin: two xs samples may read one x sample; every planted xs sample must still be there
        assert all(x[c, idx[n]] != 0 for cc, n, _ in planted if cc == c)
    _census[g.name] = Census(g, grid, x, ys, planted)
    return _census[g.name]


def direct_sums(x, y, dmin, n_bins):
    """r and b of one CPI and channel as plain sums over the impulse pairs, fp64 (exact: integers below 2^53)."""
    N = x.shape[0]
    xs = x[oracle_indices(N, dmin)]
    px = np.flatnonzero(xs)
    r = np.zeros(n_bins, dtype=np.complex128)
    b = np.zeros(n_bins, dtype=np.complex128)
    for later, out in ((xs, r), (y, b)):
        pl = np.flatnonzero(later)
        k = (pl[:, None] - px[None, :]) % N
        v = later[pl][:, None] * np.conj(xs[px])[None, :]
        keep = k < n_bins
        np.add.at(out, k[keep], v[keep])
    return r, b


_refs = {}


def oracle_rb(g, c, ch):
    """(r, b) of CPI c, channel ch by the oracle: the lines of oracle.blah2_oracle.wiener_hopf that form its normal
    equations (wiener_hopf_normal_equations; the model file asserts that return_filter=True gives the same bits), without
    a Cholesky factorisation of up to 2100 x 2100 per CPI and channel.  Computed once per process and left unchanged."""
    key = (g.name, c, ch)
    if key not in _refs:
        cs = census_for(g)
        _, r, b = O.wiener_hopf_normal_equations(cs.x[c], cs.ys[c, ch], g.dmin, g.dmin + g.n_bins)
        r.setflags(write=False)
        b.setflags(write=False)
        _refs[key] = (r, b)
    return _refs[key]


def normalisers(g, c, ch):
    """(r_ref[0], sqrt(r_ref[0] sum |y_c|^2)): the second is the Cauchy-Schwarz bound of every |b[k]|."""
    cs = census_for(g)
    r0 = float(np.sum(np.abs(cs.x[c][oracle_indices(g.N, g.dmin)]) ** 2))
    return r0, float(np.sqrt(r0 * np.sum(np.abs(cs.ys[c, ch]) ** 2)))


# ---- device planes ----------------------------------------------------------------------------------------------------------
def host_planes(fmt_name, x, ys):
    """Host arrays for format fmt_name: rows of N + IN_GAP samples, one row of filler in front of the first CPI and one behind
    the last, FILL everywhere outside the CPIs.  Returns ([arrays], row offset in array elements of the first CPI per array):
    FMT_I16: one array [B + 2, stride, 4] int16 (x and ys[0] interleaved); else one plane for x and one per channel."""
    B, N = x.shape
    stride = N + IN_GAP
    if fmt_name == "FMT_I16":
        h = np.full((B + 2, stride, 4), FILL, dtype=np.int16)
        h[1:B + 1, :N] = np.stack([x.real, x.imag, ys[:, 0].real, ys[:, 0].imag], axis=-1)
        return [h], stride
    planes = []
    for v in [x] + [ys[:, k] for k in range(ys.shape[1])]:
        if fmt_name == "FMT_I8":
            h = np.full((B + 2, stride, 2), FILL, dtype=np.int8)
            h[1:B + 1, :N] = np.stack([v.real, v.imag], axis=-1)
        else:
            h = np.full((B + 2, stride), FILL + 1j * FILL, dtype=np.complex64)
            h[1:B + 1, :N] = v
        planes.append(h)
    return planes, stride
