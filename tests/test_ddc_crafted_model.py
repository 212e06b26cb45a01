"""CPU: the crafted taps and streams of tests/ddc_crafted.py for the digital down-converter, checked without a device.

  * the case table launches every plan class of ddc_plan (seven over 1 <= D <= 64, 1 <= T <= 1024; the tiles below 64 are
    one class and the table holds the least tile, 51), the Python plan reads as csrc/ddc_kernels.hpp's does;
  * Model (the fp64 restatement of calls, rows, tiles, segments and the carried history) equals blah2_amd.ddc;
  * the conditions the GPU file rests on: census A has at most one term per output, meets every tap, and has terms in
    tiles and rows beyond the first; census B has outputs that read the history and outputs that read across a row edge;
    census C plants nothing below 1e-3 of the largest quantity of its check;
  * THE GAP AS MEASURED: with the designed taps under noise, the taps that can be dropped one at a time without any output
    leaving the contract's bound -- printed for T = 1024 at D = 1, 4, 16, 24 and for (64, 193), asserted above zero; with
    census C's taps none can;
  * the sensitivity proof: each wrong restatement (Model's faults) moves a checked output of a crafted case by more than
    1000 times that output's bound, and moves nothing where its term does not exist;
  * the single-term bound, below, against an fp32 emulation of the kernel's chain for one term.

The single-term bound.  The header's budget per output, in units of 2^-24 sum_t |g[t]| |u[m D - t]|, is: the two chains of
2 T multiply-adds per component, 2 T sqrt 2; the rounded phasor, 0.71; its fp32 complex product, 2; the fp64 phase, nothing
below m = 2^45.  Where one term alone is not zero, every other multiply-add of the chain adds an exact zero to the sum (and
the segments' partial sums add zeros), so the chain's share is that of the ONE complex product: each component is
fma(-g.y, u.y, fl(g.x u.x)) or its like, two roundings of quantities no larger than |g| |u|, over two components 2 sqrt 2.
With the phasor's 0.71 and its product's 2 the total is 2.83 + 2.71 = 5.54 < 8:

    |v_dev - p g[t] a| <= 8 2^-24 |g[t]| |a|,

the contract with its chain term 3 T replaced by 3 (T = 1 gives 3 + 8 = 11 there; this is tighter and derived the same way).
An output none of whose samples is non-zero is a sum of zeros times a phasor: exactly zero.
"""
import math
import os

import numpy as np
import pytest

import ddc_crafted as K
from conftest import ROOT


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    return blah2_amd


def taps_of(b2, h, offsets):
    """g_c as the library rounds them (fp32 of ddc_taps)."""
    return np.stack([b2.ddc_taps(h, f, K.FS).astype(np.complex64) for f in offsets])


# ------------------------------------------------------------------------------------------------------------------ table
def test_the_case_table_launches_every_plan_class():
    every = {K.plan_class(K.plan(D, T)) for D in range(1, K.MAX_D + 1) for T in range(1, K.MAX_T + 1)}
    assert every == set(K.CLASSES) and len(every) == 7
    by_class = {}
    for c in K.CASES:
        by_class.setdefault(K.plan_class(K.plan(c.D, c.T)), []).append(c)
    assert set(by_class) == every
    for k in K.CLASSES:
        cs = by_class[k]
        print(f"class (tile, threads, TR, R, G) = {k}: " + ", ".join(f"{K.case_id(c)} (tile {K.plan(c.D, c.T).tile})" for c in cs))
        assert len({(c.D, c.T) for c in cs}) >= 2
        assert max(c.T for c in cs) >= 1000
        assert {c.C for c in cs} == {1, 2, 3, 8}
    tiles = [K.plan(c.D, c.T).tile for c in K.CASES]
    assert min(tiles) == 51 == min(K.plan(D, T).tile for D in range(1, K.MAX_D + 1) for T in range(1, K.MAX_T + 1))
    Ds = {c.D for c in K.CASES}
    assert {3, 5, 24, 26, 33, 63} <= Ds and Ds & {7, 9}
    seg = [c for c in K.CASES if K.plan(c.D, c.T).G > 1]
    assert {c.fmt for c in seg} >= {"I16", "I8"}
    assert any(c.C == 8 for c in seg if K.plan(c.D, c.T).G == 2) and any(c.C == 8 for c in seg if K.plan(c.D, c.T).G == 4)
    assert [K.plan_class(K.plan(c.D, c.T)) for c in K.class_cases()] == list(K.CLASSES)


def test_the_plan_is_the_kernels():
    """The restatement was written from ddc_plan and the kernel's segment bounds as they read here; the issue's examples."""
    src = open(os.path.join(ROOT, "blah2_amd", "csrc", "ddc_kernels.hpp")).read()
    for line in ("constexpr int DDC_LDS_SAMPLES = 5120;", "constexpr int DDC_PART_SAMPLES = 768;",
                 "const uint32_t lead = (T - 1 + D - 1) / D;", "uint32_t fit = DDC_LDS_SAMPLES / D - lead - 1;",
                 "p.tile = fit >= 1024 ? 1024 : fit >= 512 ? 512 : fit >= 256 ? 256 : 192;",
                 "while (p.tile > 256 && (uint64_t)(T - 1) * 16 <= (uint64_t)(p.tile / 2) * D) p.tile /= 2;",
                 "fit = (DDC_LDS_SAMPLES - DDC_PART_SAMPLES) / D - lead - 1;", "p.tile = fit >= 128 ? 128 : fit >= 64 ? 64 : fit;",
                 "p.TR = p.tile > 64 ? 128 : 64;", "p.Lp = (p.tile + lead) | 1;",
                 "const uint32_t Tseg = (T + G - 1) / G, s0 = min(T, seg * Tseg), s1 = min(T, s0 + Tseg);"):
        assert line in src, line
    want = {(16, 1024): (192, 192, 192, 1, 1), (26, 79): (192, 192, 192, 1, 1), (24, 1024): (128, 256, 128, 1, 2),
            (33, 67): (128, 256, 128, 1, 2), (32, 1024): (64, 256, 64, 1, 4), (64, 193): (64, 256, 64, 1, 4),
            (64, 512): (59, 256, 64, 1, 4), (64, 1024): (51, 256, 64, 1, 4), (4, 17): (256, 256, 256, 1, 1),
            (1, 1024): (1024, 256, 256, 4, 1), (4, 1024): (512, 256, 256, 2, 1), (50, 800): (64, 256, 64, 1, 4)}
    for (D, T), w in want.items():
        p = K.plan(D, T)
        assert (p.tile, p.threads, p.TR, p.R, p.G) == w, (D, T)
    for D in range(1, K.MAX_D + 1):
        for T in (1, 2, D, 255, 256, 257, 1023, 1024):
            p = K.plan(D, T)
            lds = D * p.Lp + (K.PART_SAMPLES if p.G > 1 else 0)
            assert lds <= K.LDS_SAMPLES and p.tile >= 1 and p.segs[0][0] == 0 and p.segs[-1][1] == T
            assert all(a[1] == b[0] for a, b in zip(p.segs, p.segs[1:]))
            assert p.G == 1 or 4 * 4 * (p.G - 1) * p.TR <= 4 * K.PART_SAMPLES  # [G - 1][4 R CB][TR] floats at CB = 4


@pytest.mark.parametrize("D, T, gap", [(33, 67, 5), (4, 40, 0), (64, 193, 3)])
def test_the_model_is_the_restatement(b2, D, T, gap):
    """Without a fault, whatever the delivery: blah2_amd.ddc of the whole stream, and its sum S."""
    rng = np.random.default_rng(D + T)
    offsets = K.OFFSETS[3]
    g = taps_of(b2, K.comparable_taps(T), offsets)
    tile = K.plan(D, T).tile
    n_a = (tile + 9) * D
    cuts = [(n_a, 2), (D, 1), (D, 3), (n_a, 1), (2 * D, 2)]
    u = K.noise(rng, "C32", sum(n * r for n, r in cuts))
    first = 77 * D
    v, S, _ = K.Model(D, g, offsets, first).run(K.deliver(u, cuts, gap, 1e6))
    for c, f in enumerate(offsets):
        want, _, Sw = b2.ddc(u, f, K.FS, D, None, first_sample=first, g=g[c], detail=True)
        assert np.max(np.abs(v[c] - want)) <= 1e-12 * np.max(np.abs(want))
        assert np.max(np.abs(S[c] - Sw)) <= 1e-12 * np.max(Sw)


# ------------------------------------------------------------------------------------------------------------- conditions
@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_census_conditions(b2, case):
    D, T = case.D, case.T
    p = K.plan(D, T)
    cen = K.census_a(D, T, p.tile)
    n_out = cen.n_in // D
    assert cen.rows >= 2 and n_out > p.tile and cen.u.shape[1] == cen.rows * cen.n_in
    for ch in range(2):
        at = cen.where[ch]
        assert at.shape[0] >= D + 1 and np.min(np.diff(at)) >= T and math.gcd(int(at[1] - at[0]), D) == 1
        assert len(set((at % D).tolist())) == D
        has = cen.tap[ch] >= 0
        # at most one term: the stream itself, output by output
        for m in (0, n_out - 1, n_out, 2 * n_out - 1, p.tile, p.tile - 1):
            lo, hi = max(0, m * D - (T - 1)), m * D
            nz = np.flatnonzero(cen.u[ch, lo:hi + 1])
            assert nz.shape[0] == (1 if has[m] else 0)
            if has[m]:
                assert hi - (lo + nz[0]) == cen.tap[ch, m] and cen.u[ch, lo + nz[0]] == cen.amp[ch][cen.imp[ch, m]]
        assert set(cen.tap[ch][has].tolist()) == set(range(T))  # every tap is met
        m = np.flatnonzero(has)
        assert np.any(m >= n_out) and np.any((m % n_out) >= p.tile)  # rows and tiles beyond the first hold terms
        assert len({complex(a) for a in cen.amp[ch]}) == cen.amp[ch].shape[0]
    assert cen.where[0][1] - cen.where[0][0] != cen.where[1][1] - cen.where[1][0]
    assert not set(map(complex, cen.amp[0])) & set(map(complex, cen.amp[1]))
    amps = np.abs(np.concatenate(cen.amp))
    h = K.comparable_taps(T)
    # nothing planted below 1e-3 of the largest: the taps of census A and C, the impulses' amplitudes
    assert np.min(np.abs(h)) * np.min(amps) >= 1e-3 * np.max(np.abs(h)) * np.max(amps)
    assert np.min(np.abs(h)) >= 1.0 and np.max(np.abs(h)) < 2.0
    # census B: outputs that read the carried history, and outputs that read across a row edge, for every t0 >= 1
    cuts, gap = K.dense_cuts(D, p.tile)
    n_in = cuts[0][0]
    t0s = K.census_b_taps(D, T)
    assert {0, T - 1} <= set(t0s) and set(K.seam_taps(D, T)) <= set(t0s) and len(K.seam_taps(D, T)) == 2 * (p.G - 1)
    assert len(cuts) == 2 and cuts[0][1] == 2 and n_in >= T - 1 and n_in // D > p.tile and gap > 0
    assert any(t >= 1 for t in t0s)  # then output 0 of call 2 reads the history and output 0 of a row 1 the row in front


# ----------------------------------------------------------------------------------------------------------------- the gap
def hidden_taps(b2, D, T, h, n_out, seed=11):
    """The taps t that can be dropped one at a time without any output leaving the contract's bound: (over the whole
    stream, over the outputs past the start-up m >= ceil(T / D))."""
    rng = np.random.default_rng(seed)
    u = K.noise(rng, "C32", n_out * D)
    g = b2.ddc_taps(h, K.IRR, K.FS).astype(np.complex64)
    _, _, S = b2.ddc(u, K.IRR, K.FS, D, None, g=g, detail=True)
    bound = (3 * T + 8) * K.CONTRACT * S
    ext = np.concatenate([np.zeros((2, T - 1)), np.abs(u)], axis=1)
    start = -(-T // D)
    whole = steady = 0
    for t in range(T):
        term = abs(g[t]) * ext[:, T - 1 - t: T - 1 - t + (n_out - 1) * D + 1: D]  # what dropping tap t takes from each output
        whole += bool(np.all(term <= bound))
        steady += bool(np.all(term[:, start:] <= bound[:, start:]))
    return whole, steady


def test_the_gap_as_measured(b2):
    """Designed taps under noise hide hundreds of a long filter's taps from the contract; comparable taps hide none."""
    for D, T in [(1, 1024), (4, 1024), (16, 1024), (24, 1024), (64, 193)]:
        n_out = 4 * -(-T // D) + 64
        whole, steady = hidden_taps(b2, D, T, b2.ddc_design(D, T), n_out)
        cw, cs = hidden_taps(b2, D, T, K.comparable_taps(T), n_out)
        print(f"D = {D}, T = {T}, {n_out} outputs: designed taps hide {whole} of {T} over the whole stream, {steady} past the "
              f"start-up; comparable taps {cw} and {cs}")
        assert steady >= whole > 0
        assert cw == 0 and cs == 0


# ------------------------------------------------------------------------------------------------------- sensitivity proof
def census_scene(b2, D, T, C=2):
    offsets = K.OFFSETS[C]
    g = taps_of(b2, K.comparable_taps(T), offsets)
    cen = K.census_a(D, T, K.plan(D, T).tile)
    return dict(D=D, g=g, offsets=offsets, calls=K.deliver(cen.u, [(cen.n_in, cen.rows)], 5, 1e6), cen=cen, k=K.SINGLE,
                n_out=cen.u.shape[1] // D)


def dense_scene(b2, D, T, C=2):
    """Census C as the GPU file delivers it: comparable taps under noise, two calls of two rows, under the contract."""
    offsets = K.OFFSETS[C]
    g = taps_of(b2, K.comparable_taps(T), offsets)
    cuts, gap = K.dense_cuts(D, K.plan(D, T).tile)
    u = K.noise(np.random.default_rng(3), "C32", sum(n * r for n, r in cuts))
    return dict(D=D, g=g, offsets=offsets, calls=K.deliver(u, cuts, gap, 1e6), k=(3 * T + 8) * K.CONTRACT, n_out=u.shape[1] // D)


def history_scene(b2, D, T, a, how="calls", gap=5):
    offsets = K.OFFSETS[2]
    g = taps_of(b2, K.comparable_taps(T), offsets)
    cen, n1, n2 = K.history_stream(D, T, a)
    cuts = {"calls": [(n1, 1), (n2, 1)], "short": [(n1, 1)] + [(D, 1)] * (n2 // D),
            "rows": [(n1, 1), (K.UNIT * D, n2 // (K.UNIT * D))]}[how]
    return dict(D=D, g=g, offsets=offsets, calls=K.deliver(cen.u, cuts, gap, 1e6), cen=cen, k=K.SINGLE, n1=n1)


def run_fault(sc, fault):
    """(worst |faulted - right| over the right output's bound where that is not zero, the outputs that differ at all)."""
    v, S, _ = K.Model(sc["D"], sc["g"], sc["offsets"], 9 * sc["D"]).run(sc["calls"])
    w, _, _ = K.Model(sc["D"], sc["g"], sc["offsets"], 9 * sc["D"], fault).run(sc["calls"])
    bound = sc["k"] * S
    nz = bound > 0
    diff = np.abs(w - v)
    factor = float(np.max(diff[nz] / bound[nz])) if nz.any() else 0.0
    return factor, ~((w == v) | (np.isnan(w) & np.isnan(v)))


def tap_is(sc, pred):
    """Mask [C][2][n_out] of the outputs whose one term's tap satisfies pred."""
    t = sc["cen"].tap
    return np.broadcast_to((t >= 0) & pred(t), (len(sc["offsets"]),) + t.shape)


def after(sc, n):
    """Mask of the outputs at index n or later."""
    t = sc["cen"].tap
    return np.broadcast_to(np.arange(t.shape[1]) >= n, (len(sc["offsets"]),) + t.shape)


def proofs(b2):
    """(name, fault, the scene that shows it, where its term exists in that scene, a scene in which it exists nowhere)."""
    out = []
    for D, T in ((33, 67), (64, 193), (32, 1024)):
        sc = census_scene(b2, D, T)
        p = K.plan(D, T)
        tag = f"census A D{D} T{T}"
        out.append((f"first tap dropped, {tag}", ("drop", 0), sc, tap_is(sc, lambda t: t == 0), None))
        out.append((f"last tap dropped, {tag}", ("drop", T - 1), sc, tap_is(sc, lambda t: t == T - 1), None))
        for t0 in K.seam_taps(D, T):
            out.append((f"seam tap {t0} dropped, {tag}", ("drop", t0), sc, tap_is(sc, lambda t, t0=t0: t == t0), None))
            out.append((f"seam tap {t0} twice, {tag}", ("double", t0), sc, tap_is(sc, lambda t, t0=t0: t == t0), None))
        if T % p.G:
            lost = T - p.G * (T // p.G)  # kernel indices behind G floor(T / G): the taps 0 ... lost - 1
            out.append((f"Tseg = floor(T / G), {tag}", ("tseg", 0), sc, tap_is(sc, lambda t, lost=lost: t < lost), census_scene(b2, 4, 40)))
        never = census_scene(b2, 16, 12)  # the phase never reaches row D - 1: no wrap to get wrong
        # (33, 67): a segment of 34 taps from phase 0 or 1 ends as the phase reaches D + 1 = 34, a late wrap shows nowhere
        out.append((f"phase row wraps at D - 1, {tag}", ("wrap", -1), sc, None, never))
        out.append((f"phase row wraps at D + 1, {tag}", ("wrap", 1), sc, None, never))
        # (33, 67) again: no impulse lies in the 66 samples in front of a tile; census C's dense stream shows it there
        for scene, what in ((sc, tag), (dense_scene(b2, D, T), f"census C D{D} T{T}")):
            beyond = np.arange(scene["n_out"]) >= p.tile
            out.append((f"lead-in one sample off, {what}", ("leadin", 0), scene, np.broadcast_to(beyond, (2, 2, scene["n_out"])), None))
    D = 4
    sc = history_scene(b2, D, 512, 100)  # the impulse ends at history entry 510 - 100 = 410
    out.append(("history entries e >= 256 stale, H = 511", ("stale", 0), sc, after(sc, sc["n1"] // D), history_scene(b2, D, 256, 100)))
    sc = history_scene(b2, D, 300, 10)
    out.append(("history shifted by one, H = 299", ("shift", 0), sc, after(sc, sc["n1"] // D), None))
    out.append(("x and y swapped in the history, H = 299", ("swap_xy", 0), sc, after(sc, sc["n1"] // D), None))
    out.append(("position advanced by n_in, D = 4", ("pos_n_in", 0), sc, after(sc, sc["n1"] // D), history_scene(b2, 1, 300, 10)))
    sc = history_scene(b2, D, 300, 0, "short")
    out.append(("a short call overwrites the history, H = 299", ("overwrite", 0), sc, after(sc, sc["n1"] // D + 1), history_scene(b2, D, 300, 0)))
    sc = history_scene(b2, D, 300, 10, "rows")
    out.append(("row walk-back by in_stride, H = 299", ("stride_walk", 0), sc, after(sc, sc["n1"] // D + K.UNIT),
                history_scene(b2, D, 300, 10, "rows", gap=0)))
    return out


def test_every_wrong_restatement_is_caught(b2):
    """Each moves a checked output by more than 1000 bounds, differs only where its term exists, and differs nowhere in a
    scene without its term."""
    best = {}
    for name, fault, sc, exists, absent in proofs(b2):
        factor, changed = run_fault(sc, fault)
        print(f"{name}: {factor:.3g} bounds, {int(changed.sum())} outputs differ")
        if exists is not None:
            assert not np.any(changed & ~exists), name
        if absent is not None:
            f0, c0 = run_fault(absent, fault)
            assert f0 == 0.0 and not c0.any(), name
        key = fault if fault[0] in ("wrap", "drop", "double") else fault[0]
        key = (key[0], "first" if key[1] == 0 else "last" if key[1] == sc["g"].shape[1] - 1 else "seam") if key[0] in ("drop", "double") else key
        best[key] = max(best.get(key, 0.0), factor)
    for key, factor in best.items():
        assert factor > 1000.0, key
    assert set(best) == (set(K.FAULTS) - {"wrap", "drop", "double"}) | {("wrap", -1), ("wrap", 1), ("drop", "first"), ("drop", "last"),
                                                                       ("drop", "seam"), ("double", "seam")}


# -------------------------------------------------------------------------------------------------------- single-term bound
def test_the_single_term_bound_holds_for_the_fp32_chain():
    """One complex product as the kernel forms it (fl(g.x u.x), then one fused multiply-add; the phasor rounded to fp32 and
    multiplied by ddc_mul's two products and two fused multiply-adds), emulated in fp32 / fp64: under 8 2^-24 |g| |a|."""
    rng = np.random.default_rng(2)
    n = 200000
    f32 = np.float32
    g = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    a = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    th = rng.uniform(-0.5, 0.5, n)
    gx, gy, ux, uy = (z.astype(np.float64) for z in (g.real, g.imag, a.real, a.imag))

    def fma(x, y, z):  # products of fp32 numbers are exact in fp64; one more rounding to fp32
        return f32(x * y + np.float64(z)).astype(np.float64)
    xr = fma(-gy, uy, fma(gx, ux, 0.0))
    xi = fma(gy, ux, fma(gx, uy, 0.0))
    pc, ps = f32(np.cos(2 * np.pi * th)).astype(np.float64), f32(-np.sin(2 * np.pi * th)).astype(np.float64)
    vr = fma(-ps, xi, f32(pc * xr))
    vi = fma(ps, xr, f32(pc * xi))
    want = np.exp(-2j * np.pi * th) * g.astype(np.complex128) * a.astype(np.complex128)
    ratio = np.abs((vr + 1j * vi) - want) / (np.abs(g.astype(np.complex128)) * np.abs(a.astype(np.complex128)) * 2.0 ** -24)
    print(f"one term, fp32 chain emulated: worst {ratio.max():.2f} of 2^-24 |g| |a| (derived 5.54, asserted 8)")
    assert ratio.max() <= 8.0
