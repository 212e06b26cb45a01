"""CPU: the clutter-map detector's tables and its fp64 restatement (blah2hip_cmap_alpha is host arithmetic of the library,
so it runs here; ``clutter_map_alpha``, ``clutter_map``, ``gate_hits`` are process.py's).

  * tables: the library's against the restatement (at most one ulp apart), the closed form up to the memory, the anchors
    of include/blah2hip.h, back-substitution to pfa within 1e-10, constant entries beyond 16 T, the refusals;
  * false-alarm rate: 81 x 200 cells, 64 CPIs of noise, T = 8, pfa = 1e-2, normalised: 10 206 exceeding cells expected over
    ages 1 .. 63, the count within 5 % (five binomial standard deviations of 101) -- and four ways to get the definition
    wrong, whose expectations are 6 164, 15 697, 11 399 and 11 512, outside it;
  * the scene of tests/clutter_map_scenes.py: the fixed discrete never exceeds, the moving target exceeds at every age
    from 4 on, the other cells stay within five standard deviations of pfa;
  * the fp32 update: the bound ``|b_fp32 - b_fp64| <= (k + 4) 2^-24 U`` (derived in include/blah2hip.h) holds for an
    emulation of the kernel's roundings in every cell, and the share of it the emulation reaches is printed: 0.60 at T = 1,
    0.42 at T = 8 and 0.44 at T = 64 over 40 CPIs of noise;
  * the inputs of tests/test_clutter_map_gpu.py have no cell inside the decision margin (the condition of its 1e-4 cap).
"""
import ctypes as C

import numpy as np
import pytest

import clutter_map_scenes as S


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    return blah2_amd


# age: (value, half a unit of its last digit)
ANCHORS_1E2 = {1: (99.0, 1e-9), 2: (18.0, 1e-9), 3: (10.9248, 5e-5), 4: (8.6491, 5e-5), 5: (7.5594, 5e-5), 6: (6.9266, 5e-5),
               7: (6.5149, 5e-5), 8: (6.2262, 5e-5), 16: (5.45031, 5e-6), 128: (5.33810, 5e-6)}
ANCHORS_1E3 = {8: (10.97099, 5e-6), 128: (8.58850, 5e-6)}


@pytest.mark.parametrize("pfa,T,max_age", [(1e-2, 8, 200), (1e-3, 8, 130), (1e-5, 1, 20), (1e-4, 3, 60), (0.3, 2, 40)])
def test_library_table_is_the_restatement(b2, pfa, T, max_age):
    lib = b2.clutter_map_alpha_table(pfa, T, max_age)
    py = b2.clutter_map_alpha(pfa, T, max_age)
    assert np.isnan(lib[0]) and np.isnan(py[0])
    ulps = np.abs(lib[1:] - py[1:]) / np.spacing(np.minimum(lib[1:], py[1:]))
    print("largest difference in ulps:", ulps.max())
    assert ulps.max() <= 1.0
    for t in (lib, py):
        for a in range(1, min(T, max_age) + 1):
            assert t[a] == a * (pfa ** (-1.0 / a) - 1), a  # blah2hip_cfar_alpha's one-look value for n = a
        assert np.array_equal(t[1:min(T, max_age) + 1], b2.cfar_alpha_table(pfa, 1, T)[1:min(T, max_age) + 1])
        assert (t[16 * T:] == t[min(16 * T, max_age)]).all()  # entries beyond 16 T repeat that one
        assert (np.diff(t[1:16 * T + 1]) <= 1e-12).all()      # the factor falls as the average settles, then stays to a few ulps
        for a in range(1, max_age + 1):
            assert abs(b2.clutter_map_pfa(t[a], min(a, 16 * T), T) - pfa) <= 1e-10, a


def test_anchors(b2):
    for pfa, anchors in ((1e-2, ANCHORS_1E2), (1e-3, ANCHORS_1E3)):
        for t in (b2.clutter_map_alpha_table(pfa, 8, 128), b2.clutter_map_alpha(pfa, 8, 128)):
            for a, (v, tol) in anchors.items():
                assert abs(t[a] - v) <= tol, (pfa, a, t[a], v)


def test_memory_64_table_and_its_tail(b2):
    t = b2.clutter_map_alpha_table(1e-3, 64, 1100)
    assert abs(t[1024] - t[1023]) <= 1.5e-14 and (t[1024:] == t[1024]).all()
    for a in (65, 100, 640, 1024):
        assert abs(b2.clutter_map_pfa(t[a], a, 64) - 1e-3) <= 1e-10


def test_weights(b2):
    for a, T in ((1, 8), (5, 8), (8, 8), (9, 8), (40, 8), (3, 1), (100, 64)):
        w = b2.clutter_map_weights(a, T)
        assert w.shape == (a,) and abs(w.sum() - 1.0) < 1e-14 and (w >= 0).all()  # (T = 1: all weight on the newest)
    # the recursion's own weights: feed unit impulses through clutter_map
    T, n = 4, 11
    for i in range(n):
        maps = np.zeros((n, 1, 1), dtype=np.complex64)
        maps[i] = 1.0
        _, b = b2.clutter_map(maps, None, np.full(16 * T + 1, 1.0), T)
        assert abs(b[0, 0] - b2.clutter_map_weights(n, T)[n - 1 - i]) < 1e-7, i  # (r is the fp32 quotient)


def test_table_refusals(b2):
    L = b2.load()
    out = np.zeros(8)
    p = out.ctypes.data_as(C.c_void_p)
    assert L.blah2hip_cmap_alpha(1e-3, 8, 4, None) == -1
    for T in (0, 65):
        assert L.blah2hip_cmap_alpha(1e-3, T, 4, p) == -1
    for pfa in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert L.blah2hip_cmap_alpha(pfa, 8, 4, p) == -1
        with pytest.raises(ValueError):
            b2.clutter_map_alpha(pfa, 8, 4)
    with pytest.raises(ValueError):
        b2.clutter_map_alpha(1e-3, 65, 4)
    assert L.blah2hip_cmap_alpha(1e-3, 64, 4, p) == 0
    assert L.blah2hip_cmap_create(None, 8, 0, None) == -1  # NULL arguments are refused before any device is looked for


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_false_alarm_rate(b2, seed):
    T, pfa, n_cpi = 8, 1e-2, 64
    maps = S.noise(n_cpi, 81, 200, seed)
    lev = S.levels(maps)
    alpha = b2.clutter_map_alpha(pfa, T, 16 * T)
    exceed, _ = b2.clutter_map(maps, lev, alpha, T)
    assert not exceed[0].any()  # age 0 never exceeds
    n = int(exceed.sum())
    expect = 81 * 200 * 63 * pfa
    print(f"seed {seed}: {n} exceeding cells, {expect:.0f} expected")
    assert expect == 10206 and abs(n - expect) <= 0.05 * expect
    u = (np.abs(maps.astype(np.complex128)) ** 2 * lev[:, None, None]).reshape(n_cpi, -1)
    assert S.count_variant(u, alpha, T, "right") == n  # the helper counts what the restatement counts
    for variant in ("frozen", "steady", "nowarm", "shifted"):
        wrong = S.count_variant(u, alpha, T, variant)
        print(f"  {variant}: {wrong}")
        assert abs(wrong - expect) > 0.05 * expect, variant


def test_scene(b2):
    T, pfa = 8, 1e-3
    maps, discrete, target = S.scene(3)
    alpha = b2.clutter_map_alpha(pfa, T, 16 * T)
    exceed, _ = b2.clutter_map(maps, S.levels(maps), alpha, T)
    n_cpi = maps.shape[0]
    assert not exceed[:, discrete[0], discrete[1]].any()
    hit = [bool(exceed[g, r, c]) for g, (r, c) in enumerate(target)]
    print("target exceeds at ages", [g for g in range(n_cpi) if hit[g]])
    assert all(hit[4:]) and not hit[0]
    others = int(exceed.sum()) - sum(hit)
    expect = (maps[0].size - 2) * (n_cpi - 1) * pfa
    print(f"{others} other cells exceed, {expect:.1f} expected")
    assert abs(others - expect) <= 5 * np.sqrt(expect)


@pytest.mark.parametrize("T,n_cpi", [(1, 12), (2, 40), (3, 12), (8, 40), (64, 40)])
def test_fp32_update_stays_inside_the_derived_bound(b2, T, n_cpi):
    maps = S.noise(n_cpi, 21, 111, 40 + T)
    maps[:, 3, 7] *= 100.0  # a cell four decades up: the bound scales with the cell's own u
    lev = S.levels(maps).astype(np.float32)
    state = {}
    alpha = b2.clutter_map_alpha(1e-3, T, 16 * T)
    worst = 0.0
    # cut into calls, so that the bound is checked at several ages (the emulation carries its own b on)
    b32, at = None, 0
    for cut in (1, 2, 5, n_cpi - 8):
        b32 = S.emulate_f32(maps[at:at + cut], lev[at:at + cut], T, at, b32)
        b2.clutter_map(maps[at:at + cut], lev[at:at + cut].astype(np.float64), alpha, T, state)
        at += cut
        err = np.abs(b32.astype(np.float64) - state["b"])
        bound = S.b_bound(at, T, state["umax"])
        assert (err <= bound).all(), (T, at, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    print(f"T = {T}: the emulation reaches {worst:.2f} of the bound")
    assert worst > 0.01  # the bound is of the size of the error, not decades above it


def test_gpu_inputs_have_no_cell_inside_the_margin(b2):
    """The condition of test_clutter_map_gpu.py's cap of 1e-4 on the cells that may go either way: the restatement alone
    (with the levels rounded to fp32, as the device hands them out) stays within it on the compared inputs."""
    inputs = [(c.tag, S.case_maps(c), c.T, c.pfa, c.normalise) for c in S.CASES] + [("scene", S.scene(3)[0], 8, 1e-3, True)]
    for tag, maps, T, pfa, normalise in inputs:
        alpha = b2.clutter_map_alpha_table(pfa, T, 16 * T)
        lev = S.levels(maps).astype(np.float32).astype(np.float64) if normalise else None
        exceed, _, detail = b2.clutter_map(maps, lev, alpha, T, detail=True)
        inside = int(S.margin_cells(detail, alpha, T).sum())
        tested = exceed[1:].size
        print(f"{tag}: {inside} of {tested} cells inside the margin")
        assert inside <= 1e-4 * tested, tag
