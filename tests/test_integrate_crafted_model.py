"""CPU: the crafted maps, schedules and emulation of tests/integrate_crafted.py for the non-coherent integrator, checked
without a device on what tests/test_integrate_crafted_gpu.py hands to the GPU.

The clean emulation (fp32, the kernel's order) stays inside the derived cell bound ``(K W + 8) 2^-24 ref`` against
``blah2_amd.integrate_maps`` for every window, schedule, K in {1, 2} and hop in {1, W, W + 3}, gives the same bits under
every schedule and ends its windows where ``integrate_ends`` says.  The case tables reach all five ring lengths, a window
across the ring's wrap for every W > 1, three consecutive groups of four windows, a call that moves every plane of a full
history and a call on a history still filling.  Sensitivity: eight wrong walks each put more than half of the cells of the
windows they touch beyond ten times the cell bound, and five wrong epilogues each move noisePower or maxPower of an output
map of the planted scenes by ten times the 1e-3 dB gate or more.  The factors of ten are conditions, not measurements: they
are what makes a pass on the GPU mean something.

Measured here (printed by the tests): the clean emulation's largest error / bound is 0.195 (W = 3) falling to 0.12 (W = 16);
every cell mutant puts 99.87 % or more of the cells of the windows it touches beyond ten bounds (184 .. 720 windows each); a
planted cell lost moves maxPower by 0.116 dB or more on every map (the step down to the next planted cell; 34 dB at W = 1)
and one counted twice noisePower by 1.38e-2 dB or more on every map; a wave's dropped maximum moves maxPower by 0.13 dB or
more on the maps whose planted cell that wave owns, a maximum carried over from the other LDS set by 0.53 dB on every map
from the second group on, and the single-cell unit's absent cell counted moves noisePower by 1.46e-2 dB or more on the maps
whose peak is the last cell (6e-4 .. 1e-3 dB on the others: under ten gates, so those maps are not asked to catch it).

What a scene cannot do, and who does it instead.  A maximum carried over from the other LDS set shows only within a call
that has two groups with windows: the emulation starts every call with cleared sets, so the one-CPI schedule cannot show it
and the one-call schedule does.  The absent cell of the single-cell unit shows on the odd geometry alone, and there on the
maps whose planted cell is the last one; were it counted as the zero it holds in the ring, noisePower would be -inf on
every map.  The history mutants touch nothing in a single call.
"""
import numpy as np
import pytest

import blah2_amd
import integrate_crafted as IC

ND, NC = 21, 111  # the odd geometry: 2331 cells, five workgroups, the last unit a single cell
WINDOWS = list(range(1, IC.MAX_WINDOW + 1))
METRIC_WINDOWS = (1, 4, 9)


def bound_of(ref, K, W):
    return (K * W + 8) * 2.0 ** -24 * ref


def hops_of(W):
    return (1, W, W + 3)


# ---- 1. the clean emulation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", WINDOWS)
def test_clean_emulation_holds_the_bound_whatever_the_cuts(W):
    N = IC.stream_length(W)
    worst = 0.0
    for K in (1, 2):
        m = IC.maps(K, N, ND, NC, seed=500 + 10 * W + K)
        for H in hops_of(W):
            ref = blah2_amd.integrate_maps(m, None, W, H).reshape(-1, ND * NC)
            ends = blah2_amd.integrate_ends(N, W, H)
            whole = None
            for name, cuts in IC.schedules(W, N).items():
                e = IC.emulate(m, W, H, cuts)
                assert e["ends"] == ends, (K, H, name)
                assert sum(n for n, _ in e["calls"]) == len(ends)
                assert e["out"].dtype == np.float32 and e["out"].shape == ref.shape
                if whole is None:
                    whole = e
                    err = np.abs(e["out"].astype(np.float64) - ref)
                    ratio = float((err / bound_of(ref, K, W)).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (K, H, ratio)
                else:
                    assert np.array_equal(e["out"].view(np.uint32), whole["out"].view(np.uint32)), (K, H, name)
                    assert np.array_equal(e["met"].view(np.uint64), whole["met"].view(np.uint64)), (K, H, name)
                assert not e["touched"].any()
            for i in range(len(ends)):
                noise, peak = IC.set_metrics64(whole["out"][i])
                assert abs(whole["met"][i, 0] - noise) <= IC.DB_TOL and abs(whole["met"][i, 1] - peak) <= IC.DB_TOL
    print(f"\n[W {W}] clean emulation: largest error / bound {worst:.3f}")


def test_the_recipe_tells_cells_and_terms_apart():
    m = IC.maps(2, 9, ND, NC, seed=3)
    mag = np.abs(m.astype(np.complex128))
    u = mag / IC.level(2, 9)[:, :, None, None]
    assert m.dtype == np.complex64 and 0.7 - 1e-6 <= u.min() < 0.71 and 1.39 < u.max() <= 1.4 + 1e-6
    # no two neighbouring cells and no two CPIs of a cell alike to a part in a thousand, but for a few
    flat = mag.reshape(2, 9, -1)
    assert (np.abs(flat[:, :, 1:] / flat[:, :, :-1] - 1) > 1e-3).mean() > 0.99
    assert (np.abs(flat[:, 1:] / flat[:, :-1] - 1) > 1e-3).mean() > 0.99
    assert np.array_equal(IC.maps(2, 9, ND, NC, seed=3), m)


def test_schedules_are_the_cuts_they_claim():
    for W in WINDOWS:
        R, N = IC.nci_ring(W), IC.stream_length(W)
        s = IC.schedules(W, N)
        assert s["one-call"] == [N] and s["one-cpi"] == [1] * N
        assert set(s["short"][:-1]) <= {max(W - 2, 1)} and sum(s["short"]) == N
        assert s["mixed"][:-1] == [n for n in (1, W - 1, W, R + 1) if n] and s["mixed"][-1] == N - 2 * W - R - 1 > 0
        cut = IC.clipped(s["mixed"], 8)
        assert sum(cut) == N and max(cut) == min(8, max(s["mixed"])) and (cut == s["mixed"]) == (max(s["mixed"]) <= 8)


# ---- 2. the case tables -----------------------------------------------------------------------------------------------------
def test_case_tables_reach_what_they_claim():
    assert {IC.nci_ring(W) for W in WINDOWS} == {4, 8, 12, 16, 20}
    assert [IC.nci_ring(W) for W in (1, 2, 5, 6, 9, 10, 13, 14, 16)] == [4, 8, 8, 12, 12, 16, 16, 20, 20]
    facts = []
    for W in WINDOWS:
        N = IC.stream_length(W)
        straddle, steady, full_move, filling = 0, 0, 0, 0
        for name, cuts in IC.schedules(W, N).items():
            for call in IC.plan(W, 1, cuts):
                wins = [w for grp in call["groups"] for w in grp]
                straddle += sum(old > new for _, new, old in wins)
                run = best = 0
                for grp in call["groups"]:
                    run = run + 1 if len(grp) == IC.GROUP else 0
                    best = max(best, run)
                steady += best >= 3
                full_move += call["stay"] > 0 and call["hist_valid"] == W - 1 and W > 1
                filling += 0 < call["hist_valid"] < W - 1
        facts.append((W, IC.nci_ring(W), straddle, steady, full_move, filling))
        assert steady >= 1, W  # three or more consecutive groups of four windows in one call
        if W > 1:
            assert straddle >= 1, W  # a window whose oldest slot lies above its newest: across the ring's wrap
            assert full_move >= 1, W  # a call shorter than a full history: planes move up (from W = 3 on) and are stored
        if W > 2:
            assert filling >= 1, W  # a call on a history that is still filling
    print("\n(W, ring, windows across the wrap, calls with >= 3 full groups, calls moving a full history, calls on a filling history):")
    for f in facts:
        print("  ", f)
    # the hop cases of the GPU test: windows end every H CPIs, none lost at a cut
    for W in (5, 9, 13, 16):
        for H in (W, W + 3):
            for K in (2, 3, 8):
                N = IC.stream_length(W)
                cuts = IC.clipped(IC.schedules(W, N)["mixed"], 64 // K)
                calls = IC.plan(W, H, cuts)
                assert max(cuts) * K <= 64 and sum(c["n_out"] for c in calls) == len(blah2_amd.integrate_ends(N, W, H)) >= 2


# ---- 3. sensitivity of the cell gate ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", IC.CELL_MUTANTS)
def test_every_cell_mutant_moves_most_cells_of_the_windows_it_touches(mutant):
    K, w = (3, (1.0, 0.25, 4.0)) if mutant == "wrong-weights" else (2, None)
    least, touched_windows = 1.0, 0
    for W in (1, 2, 3, 5, 9, 13, 16):
        N = IC.stream_length(W)
        m = IC.maps(K, N, ND, NC, seed=700 + W)
        ref = blah2_amd.integrate_maps(m, w, W, 1).reshape(-1, ND * NC)
        bound = bound_of(ref, K, W)
        for name, cuts in IC.schedules(W, N).items():
            e = IC.emulate(m, W, 1, cuts, w=w, mutant=mutant, metrics=False)
            err = np.abs(e["out"].astype(np.float64) - ref)
            t = e["touched"]
            assert (err[~t] <= bound[~t]).all(), (W, name)  # what it does not touch stays inside the bound
            if mutant in ("hist-reversed", "no-moveup", "hist-off-one"):
                assert name != "one-call" or not t.any()
            if t.any():
                share = float((err[t] > 10 * bound[t]).mean())
                least = min(least, share)
                touched_windows += int(t.sum())
                assert share > 0.5, (W, name, share)
    assert touched_windows > 0
    print(f"\n[{mutant}] {touched_windows} windows touched; least share of their cells beyond 10 bounds: {100 * least:.2f} %")


def test_the_mutants_touch_what_they_should():
    W, N = 5, IC.stream_length(5)
    m = IC.maps(2, N, ND, NC, seed=9)
    n_out = N - W + 1
    cuts = IC.schedules(W, N)
    for mutant in ("swap", "stale-slot", "dropped-channel", "shift8"):
        assert IC.emulate(m, W, 1, cuts["one-call"], mutant=mutant, metrics=False)["touched"].sum() == n_out
    # an even map on an aligned base has no plane 8 bytes off; on a base 8 bytes off every plane is
    even = IC.maps(2, N, ND, NC + 1, seed=9)
    assert not IC.emulate(even, W, 1, cuts["one-call"], mutant="shift8", metrics=False)["touched"].any()
    assert IC.emulate(even, W, 1, cuts["one-call"], mutant="shift8", in_off=8, metrics=False)["touched"].all()
    # reversed planes: the window that holds all of them is the same sum; the W - 2 behind it are not.  In calls of one CPI
    # the reversed values are also what moves up, so later calls stay touched
    t = IC.emulate(m, W, 1, [W - 1, N - W + 1], mutant="hist-reversed", metrics=False)["touched"]
    assert t.tolist() == [False] + [True] * (W - 2) + [False] * (n_out - W + 1)
    for mutant in ("no-moveup", "hist-off-one"):
        assert IC.emulate(m, W, 1, cuts["one-cpi"], mutant=mutant, metrics=False)["touched"].all()


# ---- 4. sensitivity of the metrics gate -------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", METRIC_WINDOWS)
def test_every_metrics_mutant_moves_a_metric_by_ten_gates(W):
    K, N = 2, IC.scene_length(W, 2)
    m, at = IC.planted(K, N, ND, NC, seed=900 + W)
    need = 10 * IC.DB_TOL
    clean = IC.emulate(m, W, 1, [N], plants=at)
    n_out = len(clean["ends"])
    assert n_out == N - W + 1 and set(at[:n_out]) == set(IC.seams(ND, NC))
    for i, g in enumerate(clean["ends"]):
        assert int(np.argmax(clean["out"][i])) == at[g - W + 1], g  # the window's oldest planted cell is its maximum
        noise, peak = IC.set_metrics64(clean["out"][i])
        assert abs(clean["met"][i, 0] - noise) <= IC.DB_TOL and abs(clean["met"][i, 1] - peak) <= IC.DB_TOL
    one = IC.emulate(m, W, 1, [1] * N, plants=at)
    assert np.array_equal(one["met"].view(np.uint64), clean["met"].view(np.uint64))
    moves = {}
    for mutant in IC.METRIC_MUTANTS:
        e = IC.emulate(m, W, 1, [N], mutant=mutant, plants=at)
        assert np.array_equal(e["out"].view(np.uint32), clean["out"].view(np.uint32))
        moves[mutant] = np.abs(e["met"] - clean["met"]).max(axis=1)
    for mutant in ("lost", "twice"):  # on every map
        assert (moves[mutant] >= need).all(), (mutant, moves[mutant].min())
    for mutant in IC.METRIC_MUTANTS:  # on some map
        assert moves[mutant].max() >= need, (mutant, moves[mutant].max())
    # each dropped wave shows on the maps whose planted cell that wave owns, the absent cell where the last cell is planted
    for i, g in enumerate(clean["ends"]):
        cell = at[g - W + 1]
        wave = cell // 128 % 4
        assert moves[f"wave-max-{wave}"][i] >= need, (g, cell)
        if cell == ND * NC - 1:
            assert moves["absent-cell"][i] >= need, g
    # carried over: every window from the second group on has a taller one in the other set
    assert (moves["max-carried"][IC.GROUP:] >= need).all()
    # ... and calls of one CPI cannot show it: every call starts with cleared sets
    assert np.array_equal(IC.emulate(m, W, 1, [1] * N, mutant="max-carried", plants=at)["met"], clean["met"])
    print(f"\n[W {W}] metrics mutants, dB moved (least over the maps / largest): "
          + ", ".join(f"{k} {v.min():.2e} / {v.max():.2e}" for k, v in moves.items()))


def test_the_stream_scaled_down_lies_below_0_db():
    m = IC.maps(2, 12, ND, NC, seed=5)
    small = (m * np.complex64(1e-3)).astype(np.complex64)
    e = IC.emulate(small, 4, 1, [12])
    assert e["out"].max() < 1.0 and (e["met"][:, 1] == -e["met"][:, 0]).all()
