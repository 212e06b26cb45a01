"""CPU: integration along tracks (blah2hip_nci_process_tracks_dev) -- the fp64 restatement ``integrate_tracks``, the tables of
``track_tables``, an fp32 emulation of the device's walk (tests/track_scenes.py) with eight wrong variants of it, and the
walking-echo scene.  No GPU: what tests/test_tracks_gpu.py asks of the device is shown here to be reachable by the
definition's fp32 arithmetic and out of reach for its near misses.

Bound: a cell lies within (n_surv W + 8) 2^-24 of the fp64 value of the hypothesis that is named (derived in
include/blah2hip.h: every term is non-negative, a term passes n_surv + 2 roundings into p, at most W - 1 additions -- an
addition of +0 for a term outside the map rounds nothing --, the scale and the square root; the selection adds no rounding).

The scene (SCENE in tests/track_scenes.py; seed 3, 21 x 111 cells, W = 8, 9 dB per look): figures printed by the test, recorded
in DESIGN.md section 7 item 19.
"""
import numpy as np
import pytest

import blah2_amd as b2
import track_scenes as TS


@pytest.fixture(scope="module")
def shared():
    """The shared input with its fp64 restatement, computed once and left unchanged."""
    maps, walk, q = TS.shared_input()
    s = TS.SHARED
    levels, index, sums = b2.integrate_tracks(maps, walk, q, None, s["W"], s["H"])
    scale = float(np.float32(1.0 / s["W"]))
    return dict(s, maps=maps, walk=walk, q=q, levels=levels, index=index, sums=sums, scale=scale)


def test_shared_input_has_no_two_hypotheses_alike(shared):
    """Checked first: for every output map, every cell and every pair of hypotheses the fp64 sums differ by more than
    2 (n_surv W + 8) 2^-24 of the larger, so the index is defined in every cell and none is left out of any comparison."""
    assert shared["sums"].shape == (3, 3, 21, 111)
    closest = TS.closest_pair(shared["sums"])
    print(f"closest pair of hypotheses: {closest:.3e} of the larger, against {2 * TS.bound(shared['K'], shared['W']):.3e}")
    assert closest > 2 * TS.bound(shared["K"], shared["W"])


def test_zero_walk_and_the_bank_of_zero_is_integrate_maps():
    maps = TS.IC.maps(3, 7, 9, 13, seed=5)
    w = (1.0, 0.25, 4.0)
    for W, H in ((1, 1), (3, 1), (3, 2), (4, 5)):
        levels, index, sums = b2.integrate_tracks(maps, None, None, w, W, H)
        assert np.array_equal(levels, b2.integrate_maps(maps, w, W, H))
        assert not index.any() and sums.shape[0] == 1
        levels0, _, _ = b2.integrate_tracks(maps, np.zeros(9), [0.0], w, W, H)
        assert np.array_equal(levels0, levels)


@pytest.mark.parametrize("name", ["zero", "physical", "seams", "beyond", "jagged", "alternating"])
def test_track_tables_against_a_scalar_loop(name):
    walk = TS.tables(21, 111)[name]
    q = np.array([0.0, 1.0, -1.0, 0.5, -0.5, 0.37, -2.5, 1.0])  # ties of rint (0.5 a), a fraction, a duplicate
    for W in (1, 2, 8, 16):
        if np.abs(q).max() * (W - 1) >= 21:
            q = q[np.abs(q) * (W - 1) < 21]
        jr, s = b2.track_tables(walk, q, W)
        jr0, s0 = TS.scalar_tables(walk, q, W)
        assert jr.dtype == np.int32 and s.dtype == np.int32 and jr.shape == (q.size, W, 21)
        assert np.array_equal(jr, jr0) and np.array_equal(s, s0)
        assert (jr[:, 0] == np.arange(21)).all() and not s[:, 0].any()  # age 0 is the cell itself
    assert b2.track_tables(np.zeros(5), None, 3)[0].shape == (1, 3, 5)
    with pytest.raises(ValueError):
        b2.track_tables(np.full(5, np.nan), None, 2)


def test_fp32_emulation_stays_within_the_derived_bound(shared):
    out, index = TS.emulate(shared["maps"], shared["walk"], shared["q"], shared["W"], shared["H"])
    assert np.array_equal(index, shared["index"])  # no two hypotheses are close: the fp32 walk names the fp64 winner
    rel, _ = TS.named_error(out, index, shared["sums"], shared["scale"])
    print(f"fp32 emulation: largest error / bound {rel.max() / TS.bound(shared['K'], shared['W']):.3f}")
    assert (rel <= TS.bound(shared["K"], shared["W"])).all()
    assert len(np.unique(index)) == 3  # every hypothesis wins somewhere


@pytest.mark.parametrize("mutant", TS.MUTANTS)
def test_wrong_variants_miss_the_bound_by_a_factor_of_ten(shared, mutant):
    out, index = TS.emulate(shared["maps"], shared["walk"], shared["q"], shared["W"], shared["H"], mutant=mutant)
    rel, _ = TS.named_error(out, index, shared["sums"], shared["scale"])
    worst = rel.max() / TS.bound(shared["K"], shared["W"])
    print(f"{mutant}: largest error / bound {worst:.3g}, {int((rel > TS.bound(shared['K'], shared['W'])).sum())} cells outside")
    assert worst >= 10.0


def test_the_scene_is_found_along_the_track_and_lost_by_the_plain_sum():
    maps, walk, q, (row, col), true_k = TS.scene()
    W = TS.SCENE["W"]
    levels, index, _ = b2.integrate_tracks(maps, walk, q, None, W, 1)
    plain = b2.integrate_maps(maps, None, W, 1)
    assert levels.shape == plain.shape == (1, 21, 111)
    db = lambda lv, at: 20.0 * np.log10(lv[0][at] / np.median(lv[0]))  # noqa: E731
    print(f"scene: aligned {db(levels, (row, col)):.2f} dB over the median with hypothesis {int(index[0, row, col])}, "
          f"plain window sum {db(plain, (row, col)):.2f} dB over its median")
    assert np.unravel_index(np.argmax(levels[0]), levels[0].shape) == (row, col)
    assert int(index[0, row, col]) == true_k
    assert np.unravel_index(np.argmax(plain[0]), plain[0].shape) != (row, col)
