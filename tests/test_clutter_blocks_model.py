"""The fp64 restatement of the block clutter filter (tests/clutter_blocks_ref.py) against the oracle, the compiled
reference where it is built, and the condition on the drifting-clutter scene that the GPU property test relies on."""
import os

import numpy as np
import pytest

from oracle import blah2_oracle as O
import clutter_blocks_ref as R


@pytest.mark.parametrize("dmin,dmax", [(0, 8), (-3, 13), (2, 18)])
def test_one_block_is_the_oracle(dmin, dmax):
    n = 4096
    x, y = O.synth_iq(n, seed=11, fs=1_000_000, targets=((dmin + 2, 0.0, 0.3), (dmin + 5, 40.0, 0.05)))
    ok_ref, y_ref, w_ref, r_ref, b_ref = O.wiener_hopf(x, y, dmin, dmax, return_filter=True)
    ok, yf, w, r, b = R.wiener_hopf_blocks(x, y, dmin, dmax, 1)
    assert ok_ref and ok.all()
    assert np.array_equal(w[0], w_ref) and np.array_equal(r[0], r_ref) and np.array_equal(b[0], b_ref)
    err = np.max(np.abs(yf - y_ref)) / np.max(np.abs(y_ref))
    print(f"\n[blocks model B=1 {dmin}..{dmax}] y {err:.2e}")
    assert err <= 1e-12


def test_history_crosses_the_block_edge():
    """Block j's first outputs use block j - 1's samples: they differ from the block filtered alone (zero history) there,
    and only there."""
    n, B, dmin, dmax = 4096, 4, 0, 16
    L, nb = n // B, dmax - dmin
    x, y = O.synth_iq(n, seed=12, fs=1_000_000, targets=((2, 0.0, 0.3),))
    ok, yf, w, _, _ = R.wiener_hopf_blocks(x, y, dmin, dmax, B)
    assert ok.all()
    for j in range(1, B):
        _, alone = O.wiener_hopf(x[j * L:(j + 1) * L], y[j * L:(j + 1) * L], dmin, dmax)
        d = np.abs(yf[j * L:(j + 1) * L] - alone)
        assert d[:nb - 1].max() > 1.0 and d[nb - 1:].max() <= 1e-9 * np.abs(alone).max()
    # direct evaluation of the definition at a block's first sample
    xs = R.shifted_reference(x, dmin)
    n0 = 2 * L
    direct = y[n0] - sum(w[2][k] * xs[n0 - k] for k in range(nb))
    assert abs(direct - yf[n0]) <= 1e-9 * abs(y[n0])


def test_failed_block_passes_through():
    n, B = 2048, 4
    L = n // B
    x, y = O.synth_iq(n, seed=13, fs=1_000_000, targets=((2, 0.0, 0.3),))
    x = x.copy()
    x[2 * L:3 * L] = 0
    ok, yf, w, _, _ = R.wiener_hopf_blocks(x, y, 0, 8, B)
    assert ok.tolist() == [True, True, False, True]
    assert np.array_equal(yf[2 * L:3 * L], y[2 * L:3 * L]) and not w[2].any()
    assert not np.array_equal(yf[3 * L:], y[3 * L:])


@pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(__file__), "..", "oracle", "_ref", "libblah2ref.so")),
                    reason="the compiled reference is not built")
def test_block_taps_are_the_compiled_reference():
    """The compiled reference on a block alone (nSamples = L): its filtered block determines its taps (y - y_out = w * xs on
    the block's own shifted channel, solved in the least-squares sense), which are the restatement's for that block."""
    from oracle import ref_lib
    n, B, dmin, dmax = 4096, 4, -2, 10
    L, nb = n // B, dmax - dmin
    x, y = O.synth_iq(n, seed=14, fs=1_000_000, targets=((0, 0.0, 0.3), (4, 30.0, 0.1)))
    ok, _, w, _, _ = R.wiener_hopf_blocks(x, y, dmin, dmax, B)
    assert ok.all()
    for j in range(B):
        xb, yb = x[j * L:(j + 1) * L], y[j * L:(j + 1) * L]
        ok_ref, y_ref, _ = ref_lib.wiener_hopf(xb, yb, dmin, dmax)
        assert ok_ref
        xs = R.shifted_reference(xb, dmin)
        rows = 8 * nb
        M = np.zeros((rows, nb), dtype=np.complex128)
        for k in range(nb):
            M[k:, k] = xs[:rows - k]
        w_ref = np.linalg.lstsq(M, (yb - y_ref)[:rows], rcond=None)[0]
        err = np.max(np.abs(w_ref - w[j])) / np.max(np.abs(w[j]))
        print(f"\n[blocks model vs compiled reference, block {j}] w {err:.2e}")
        assert err <= 1e-9


def test_scene_rewards_blocks():
    """A condition on the INPUTS of the GPU property test: on the drifting-clutter scene 16 blocks leave at least 12 dB
    less than one tap set per CPI (so that test cannot pass on a scene where blocks do nothing)."""
    x, y = R.drifting_scene()
    res = {}
    for B in (1, 4, 16, 32):
        ok, yf, _, _, _ = R.wiener_hopf_blocks(x, y, R.SCENE_DMIN, R.SCENE_DMAX, B)
        assert ok.all()
        res[B] = R.residual_db(yf, y)
    print("\n[blocks scene] residual dB against the input: " + ", ".join(f"B={B}: {v:.1f}" for B, v in res.items()))
    assert res[1] - res[16] >= 12.0
    assert res[1] > res[4] > res[16] > res[32]
