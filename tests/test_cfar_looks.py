"""CPU: the detectors' threshold factors for cells that are sums of L looks (blah2hip_cfar_alpha, host arithmetic of the
library: no GPU is touched, like the helpers of tests/test_abi.py).

A cell of the sum of L looks of noise is Gamma(L), the sum of n training cells Gamma(nL); with the threshold
alpha (tot / n), t = alpha / n and m = nL

    Pfa(t) = sum_{k<L} C(m+k-1, k) t^k / (1+t)^(m+k)

Checks: one look is the reference's closed form bit for bit; the table solves Pfa(t) = pfa -- exactly, in rational
arithmetic, for three tuples (bound 1e-12 of pfa; the pure-Python restatement measured 1.4e-15), and through the
restatement's fp64 Pfa on a grid up to L = 1024, n = 2048 (bound 1e-10; the restatement alone measured 4.5e-13); alpha falls
strictly with L and with n; and a seeded Monte Carlo of 4e6 Gamma draws lands within 5 binomial sigma of N pfa (measured
-0.03 and +0.35 sigma), where the one-look factor gives under a tenth of it (measured 0 and 3527 of 40000).
"""
import math
from fractions import Fraction

import numpy as np
import pytest

LOOKS = (2, 4, 8, 64, 128, 1024)
TRAIN = (1, 2, 8, 16, 200, 2048)
PFAS = (1e-2, 1e-3, 1e-6)


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    return blah2_amd


_tables = {}


def table(b2, pfa, looks, max_n):
    """The library's table, computed once per (pfa, looks) at the largest size any test asks for and left unchanged."""
    key = (pfa, looks)
    if key not in _tables or _tables[key].size <= max_n:
        _tables[key] = b2.cfar_alpha_table(pfa, looks, max_n)
    return _tables[key]


def pfa_exact(t, n, L):
    """Pfa(t) in rational arithmetic for the double t."""
    t, m = Fraction(t), n * L
    s, c = Fraction(0), Fraction(1)
    for k in range(L):
        if k:
            c = c * (m + k - 1) / k
        s += c * t ** k / (1 + t) ** (m + k)
    return s


@pytest.mark.parametrize("pfa", [1e-2, 1e-5])
def test_one_look_is_the_closed_form_bit_for_bit(b2, pfa):
    a = b2.cfar_alpha_table(pfa, 1, 64)
    assert math.isnan(a[0])
    want = np.array([n * (math.pow(pfa, -1.0 / n) - 1) for n in range(1, 65)])
    assert np.array_equal(a[1:].view(np.uint64), want.view(np.uint64))
    # ... and so is the pure-Python restatement
    assert np.array_equal(b2.cfar_alpha(pfa, 1, 64)[1:].view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("pfa,L,n", [(1e-3, 4, 8), (1e-6, 8, 16), (1e-2, 16, 2)])
def test_the_table_solves_the_exact_equation(b2, pfa, L, n):
    a = table(b2, pfa, L, n)
    assert math.isnan(a[0])
    rel = float(pfa_exact(float(a[n]) / n, n, L) / Fraction(pfa) - 1)
    print(f"pfa={pfa} L={L} n={n}: alpha={a[n]!r}, exact Pfa / pfa - 1 = {rel:.3e}")
    assert abs(rel) <= 1e-12
    assert a[n] == b2.cfar_alpha(pfa, L, n)[n]  # the restatement is the same arithmetic
    if (pfa, L, n) == (1e-3, 4, 8):
        assert abs(a[n] - 3.824166284355) <= 1e-9
        # the one-look factor the detectors used on such a sum: far too high
        assert abs(b2.cfar_alpha_table(pfa, 1, n)[n] - 10.97) < 0.01


def test_the_table_back_substitutes_on_the_grid_and_falls_with_looks_and_cells(b2):
    worst = 0.0
    for pfa in PFAS:
        grid = np.empty((len(LOOKS), len(TRAIN)))
        for i, L in enumerate(LOOKS):
            a = table(b2, pfa, L, max(TRAIN))
            for j, n in enumerate(TRAIN):
                back = b2.cfar_pfa(a[n], n, L)
                worst = max(worst, abs(back - pfa) / pfa)
                assert abs(back - pfa) <= 1e-10 * pfa, (pfa, L, n, back)
                grid[i, j] = a[n]
        assert (np.diff(grid, axis=0) < 0).all(), pfa  # more looks: a lower factor
        assert (np.diff(grid, axis=1) < 0).all(), pfa  # more training cells: a lower factor
        one = b2.cfar_alpha_table(pfa, 1, max(TRAIN))
        assert (grid[0] < one[list(TRAIN)]).all(), pfa
    print(f"largest |Pfa(alpha) / pfa - 1| on the grid: {worst:.3e}")


@pytest.mark.parametrize("L,n,pfa", [(4, 8, 1e-3), (2, 16, 1e-2)])
def test_monte_carlo_false_alarm_rate(b2, L, n, pfa):
    N = 4_000_000
    rng = np.random.default_rng(20250 + L)
    cell = rng.gamma(L, 1.0, N)
    train = rng.gamma(n * L, 1.0, N)
    a = table(b2, pfa, L, n)[n]
    fa = int((cell > a * (train / n)).sum())
    sigma = math.sqrt(N * pfa * (1 - pfa))
    one = int((cell > b2.cfar_alpha_table(pfa, 1, n)[n] * (train / n)).sum())
    print(f"L={L} n={n} pfa={pfa}: {fa} false alarms of {N * pfa:.0f} expected ({(fa - N * pfa) / sigma:+.2f} sigma); "
          f"the one-look factor: {one}")
    assert abs(fa - N * pfa) <= 5 * sigma
    assert one < 0.1 * N * pfa


def test_refusals_and_the_python_constants(b2):
    from blah2_amd import _lib
    L = _lib.load()
    out = np.zeros(4)
    p = out.ctypes.data
    assert L.blah2hip_cfar_alpha(1e-3, 0, 3, p) == _lib.ERR_INVALID
    assert L.blah2hip_cfar_alpha(1e-3, _lib.MAX_CFAR_LOOKS + 1, 3, p) == _lib.ERR_INVALID
    assert L.blah2hip_cfar_alpha(1e-3, 2, 3, None) == _lib.ERR_INVALID
    for bad in (0.0, 1.0, -1e-3, float("nan")):
        assert L.blah2hip_cfar_alpha(bad, 2, 3, p) == _lib.ERR_INVALID, bad
    assert (out == 0).all()
    assert L.blah2hip_cfar_alpha(1e-3, _lib.MAX_CFAR_LOOKS, 3, p) == _lib.OK and math.isnan(out[0]) and (out[1:] > 0).all()
    assert _lib.OPT_CFAR_LOOKS == 13 and _lib.NK_NCI == 0 and _lib.NCI_KERNEL_NAMES[_lib.NK_NCI] == "nci"
