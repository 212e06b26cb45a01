"""CPU: the ordered-statistic detectors' tables (blah2hip_oscfar_alpha, host arithmetic of the library) and their rule as
process.py restates it (oscfar_rank, oscfar_pfa, oscfar_alpha, oscfar_hits).  No GPU is touched.

  * the tables against the closed form prod_{i<k} (n - i) / (n - i + alpha), the C table against the Python one, one look
    through the quadrature of the other looks, alpha falling with the looks, the rank rule and the refusals;
  * Monte Carlo: the false-alarm count of 4e6 independent (cell, window) draws within 4 sigma of N pfa, and the count rule
    equal to np.partition's order statistic on every draw;
  * the restatement on a flat map (ties at every rank), at ranks 1 and 1000 per mille, 1-D window against (g, t, 0, 0);
  * the masking scene the GPU module repeats: three equal echoes four cells apart, where the cell-averaging detector loses
    the middle one and the ordered-statistic detector keeps it.
"""
import math

import numpy as np
import pytest

from oracle import blah2_oracle as O


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    return blah2_amd


def permille_for(b2, n, k):
    return next(p for p in range(1, 1001) if b2.oscfar_rank(n, p) == k)


CLOSED = [(12, 9, 1e-2, 4.862449608914), (16, 12, 1e-3, 7.421411314149), (7, 6, 2e-2, 3.632036163585),
          (254, 191, 1e-5, None), (5, 5, 1e-3, None), (5, 1, 1e-3, None)]


@pytest.mark.parametrize("n,k,pfa,value", CLOSED)
def test_table_back_substitutes_into_the_closed_form(b2, n, k, pfa, value):
    alpha, rank = b2.oscfar_alpha_table(pfa, 1, permille_for(b2, n, k), n)
    assert math.isnan(alpha[0]) and rank[0] == 0 and rank[n] == k
    prod = 1.0
    for i in range(k):
        prod *= (n - i) / (n - i + alpha[n])
    assert abs(prod - pfa) < 1e-10, (prod, pfa)
    assert abs(b2.oscfar_pfa(alpha[n], n, k) - pfa) < 1e-10
    if value is not None:
        assert abs(alpha[n] - value) < 1e-11 * value, alpha[n]


def test_c_and_python_tables_agree(b2):
    grid = [1, 2, 3, 5, 8, 12, 16, 31, 64, 153, 254, 300]
    for pfa, pm in ((1e-3, 750), (1e-6, 500), (2e-2, 1000), (1e-2, 1)):
        ca, cr = b2.oscfar_alpha_table(pfa, 1, pm, max(grid))
        for n in grid:
            pa, pr = b2.oscfar_alpha(pfa, 1, pm, n)
            assert pr[n] == cr[n] == b2.oscfar_rank(n, pm)
            assert abs(pa[n] - ca[n]) <= 1e-12 * ca[n], (pfa, pm, n, pa[n], ca[n])
    # more looks: the quadrature on both sides
    ca, cr = b2.oscfar_alpha_table(1e-3, 4, 750, 16)
    pa, pr = b2.oscfar_alpha(1e-3, 4, 750, 16)
    assert np.array_equal(cr, pr) and math.isnan(ca[0]) and math.isnan(pa[0])
    assert np.max(np.abs(pa[1:] / ca[1:] - 1.0)) <= 1e-12
    ca, _ = b2.oscfar_alpha_table(1e-4, 16, 600, 12)
    pa, _ = b2.oscfar_alpha(1e-4, 16, 600, 12)
    assert abs(pa[12] / ca[12] - 1.0) <= 1e-12


def test_one_look_through_the_quadrature(b2):
    for n, k, pfa, _ in CLOSED:
        if n > 20:
            continue
        pm = permille_for(b2, n, k)
        closed, _ = b2.oscfar_alpha_table(pfa, 1, pm, n)
        quad, _ = b2.oscfar_alpha(pfa, 1, pm, n, quadrature=True)
        assert abs(quad[n] / closed[n] - 1.0) <= 1e-9, (n, k, quad[n], closed[n])
        assert abs(b2.oscfar_pfa(closed[n], n, k, 1, quadrature=True) / pfa - 1.0) <= 1e-9


def test_alpha_falls_with_the_looks(b2):
    a = [b2.oscfar_alpha_table(1e-3, L, 750, 16)[0][16] for L in (1, 2, 4, 8)]
    assert all(x > y for x, y in zip(a, a[1:])), a
    assert abs(a[0] - 7.42) < 0.01 and abs(a[2] - 2.992) < 0.001, a
    # the table's own quadrature back-substitutes
    assert abs(b2.oscfar_pfa(a[2], 16, 12, 4) / 1e-3 - 1.0) < 1e-9


def test_rank_rule(b2):
    for n in (1, 2, 7, 12, 153, 254):
        assert b2.oscfar_rank(n, 1000) == n and b2.oscfar_rank(n, 1) == 1
    assert b2.oscfar_rank(12, 750) == 9 and b2.oscfar_rank(16, 750) == 12 and b2.oscfar_rank(13, 750) == 10
    _, rank = b2.oscfar_alpha_table(1e-3, 1, 750, 254)
    assert [int(r) for r in rank] == [0] + [b2.oscfar_rank(n, 750) for n in range(1, 255)]
    with pytest.raises(ValueError):
        b2.oscfar_rank(5, 0)
    with pytest.raises(ValueError):
        b2.oscfar_rank(5, 1001)


def test_refusals(b2):
    from blah2_amd import _lib
    from blah2_amd.process import _ptr
    L = _lib.load()
    out, rk = np.zeros(4), np.zeros(4, dtype=np.uint32)
    p, r = _ptr(out), _ptr(rk)
    assert L.blah2hip_oscfar_alpha(1e-3, 1, 750, 3, None, r) == _lib.ERR_INVALID
    assert L.blah2hip_oscfar_alpha(1e-3, 0, 750, 3, p, r) == _lib.ERR_INVALID
    assert L.blah2hip_oscfar_alpha(1e-3, _lib.MAX_CFAR_LOOKS + 1, 750, 3, p, r) == _lib.ERR_INVALID
    assert L.blah2hip_oscfar_alpha(1e-3, 1, 0, 3, p, r) == _lib.ERR_INVALID
    assert L.blah2hip_oscfar_alpha(1e-3, 1, 1001, 3, p, r) == _lib.ERR_INVALID
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        for looks in (1, 2):
            assert L.blah2hip_oscfar_alpha(bad, looks, 750, 3, p, r) == _lib.ERR_INVALID, bad
    assert b"pfa" in L.blah2hip_last_error()
    assert L.blah2hip_oscfar_alpha(1e-3, 1, 750, 3, p, None) == _lib.OK  # the ranks are optional
    assert math.isnan(out[0]) and (out[1:] > 0).all()
    assert L.blah2hip_oscfar_alpha(1e-3, 2, 1000, 3, p, r) == _lib.OK and rk.tolist() == [0, 1, 2, 3]


MC = [(1, 16, 1e-3), (1, 12, 1e-2), (4, 16, 1e-3)]


@pytest.mark.parametrize("looks,n,pfa", MC)
def test_monte_carlo_false_alarms(b2, looks, n, pfa):
    """4e6 independent (cell, window) draws of noise: the false alarms lie within 4 sqrt(N pfa) of N pfa, and the count rule
    is np.partition's decision on every draw."""
    N, chunk = 4_000_000, 500_000
    k = b2.oscfar_rank(n, 750)
    assert k == {12: 9, 16: 12}[n]
    alpha = b2.oscfar_alpha_table(pfa, looks, 750, n)[0][n]
    rng = np.random.default_rng(20261020 + 97 * looks + n)
    alarms = 0
    for _ in range(N // chunk):
        x = rng.standard_gamma(float(looks), (chunk, n + 1))
        cell, train = x[:, 0], x[:, 1:]
        by_count = (alpha * train < cell[:, None]).sum(axis=1) >= k
        kth = np.partition(train, k - 1, axis=1)[:, k - 1]
        assert np.array_equal(by_count, cell > alpha * kth)
        alarms += int(by_count.sum())
    sigma = math.sqrt(N * pfa)
    print(f"L={looks} n={n} pfa={pfa}: {alarms} false alarms, {(alarms - N * pfa) / sigma:+.2f} sigma")
    assert abs(alarms - N * pfa) <= 4.0 * sigma, (alarms, N * pfa)


def flat_case(b2, w, pm, plant):
    nD, nC = 9, 40
    m = np.ones((nD, nC), dtype=np.complex64)
    for (i, j), v in plant.items():
        m[i, j] = v
    delay, doppler = np.arange(nC) - 3, np.arange(nD) - 4.0
    w4 = w if len(w) == 4 else (w[0], w[1], 0, 0)
    max_n = (2 * (w4[0] + w4[1]) + 1) * (2 * (w4[2] + w4[3]) + 1)
    alpha, rank = b2.oscfar_alpha_table(1e-3, 1, pm, max_n)
    r, c, s = b2.oscfar_hits(m, delay, doppler, 1.5, alpha, rank, w, -128, 0.0)
    return m, alpha, rank, list(zip(r.tolist(), c.tolist())), s


def test_restatement_on_a_flat_map(b2):
    """Every power equal: no cell is above alpha times another (alpha > 1), whatever the rank.  A planted cell hits once it
    exceeds alpha[n] times the floor, its neighbours do not, and a second planted cell in its window costs one rank."""
    for pm in (1, 500, 750, 1000):
        m, alpha, rank, hits, _ = flat_case(b2, (2, 6), pm, {})
        assert hits == [] and (alpha[1:] > 1).all()
    amp = np.float32(10.0)  # power 100, above every alpha[n] of this table
    m, alpha, rank, hits, snr = flat_case(b2, (2, 6), 750, {(4, 20): amp})
    assert alpha[12] < 100.0 and hits == [(4, 20)]
    assert abs(snr[0] - (5.0 * math.log10(100.0) - 1.5)) < 1e-12
    # column 1 has 6 training cells behind it and none in front (column 0 never trains); column 0 has 6 as well
    m, alpha, rank, hits, _ = flat_case(b2, (2, 6), 750, {(0, 0): amp, (0, 1): amp, (8, 39): amp})
    assert hits == [(0, 0), (0, 1), (8, 39)]
    # rank 1000: every training cell must lie below, so one equal neighbour in the window masks; rank 750 keeps both
    plant = {(4, 20): amp, (4, 24): amp}
    assert flat_case(b2, (2, 6), 1000, plant)[3] == []
    assert flat_case(b2, (2, 6), 750, plant)[3] == [(4, 20), (4, 24)]
    # rank 1: one training cell below is enough, and alpha is that of the smallest of n
    m, alpha, rank, hits, _ = flat_case(b2, (2, 6), 1, {(4, 20): np.float32(300.0)})
    assert (rank[1:] == 1).all() and hits == [(4, 20)]
    # special values: a NaN or +Inf training cell costs a rank, a NaN cell under test never hits, a +Inf cell does
    plant = {(4, 20): amp, (4, 24): np.complex64(complex(np.nan, 0)), (4, 17): np.complex64(complex(np.inf, 0))}
    assert flat_case(b2, (2, 6), 750, plant)[3] == [(4, 17), (4, 20)]
    assert flat_case(b2, (2, 6), 1000, plant)[3] == []
    m = np.zeros((5, 30), dtype=np.complex64)
    alpha, rank = b2.oscfar_alpha_table(1e-3, 1, 750, 12)
    assert b2.oscfar_hits(m, np.arange(30), np.arange(5.0), 0.0, alpha, rank, (2, 6))[0].size == 0


def test_one_d_window_is_the_two_d_window_without_doppler_cells(b2):
    rng = np.random.default_rng(11)
    nD, nC = 13, 57
    m = (np.sqrt(rng.exponential(1.0, (nD, nC))) * np.exp(2j * np.pi * rng.uniform(0, 1, (nD, nC)))).astype(np.complex64)
    m[rng.integers(0, nD, 30), rng.integers(0, nC, 30)] *= 30
    delay, doppler = np.arange(nC) - 5, (np.arange(nD) - 6) * 0.5
    for g, t in ((2, 6), (0, 1), (3, 20), (1, 60)):
        alpha, rank = b2.oscfar_alpha_table(2e-2, 1, 750, 2 * t + 1 + 2 * g)
        one = b2.oscfar_hits(m, delay, doppler, 2.0, alpha, rank, (g, t), -2, 1.0)
        two = b2.oscfar_hits(m, delay, doppler, 2.0, alpha, rank, (g, t, 0, 0), -2, 1.0)
        assert all(np.array_equal(a, b) for a, b in zip(one, two)) and one[0].size > 0
        assert (delay[one[1]] >= -2).all() and (np.abs(doppler[one[0]]) >= 1.0).all()


def masking_scene(n_rows=1, n_cols=40):
    """A flat unit floor with three cells of power 10^1.5 four apart in every row; the middle one is at column 20."""
    m = np.ones((n_rows, n_cols), dtype=np.complex64)
    for j in (16, 20, 24):
        m[:, j] = np.float32(10.0 ** 0.75)
    return m


def test_masking_scene(b2):
    """Guard 2, train 6, pfa 1e-3: the echoes at +-4 sit in the middle cell's training window.  Cell averaging: margin
    p / threshold ~ 0.55, a miss.  Ordered statistic at 750 per mille: the 9th smallest of 12 is floor, margin ~ 3.7."""
    m = masking_scene()
    delay, doppler = np.arange(40), np.array([5.0])
    p = float(np.float64(m[0, 20].real) ** 2)
    dl, _, _ = O.cfar1d(m, delay, doppler, 0.0, 1e-3, 2, 6, -128, 0.0)
    assert 20.0 not in dl.tolist()
    ca_margin = p / (12 * (1e-3 ** (-1.0 / 12) - 1) * ((10 + 2 * p) / 12))
    assert abs(ca_margin - 0.55) < 0.01 and ca_margin < 1 / 1.2
    alpha, rank = b2.oscfar_alpha_table(1e-3, 1, 750, 12)
    r, c, _ = b2.oscfar_hits(m, delay, doppler, 0.0, alpha, rank, (2, 6))
    assert (0, 20) in list(zip(r.tolist(), c.tolist()))
    os_margin = p / (alpha[12] * 1.0)  # the 9th smallest of the window's 12 cells is floor
    assert rank[12] == 9 and abs(os_margin - 3.7) < 0.1 and os_margin > 1.2
