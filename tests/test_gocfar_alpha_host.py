"""CPU suite: the greatest-of / smallest-of threshold arithmetic (blah2_amd/csrc/cfar_alpha.hpp: goso_pfa, goso_alpha_fill)
compiled on its own for the host with the address and undefined-behaviour sanitizers (tests/host/emulate_gocfar_alpha.cpp)
against the library's blah2hip_gocfar_alpha and the pure-Python restatement gocfar_alpha, to 1e-12 relative; the known
answers of include/blah2hip.h, the closed forms at a = b = 1, the textbook sum for equal halves, back-substitution,
symmetry, the averaging value where one half is empty, every refusal, and a Monte Carlo of the rule itself."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO, SO = 1, 2
SIZES = (1, 2, 3, 8, 16, 127)
GRID = [(a, b) for a in SIZES for b in SIZES]
GRID_PFAS = (1e-2, 1e-4, 1e-8)
KNOWN = [  # (a, b, pfa, GO, SO): include/blah2hip.h
    (8, 8, 1e-3, 7.487313, 12.599715),
    (3, 8, 1e-3, 8.211435, 27.069698),
    (16, 5, 1e-2, 4.502739, 7.845986),
    (1, 1, 1e-3, (-3 + math.sqrt(8001)) / 2, 1998.0),
    (1960, 1960, 1e-6, 13.673908, 14.028149),
]
EDGE = [(0, 5), (7, 0), (0, 0), (1, 127), (40, 0)]
LONG = [(100 + k, 150) for k in range(100)]  # 30 000 terms: past the 20 000 from which the filler starts threads


def specs():
    """[(kind, pfa, pairs)] -- every list the program and the library are asked for."""
    out = []
    for kind in (GO, SO):
        out += [(kind, pfa, GRID) for pfa in GRID_PFAS]
        out += [(kind, pfa, [(a, b)]) for a, b, pfa, _, _ in KNOWN]
        out += [(kind, 1e-3, EDGE), (kind, 1e-3, LONG)]
    return out


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """One build and one run of the program for all lists: [alpha per spec]."""
    exe = str(tmp_path_factory.mktemp("gocfar_alpha") / "emulate_gocfar_alpha")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "host", "emulate_gocfar_alpha.cpp")])
    args = [":".join([str(k), float(p).hex()] + [f"{a},{b}" for a, b in pairs]) for k, p, pairs in specs()]
    out = subprocess.run([exe, *args], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr  # a clean exit: no sanitizer report, no failed guard
    assert out.stderr == ""
    lines, got = out.stdout.splitlines(), []
    for k, p, pairs in specs():
        assert lines.pop(0) == f"go {len(pairs)}"
        got.append(np.array([math.nan if v == "nan" else float.fromhex(v) for v in lines.pop(0).split()]))
        assert got[-1].size == len(pairs)
    assert not lines
    return got


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    return blah2_amd


def lib_table(b2, kind, pfa, pairs):
    return b2.gocfar_alpha_table(pfa, kind, [a for a, _ in pairs], [b for _, b in pairs])


def close(x, y, rel):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return bool(np.all((np.isnan(x) & np.isnan(y)) | (np.abs(x - y) <= rel * np.abs(y))))


def test_program_and_library_agree(b2, tables):
    for (kind, pfa, pairs), alpha in zip(specs(), tables):
        lib = lib_table(b2, kind, pfa, pairs)
        assert close(alpha, lib, 1e-12), (kind, pfa, pairs[:4], alpha[:4], lib[:4])


def test_python_restatement_agrees(b2, tables):
    n = 0
    for (kind, pfa, pairs), alpha in zip(specs(), tables):
        if pairs is LONG:
            pairs, alpha = pairs[::25], alpha[::25]
        py = [b2.gocfar_alpha(pfa, kind, a, b) for a, b in pairs]
        assert close(py, alpha, 1e-12), (kind, pfa, pairs[:4], py[:4], alpha[:4])
        n += len(pairs)
    assert n > 200


def test_known_answers(b2):
    for a, b, pfa, go, so in KNOWN:
        got = (lib_table(b2, GO, pfa, [(a, b)])[0], lib_table(b2, SO, pfa, [(a, b)])[0])
        assert abs(got[0] - go) <= 1e-6 and abs(got[1] - so) <= 1e-6, (a, b, pfa, got, go, so)
    # cell averaging over the 16 cells, for comparison
    assert abs(b2.cfar_alpha_table(1e-3, 1, 16)[16] - 8.638824) <= 1e-6


@pytest.mark.parametrize("pfa", [1e-2, 1e-3, 1e-6])
def test_closed_forms_for_one_cell_each_side(b2, pfa):
    """a = b = 1: Pfa_SO = 2 / (2 + alpha), Pfa_GO = 2 / ((1 + alpha)(2 + alpha))."""
    go, so = lib_table(b2, GO, pfa, [(1, 1)])[0], lib_table(b2, SO, pfa, [(1, 1)])[0]
    assert abs(so - (2.0 / pfa - 2.0)) <= 1e-12 * so
    assert abs(go - (-3.0 + math.sqrt(1.0 + 8.0 / pfa)) / 2.0) <= 1e-12 * go


@pytest.mark.parametrize("n", [1, 2, 3, 8, 16])
def test_equal_halves_are_the_textbook_sum(b2, n):
    for alpha in (0.5, 4.0, 11.0, 40.0):
        so = 2.0 * sum(math.comb(n - 1 + k, k) * (2.0 + alpha / n) ** -(n + k) for k in range(n))
        both = 2.0 * (1.0 + alpha / n) ** -n
        go = both - so
        assert abs(b2.gocfar_pfa(alpha, "so", n, n) - so) <= 1e-12 * so
        assert abs(b2.gocfar_pfa(alpha, "go", n, n) - go) <= 1e-12 * both  # a difference: relative to its larger term


def exact_pfa(alpha, kind, a, b):
    """The formulas of include/blah2hip.h in exact rational arithmetic on the double ``alpha``."""
    from fractions import Fraction as F

    def T(a, b):
        s = 1 + (F(alpha) + b) / a
        return sum(math.comb(a - 1 + j, j) * F(b, a) ** j / s ** (a + j) for j in range(b))

    so = T(a, b) + T(b, a)
    return so if kind == SO else (1 + F(alpha) / a) ** -a + (1 + F(alpha) / b) ** -b - so


def test_back_substitution(b2):
    """alpha into the restatement AND into the textbook expressions evaluated exactly: both within 1e-10 of pfa."""
    worst = 0.0
    for kind in (GO, SO):
        for pfa in GRID_PFAS:
            for (a, b), alpha in zip(GRID, lib_table(b2, kind, pfa, GRID)):
                back = b2.gocfar_pfa(alpha, kind, a, b)
                assert abs(back - pfa) <= 1e-10 * pfa, (kind, pfa, a, b, alpha, back)
                exact = float(exact_pfa(float(alpha), kind, a, b) / pfa) - 1.0
                worst = max(worst, abs(back / pfa - 1.0), abs(exact))
                assert abs(exact) <= 1e-10, (kind, pfa, a, b, alpha, exact)
    print("worst relative back-substitution error", worst)


def test_symmetry(b2):
    for kind in (GO, SO):
        for pfa in GRID_PFAS:
            t = dict(zip(GRID, lib_table(b2, kind, pfa, GRID)))
            for a, b in GRID:
                assert t[(a, b)] == t[(b, a)], (kind, pfa, a, b)
            assert b2.gocfar_alpha(pfa, kind, 3, 16) == b2.gocfar_alpha(pfa, kind, 16, 3)


def test_ordering_against_cell_averaging(b2):
    """Smallest-of needs the highest factor and greatest-of the lowest; the averaging factor over all the cells lies between."""
    for a, b in ((8, 8), (3, 8), (16, 5), (1, 1)):
        ca = b2.cfar_alpha_table(1e-3, 1, a + b)[a + b]
        assert lib_table(b2, GO, 1e-3, [(a, b)])[0] < ca < lib_table(b2, SO, 1e-3, [(a, b)])[0]


def test_an_empty_half_gets_the_averaging_value(b2, tables):
    for kind in (GO, SO):
        for pfa in (1e-3, 0.2):
            t = lib_table(b2, kind, pfa, EDGE)
            ca = b2.cfar_alpha_table(pfa, 1, 127)
            for (a, b), v in zip(EDGE, t):
                if a and b:
                    continue
                assert (math.isnan(v) and a + b == 0) or v == ca[a + b], (kind, pfa, a, b, v)
            assert math.isnan(b2.gocfar_alpha(pfa, kind, 0, 0)) and b2.gocfar_alpha(pfa, kind, 0, 5) == ca[5]


def test_refusals(b2, built_lib):
    from blah2_amd import _lib
    a = np.array([3, 8], dtype=np.uint32)
    b = np.array([8, 3], dtype=np.uint32)
    out = np.full(2, -7.0)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    f = built_lib.blah2hip_gocfar_alpha
    assert f(1e-3, GO, 2, vp(a), vp(b), vp(out)) == _lib.OK and out[0] == out[1] > 0
    out[:] = -7.0
    for args in ((1e-3, GO, 2, None, vp(b), vp(out)), (1e-3, GO, 2, vp(a), None, vp(out)), (1e-3, SO, 2, vp(a), vp(b), None),
                 (1e-3, 0, 2, vp(a), vp(b), vp(out)), (1e-3, 3, 2, vp(a), vp(b), vp(out)),
                 (0.0, GO, 2, vp(a), vp(b), vp(out)), (1.0, SO, 2, vp(a), vp(b), vp(out)), (-0.5, GO, 2, vp(a), vp(b), vp(out)),
                 (math.nan, SO, 2, vp(a), vp(b), vp(out))):
        assert f(*args) == _lib.ERR_INVALID, args[:3]
        assert (out == -7.0).all()
    for bad in (("xo", 3, 8), (0, 3, 8), (3, 3, 8), (True, 3, 8)):
        with pytest.raises(ValueError):
            b2.gocfar_alpha(1e-3, *bad)
    for pfa in (0.0, 1.0):
        with pytest.raises(ValueError):
            b2.gocfar_alpha(pfa, "go", 3, 8)
    with pytest.raises(ValueError):
        b2.gocfar_pfa(1.0, "go", 0, 8)


@pytest.mark.parametrize("a,b", [(8, 8), (3, 8), (1, 8), (16, 5)])
def test_monte_carlo(b2, a, b):
    """4e6 draws of the rule under unit-power noise: the measured rate within 4 binomial standard deviations of pfa."""
    N = 4_000_000
    rng = np.random.default_rng(20261021 + 1000 * a + b)
    cell = rng.exponential(1.0, N)
    mu_a = rng.gamma(a, 1.0, N) / a
    mu_b = rng.gamma(b, 1.0, N) / b
    for pfa in (1e-2, 1e-3):
        sd = math.sqrt(pfa * (1.0 - pfa) / N)
        for kind in (GO, SO):
            alpha = lib_table(b2, kind, pfa, [(a, b)])[0]
            hA, hB = cell > alpha * mu_a, cell > alpha * mu_b
            rate = float(np.mean(hA & hB if kind == GO else hA | hB))
            print(f"a {a} b {b} pfa {pfa} kind {kind}: alpha {alpha:.6f} rate {rate:.3e} ({(rate - pfa) / sd:+.2f} sd)")
            assert abs(rate - pfa) <= 4.0 * sd, (a, b, pfa, kind, rate)
