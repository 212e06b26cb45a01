"""CPU suite: the detectors' threshold arithmetic (blah2_amd/csrc/cfar_alpha.hpp) compiled on its own for the host with the
address and undefined-behaviour sanitizers (tests/host/emulate_cfar_alpha.cpp) against the library's blah2hip_cfar_alpha and
blah2hip_oscfar_alpha, which are built from the same header with the same libm and without fused multiply-adds: every
table bit for bit.  The tuples take every branch: one look and more, the bisection's doubling bracket at a small pfa,
rank 1 (no smaller cell), rank 1000 (no larger one), the ordered-statistic table at the size from which it starts threads
(16 entries with more than one look) and a cell-averaging table of 128 looks x 512 entries = 65 536 terms, past the 50 000
from which that one does."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CA = [(1e-3, 1, 64), (1e-3, 4, 32), (1e-6, 64, 16), (1e-3, 128, 512)]                # (pfa, looks, max_n)
OS = [(1e-3, 1, 750, 64), (1e-2, 1, 1000, 12), (1e-3, 4, 750, 16), (1e-3, 2, 1, 16)]  # (pfa, looks, rank_permille, max_n)


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """One build and one run of the program for all tuples: {tuple: (alpha[1:], rank[1:] or None)}."""
    exe = str(tmp_path_factory.mktemp("cfar_alpha") / "emulate_cfar_alpha")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "host", "emulate_cfar_alpha.cpp")])
    specs = [f"ca:{float(p).hex()}:{L}:{n}" for p, L, n in CA] + [f"os:{float(p).hex()}:{L}:{r}:{n}" for p, L, r, n in OS]
    out = subprocess.run([exe, *specs], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr  # a clean exit: no sanitizer report, no failed guard
    assert out.stderr == ""
    lines, got = out.stdout.splitlines(), {}
    for t in CA + OS:
        kind, n = lines.pop(0).split()
        assert (kind, int(n)) == ("ca" if len(t) == 3 else "os", t[-1])
        alpha = np.array([float.fromhex(v) for v in lines.pop(0).split()])
        rank = np.array([int(v) for v in lines.pop(0).split()], dtype=np.uint32) if kind == "os" else None
        assert alpha.size == t[-1]
        got[t] = (alpha, rank)
    assert not lines
    return got


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_one_look_averaging_is_the_closed_form_bit_for_bit(tables):
    pfa, looks, max_n = CA[0]
    assert looks == 1
    want = np.array([n * (math.pow(pfa, -1.0 / n) - 1) for n in range(1, max_n + 1)])
    assert np.array_equal(bits(tables[CA[0]][0]), bits(want))


@pytest.mark.parametrize("t", CA, ids=str)
def test_averaging_tables_are_the_library_s(built_lib, tables, t):
    import blah2_amd
    lib = blah2_amd.cfar_alpha_table(*t)
    assert math.isnan(lib[0])
    differ = np.flatnonzero(bits(tables[t][0]) != bits(lib[1:]))
    assert differ.size == 0, (t, differ + 1, tables[t][0][differ], lib[1:][differ])


@pytest.mark.parametrize("t", OS, ids=str)
def test_ordered_statistic_tables_are_the_library_s(built_lib, tables, t):
    import blah2_amd
    lib, rank = blah2_amd.oscfar_alpha_table(*t)
    assert math.isnan(lib[0]) and rank[0] == 0
    assert np.array_equal(tables[t][1], rank[1:])
    differ = np.flatnonzero(bits(tables[t][0]) != bits(lib[1:]))
    assert differ.size == 0, (t, differ + 1, tables[t][0][differ], lib[1:][differ])
