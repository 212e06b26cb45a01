"""CPU suite: the ticketed pulse walk of rangew1k_kernel (blah2_amd/csrc/range_walk.hpp), compiled for the host with the
address and undefined-behaviour sanitizers and pulled the way the kernel pulls it, in adversarial orders
(tests/host/emulate_range_walk.cpp): nPulses 1, 5, 11, 12, 13, 95, 96, 97, 603, 1026, 131 328 against grids
1, 2, 3, 7, 8, 9, 16, 24, 256, five orders of the pulls each."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PULSES = [1, 5, 11, 12, 13, 95, 96, 97, 603, 1026, 131_328]
GRIDS = [1, 2, 3, 7, 8, 9, 16, 24, 256]
ORDERS = 5


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rwalk") / "emulate_range_walk")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "host", "emulate_range_walk.cpp")])
    return exe


def test_every_pulse_once_and_every_wave_ends(emu):
    """The program's own checks: every pulse handed out exactly once in every order of the pulls, every wave ends, an
    exhausted wave stays exhausted, the exit word closes the launch once and the nine words are zero afterwards; with no
    skew the first min(grid, blocks) blocks go to the workgroups that own them in the static walk."""
    out = subprocess.run([emu], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == ["ok", str(len(PULSES) * len(GRIDS) * ORDERS)]


def _walk(exe, G, N, order):
    out = subprocess.run([exe, str(G), str(N), str(order)], capture_output=True, text=True, check=True)
    return np.array([[int(v) for v in ln.split()] for ln in out.stdout.splitlines()]).reshape(-1, 3)


@pytest.mark.parametrize("G,N", [(1, 97), (3, 97), (7, 603), (8, 603), (9, 1026), (24, 95), (256, 1026), (2, 5)])
@pytest.mark.parametrize("order", range(ORDERS))
def test_the_printed_walk(emu, G, N, order):
    """The same once more from the printed hand-outs, in numpy: a permutation of the pulses, by waves of the grid only.
    Grids below 8 leave heads no workgroup starts at: their pulses come up all the same."""
    w = _walk(emu, G, N, order)
    assert sorted(w[:, 2]) == list(range(N))
    assert w[:, 0].min() >= 0 and w[:, 0].max() < G and w[:, 1].min() >= 0 and w[:, 1].max() < 12
    if G < 8:  # blocks of the heads G .. 7 exist from 12 G pulses on and were taken by somebody
        orphan = (w[:, 2] // 12) % 8 >= G
        assert orphan.any() == (N > 12 * G)


@pytest.mark.parametrize("G,N", [(8, 603), (9, 1026), (256, 131_328), (3, 30), (16, 97)])
def test_no_skew_keeps_the_static_first_round(emu, G, N):
    """Order 0 (all waves in step): wave w of workgroup b starts on pulse 12 b + w, as in the static walk, and while every
    head has work a workgroup stays on the blocks of its own head."""
    w = _walk(emu, G, N, 0)
    first = {}
    for b, wave, pulse in w:
        first.setdefault((b, wave), pulse)
    for (b, wave), pulse in first.items():
        if 12 * b + wave < N:
            assert pulse == 12 * b + wave, (b, wave, pulse)
    if G % 8 == 0 and N % 96 == 0:  # equal shares: nobody ever leaves its head
        assert np.all((w[:, 2] // 12) % 8 == w[:, 0] % 8)


def test_headline_launch_shares(emu):
    """131 328 pulses on 3072 waves in step: 42 or 43 pulses each, as with the static walk."""
    w = _walk(emu, 256, 131_328, 0)
    counts = np.bincount(w[:, 0] * 12 + w[:, 1], minlength=3072)
    assert counts.min() >= 42 and counts.max() <= 43 and counts.sum() == 131_328
