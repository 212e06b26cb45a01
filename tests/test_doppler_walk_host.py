"""CPU suite: the tile walk of the persistent Doppler kernels at nD <= 513 (blah2_amd/csrc/doppler_walk.hpp), compiled
for the host with the address and undefined-behaviour sanitizers and walked the way the kernels walk it
(tests/host/emulate_walk.cpp): every grid 1 ... 64 and every multiple of 8 up to 512 against the tile counts
1, 7, 19, 56, 57, 511, 512, 513, 6656."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRIDS = list(range(1, 65)) + list(range(72, 513, 8))
TILES = [1, 7, 19, 56, 57, 511, 512, 513, 6656]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("walk") / "emulate_walk")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "host", "emulate_walk.cpp")])
    return exe


def test_every_grid_and_tile_count(emu):
    """The program's own checks: every tile exactly once, increasing per workgroup, none after none, consecutive tiles
    per label and iteration on grids divisible by 8, b + k G on the others."""
    out = subprocess.run([emu], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == ["ok", str(len(GRIDS) * len(TILES))]


def _walk(exe, G, T):
    out = subprocess.run([exe, str(G), str(T)], capture_output=True, text=True, check=True)
    return np.array([[int(v) for v in ln.split()] for ln in out.stdout.splitlines()]).reshape(-1, 3)


@pytest.mark.parametrize("G,T", [(8, 57), (16, 57), (24, 57), (56, 57), (16, 52), (64, 7), (512, 6656), (504, 6656), (8, 1)])
def test_xcd_local_grids_from_the_printed_walk(emu, G, T):
    """The same properties once more, from the printed map and in numpy (independent of the program's checks)."""
    w = _walk(emu, G, T)
    assert sorted(w[:, 2]) == list(range(T))
    for b in range(G):
        mine = w[w[:, 0] == b]
        assert list(mine[:, 1]) == list(range(len(mine))) and np.all(np.diff(mine[:, 2]) > 0)
    for k in range(w[:, 1].max() + 1):
        for x in range(8):
            g = w[(w[:, 1] == k) & (w[:, 0] % 8 == x)]
            g = g[np.argsort(g[:, 0])]
            assert np.all(np.diff(g[:, 2]) == 1), (k, x)
            assert list(g[:, 0]) == list(range(x, x + 8 * len(g), 8))  # the label's first workgroups, none skipped
    for x in range(8):  # a label keeps one contiguous range: its iterations continue where it left off
        g = w[w[:, 0] % 8 == x]
        g = g[np.lexsort((g[:, 0], g[:, 1]))]
        assert np.all(np.diff(g[:, 2]) == 1), x


@pytest.mark.parametrize("G,T", [(5, 57), (19, 19), (4, 57), (63, 6656), (1, 7)])
def test_other_grids_keep_the_strided_walk(emu, G, T):
    w = _walk(emu, G, T)
    assert np.array_equal(w[:, 2], w[:, 0] + w[:, 1] * G) and sorted(w[:, 2]) == list(range(T))


def test_headline_launch_is_balanced(emu):
    """configs[1] x 256 CPIs on 512 workgroups: 13 tiles each, as with the strided walk."""
    w = _walk(emu, 512, 6656)
    assert np.all(np.bincount(w[:, 0], minlength=512) == 13)
