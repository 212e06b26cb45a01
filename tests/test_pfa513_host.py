"""CPU suite: the 513-point prime-factor transform of fft_pfa513.hpp, compiled for the host and run
lane by lane (tests/host/emulate_pfa513.cpp), against numpy.fft."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pfa") / "emulate_pfa513")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "emulate_pfa513.cpp")])
    return exe


def _run(emu, tmp_path, x):
    x = x.astype(np.complex64)
    path = tmp_path / "x.txt"
    np.savetxt(path, np.stack([x.real, x.imag], axis=1), fmt="%.9g")
    out = subprocess.run([emu, str(path)], capture_output=True, text=True, check=True)
    y = np.loadtxt(out.stdout.splitlines())
    return x, y[:, 0] + 1j * y[:, 1]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_pfa513_matches_numpy(emu, tmp_path, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(513) + 1j * rng.standard_normal(513)
    x, got = _run(emu, tmp_path, x)
    want = np.fft.fft(x.astype(np.complex128))
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    assert err < 1e-6, err


def test_pfa513_each_bin(emu, tmp_path):
    # a tone on every bin at once is the all-bins check of the output map: a pure tone at bin m
    # must come out at bin m and nowhere else
    n = np.arange(513)
    for m in (0, 1, 19, 27, 256, 257, 512):
        x = np.exp(2j * np.pi * m * n / 513)
        x, got = _run(emu, tmp_path, x)
        assert np.argmax(np.abs(got)) == m
        want = np.fft.fft(x.astype(np.complex128))
        assert np.max(np.abs(got - want)) / 513 < 1e-6


def test_pfa513_dc_offset(emu, tmp_path):
    # a large common value on a small signal: the DC removal keeps the small bins accurate
    rng = np.random.default_rng(7)
    x = 1e3 * (1 + 1j) + 1e-2 * (rng.standard_normal(513) + 1j * rng.standard_normal(513))
    x, got = _run(emu, tmp_path, x)
    want = np.fft.fft(x.astype(np.complex128))
    assert abs(got[0] - want[0]) / abs(want[0]) < 1e-6
    assert np.max(np.abs(got[1:] - want[1:])) < 1e-6 * np.max(np.abs(want[1:])) * 10
