"""CPU: a NumPy model of the candidate test of hot_columns_kernel (csrc/capi.hip, "hot columns"), with the kernel's own constants.

A column is transformed again in fp64 when its amplitude estimate from the range map, times nD / HOT_BOUND, reaches HOT_RATIO x
the map's mean level.  The estimate is the larger of two sample standard deviations of the column: over the S pulses
0 .. S-1 and over the S pulses floor((2s+1) nD / (2S)), S = HOT_SET_SMALL up to nD = HOT_SET_SMALL_ND, else HOT_SET_LARGE.
The kernel's threshold assumes that the estimate reads at least HOT_BOUND of a tone's amplitude at every Doppler; these tests sweep a tone over every Doppler on a
1/16-bin grid and check that, and that white-noise columns stay clear of the lowered threshold.  The constants are read from
the kernel source, so a change of the kernel that the model does not follow fails here.
"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPI = os.path.join(ROOT, "blah2_amd", "csrc", "capi.hip")
ND_SWEEP = (101, 257, 513, 1025, 1537, 2049, 4096)
NOISE_MARGIN_DB = 2.0  # white-noise columns stay this far under the test at every nD, in the map's dB (10 log10 |z|):
                       # the typical column sits a factor 0.75 HOT_BOUND HOT_RATIO / sqrt(nD) under it (2.3 = 3.7 dB at nD = 4096)


def kernel_constants():
    """HOT_* from the constexpr lines of capi.hip."""
    src = open(CAPI).read()
    out = {}
    for line in re.findall(r"^constexpr\s+(?:int|double)\s+(HOT_[^;]*);", src, flags=re.M):
        for name, val in re.findall(r"(HOT_\w+)\s*=\s*([0-9.eE+-]+)", line):
            out[name] = float(val) if "." in val or "e" in val.lower() else int(val)
    return out, src


C, SRC = kernel_constants()


def set_size(nD):
    return C["HOT_SET_SMALL"] if nD <= C["HOT_SET_SMALL_ND"] else C["HOT_SET_LARGE"]


def spaced_pulses(nD):
    S = set_size(nD)
    return ((2 * np.arange(S) + 1) * nD) // (2 * S)


def block_pulses(nD):
    return np.arange(min(set_size(nD), nD))


def estimate(cols, nD):
    """The kernel's amplitude estimate of each column of cols [nD, ncol] (complex): max of the two sample standard deviations."""
    def sd(idx):
        r = cols[idx]
        return np.sqrt(np.maximum(np.mean(np.abs(r) ** 2, axis=0) - np.abs(np.mean(r, axis=0)) ** 2, 0.0))
    return np.maximum(sd(block_pulses(nD)), sd(spaced_pulses(nD)))


def tone_ratio(nD, k):
    """Estimate / amplitude of the unit tone e^{2 pi i k p / nD} for each k (bins off zero Doppler).  For |k| < 1 the tone is
    partly zero-Doppler content; there the reference is its largest off-zero-Doppler cell / nD, what the map shows of it."""
    k = np.asarray(k, dtype=np.float64)
    pulses = np.arange(nD)
    # the estimate only reads these pulses: the tone is built there alone (the sweep at nD = 4096 has 65 536 tones)
    rows = np.union1d(block_pulses(nD), spaced_pulses(nD))
    cols = np.zeros((nD, k.size), dtype=np.complex128)
    cols[rows] = np.exp(2j * np.pi * np.outer(rows, k) / nD)
    out = estimate(cols, nD)
    near = np.abs(k) < 1.0
    if near.any():
        full = np.exp(2j * np.pi * np.outer(pulses, k[near]) / nD)
        out[near] /= np.abs(np.fft.fft(full, axis=0))[1:].max(axis=0) / nD
    return out


def sweep(nD):
    """k over [-nD/2, nD/2] on a 1/16-bin grid, zero Doppler itself left out (a constant column is no candidate)."""
    k = np.arange(-8 * nD, 8 * nD + 1) / 16.0
    k = k[k != 0.0]
    return k, tone_ratio(nD, k)


def worst_k(nD):
    """The Doppler (bins) where the estimate reads least of a tone, and that ratio."""
    k, r = sweep(nD)
    i = int(np.argmin(r))
    return float(k[i]), float(r[i])


def test_constants_are_read_from_the_kernel():
    for name in ("HOT_SET_SMALL", "HOT_SET_LARGE", "HOT_SET_SMALL_ND", "HOT_BOUND", "HOT_RATIO", "HOT_MAX", "HOT_CAND", "HOT_ND_MAX"):
        assert name in C, (name, C)
    assert 0.0 < C["HOT_BOUND"] <= 1.0
    # the sample positions the model restates, as the kernel writes them
    assert "(int64_t)(2 * i + 1) * nD) / (2 * S)" in SRC
    assert "i < nD ? i : 0" in SRC and "min(S, nD)" in SRC
    assert "nD <= HOT_SET_SMALL_ND ? hot_estimate<HOT_SET_SMALL>(Rj, nD) : hot_estimate<HOT_SET_LARGE>(Rj, nD)" in SRC
    assert "10.0 * std::log10(HOT_RATIO * HOT_BOUND)" in SRC


@pytest.mark.parametrize("nD", ND_SWEEP)
def test_the_estimate_reads_a_tone_at_every_doppler(nD):
    assert nD <= C["HOT_ND_MAX"]
    k, r = sweep(nD)
    i = int(np.argmin(r))
    print(f"\n[hot model] nD {nD}: worst estimate / amplitude {r[i]:.3f} at k = {k[i]:+.4f} bins; "
          f"at k = 8, 16, 64: {tone_ratio(nD, [8.0, 16.0, 64.0]).round(3)}")
    assert r[i] >= C["HOT_BOUND"], (nD, float(k[i]), float(r[i]))
    # nor does it read more than the tone: the ordering of candidates is by strength within [HOT_BOUND, 1]
    assert r[np.abs(k) >= 1.0].max() <= 1.0 + 1e-9


@pytest.mark.parametrize("nD", ND_SWEEP)
def test_noise_columns_stay_under_the_test(nD):
    """White complex noise, sigma per pulse: the map's mean level (Map::set_metrics: mean of 10 log10 |cell|) is ~0.75 sigma
    sqrt(nD), the estimate ~sigma; the kernel's test is estimate x nD / HOT_BOUND >= HOT_RATIO x level."""
    rng = np.random.default_rng(20 + nD)
    ncol = max(256, 2 ** 21 // nD)
    cols = rng.standard_normal((nD, ncol)) + 1j * rng.standard_normal((nD, ncol))
    level_db = float(np.mean(10.0 * np.log10(np.abs(np.fft.fft(cols, axis=0)))))
    thr_db = level_db + 10.0 * np.log10(C["HOT_RATIO"] * C["HOT_BOUND"]) - 10.0 * np.log10(nD)
    est_db = 10.0 * np.log10(estimate(cols, nD))
    margin = thr_db - float(est_db.max())
    print(f"\n[hot model] nD {nD}: {ncol} noise columns, the largest estimate {margin:.2f} dB (10 log10 |z|) under the test")
    assert margin >= NOISE_MARGIN_DB, (nD, margin)
