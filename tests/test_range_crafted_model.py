"""CPU: the crafted range-kernel inputs of tests/range_crafted.py, checked without a device.

For every geometry of the table: the restated planner gives the table's segmentation; the fp64 oracle's FFT form and its
time-domain form agree on the census to 1e-12 of the peak; every planted product is at least 1e-3 of the map's peak (so a
lost, extra or misplaced pair misses the GPU tests' 1e-5 gate by 100 times); all samples fit int8.  Then the sensitivity
proof: three deliberately wrong restatements of the correlation each miss the 1e-5 gate on the census by more than 1000
times -- what the GPU tests would report for such a kernel, shown without making a kernel fail on a device."""
import os
import re

import numpy as np
import pytest

import range_crafted as RC
from conftest import ROOT
from oracle import blah2_oracle as O

PEAK_TOL = 1e-5  # tests/test_timed_kernels_gpu.py
ALL = RC.GEOMS + (RC.CHUNKED,)
_cache = {}


def case(g, seed=1):
    if (g.name, seed) not in _cache:
        d = RC.dims_of(g)
        x, y = RC.census(d, g.n_seg, g.seg_len, seed, extra_cols=RC.extra_cols_of(g))
        _cache[(g.name, seed)] = (d, x, y, RC.reference(d, x, y))
    return _cache[(g.name, seed)]


def test_the_chunk_cap_is_the_engines():
    src = open(os.path.join(ROOT, "blah2_amd", "csrc", "capi.hip")).read()
    m = re.search(r"lag_chunks\(h, 4081\);\s*if \(h->chunks.size\(\) > 1 \|\| h->maxChunk > 4081\) lag_chunks\(h, (\d+)\);", src)
    assert m and int(m.group(1)) == RC.LAG_CHUNK_CAP
    assert RC.chunk_seams(4431) == [2048, 4096] and RC.chunk_seams(4081) == []


@pytest.mark.parametrize("g", ALL, ids=[g.name for g in ALL])
def test_plan_and_dims(g):
    d = RC.dims_of(g)
    assert (d.n_doppler_bins, d.n_corr, d.n_samples) == (5, g.n_corr, 5 * g.n_corr + 4)
    assert d.n_delay_bins == g.delay_max - g.delay_min + 1
    assert RC.plan_of(g) == (g.n_seg, g.seg_len)
    assert g.n_seg * g.seg_len >= g.n_corr > (g.n_seg - 1) * g.seg_len
    assert g.seg_len + min(d.n_delay_bins, RC.LAG_CHUNK_CAP if d.n_delay_bins > 4081 else d.n_delay_bins) - 1 <= g.fft_len


def test_the_table_pins_what_it_says():
    """Window lengths and the variant thresholds of the launch code, from the table's own numbers."""
    w = {g.name: g.seg_len + (g.delay_max - g.delay_min + 1) - 1 for g in RC.GEOMS}
    nd = {g.name: g.delay_max - g.delay_min + 1 for g in RC.GEOMS}
    full = [n for n, g in RC.GEOM_BY_NAME.items() if g is not RC.CHUNKED and w[n] == g.fft_len]
    assert len(full) >= 8
    assert w["1k-448x1728"] == 1023 and w["2k-257x3072"] == 1792 and w["2k-258x3072"] == 1793
    # REUSE: segLen == 576 and nDelay <= 449; OUT7: nDelay <= 448; SHORTX: segLen <= 576
    assert (nd["1k-449x1728"], nd["1k-448x1728"], nd["1k-450x1725"]) == (449, 448, 450)
    assert RC.GEOM_BY_NAME["1k-448x1154"].seg_len == 577 and RC.GEOM_BY_NAME["1k-450x1725"].seg_len == 575
    assert RC.GEOM_BY_NAME["1k-449x1729"].n_corr - 3 * 576 == 1
    # shortw: segLen <= 1536, window <= 1792, nDelay <= 448; half-zero x of range_kernel<16>: segLen <= 2048
    assert RC.GEOM_BY_NAME["4k-2049x4096"].seg_len == 2048 and RC.GEOM_BY_NAME["4k-2050x4094"].seg_len == 2047


@pytest.mark.parametrize("g", ALL, ids=[g.name for g in ALL])
def test_census_values_and_amplitude_condition(g):
    d, x, y, ref = case(g)
    for v in (x, y):
        assert v.shape == (d.n_samples,) and np.array_equal(v.real, np.rint(v.real)) and np.array_equal(v.imag, np.rint(v.imag))
        assert max(np.abs(v.real).max(), np.abs(v.imag).max()) <= 7  # fits int8 (and int16, fp16, fp32) exactly
        nz = np.abs(v[np.abs(v) > 0])
        assert nz.min() >= 3
        assert np.all(np.abs(v[-RC.TAIL:]) > 0)
    used = d.n_doppler_bins * d.n_corr
    # sparse: a few hundred impulses at the most; pulses 0 and 1 both populated, pulse 3 empty
    assert 0 < np.count_nonzero(x[:used]) <= 4 * (4 + 3 * (g.n_seg - 1))
    assert np.count_nonzero(x[3 * d.n_corr:4 * d.n_corr]) == 0 and np.count_nonzero(x[d.n_corr:2 * d.n_corr]) > 0
    peak = np.abs(ref).max()
    ratio = RC.smallest_product(d, x, y) / peak
    print(f"\n[{g.name}] smallest planted product / peak = {ratio:.3e}, peak {peak:.1f}")
    assert ratio >= 1e-3


@pytest.mark.parametrize("g", ALL, ids=[g.name for g in ALL])
def test_fft_form_and_time_domain_form_agree(g):
    """O.ambiguity_process against the definition: O.ambiguity_process_direct, and its sparse restatement that the
    sensitivity proof mutates (range_crafted.correlate: the same sums over the populated samples only)."""
    d, x, y, ref = case(g)
    peak = np.abs(ref).max()
    sparse = RC.correlate(d, x, y, g.n_seg, g.seg_len)
    assert np.abs(sparse - ref).max() <= 1e-12 * peak
    direct = O.ambiguity_process_direct(d, x, y)
    assert np.abs(direct - ref).max() <= 1e-12 * peak
    assert np.abs(direct - sparse).max() <= 1e-12 * peak


@pytest.mark.parametrize("mutant", ["leak", "first", "segend"])
@pytest.mark.parametrize("g", ALL, ids=[g.name for g in ALL])
def test_wrong_kernels_would_fail_the_gate_by_1000_times(g, mutant):
    """y read across pulse boundaries / the pulse's first y sample read as zero / the last x sample of each segment
    dropped: each moves the census map by more than 1000 x 1e-5 of its peak."""
    d, x, y, ref = case(g)
    bad = RC.correlate(d, x, y, g.n_seg, g.seg_len, mutant)
    moved = np.abs(bad - ref).max() / np.abs(ref).max()
    print(f"\n[{g.name}] {mutant}: {moved:.3e} of the peak")
    if mutant == "first" and g.delay_min > 0:
        # a window of positive lags only never multiplies the pulse's first y sample (y[a + lag], a >= 0, lag >= 1): the
        # definition itself does not read it, so there is nothing for this mutant to get wrong
        assert moved <= 1e-12
        return
    assert moved > 1000 * PEAK_TOL


def test_one_pulse_census_has_constant_modulus_columns():
    """The Doppler-row census (one populated pulse): every column of the map has the same modulus in all nD rows."""
    args = (-3, 36, -32, 32, 65 * 40 + 4, 65 * 40 + 4)
    d = O.ambiguity_dims(*args, True)
    assert (d.n_doppler_bins, d.n_corr, d.n_delay_bins) == (65, 40, 40)
    for i0 in (0, 1, 63, 64, 32):
        x, y = RC.census(d, 1, 40, 7 + i0, pulses=[i0])
        ref = RC.reference(d, x, y)
        mod = np.abs(ref)
        assert mod.max() > 0 and np.abs(mod - mod[0:1]).max() <= 1e-12 * mod.max()
        assert RC.smallest_product(d, x, y) >= 1e-3 * mod.max()
