"""CPU: the crafted taps and pulses of tests/fir_crafted.py for the fused FIR range kernel, checked without a device.

The table's dims, block counts and the launcher's acceptance conditions; the helper's filter against the oracle's own
(oracle.blah2_oracle.wiener_hopf with its solved taps); the sparse time-domain restatement against the fp64 reference on
every case the GPU tests run; the amplitude condition (every planted product at least 1e-3 of the map's peak); and the
sensitivity proof: seven deliberately wrong restatements of the kernel's edge handling each move the census map by more than
1000 x 1e-5 of its peak on every row where the term exists, and by nothing where it does not.  Last, the NumPy model of the
kernel's transform sequence (tools/proto/fir_range_fusion_model.py) against the same reference."""
import os
import re
import sys

import numpy as np
import pytest

import fir_crafted as FC
from conftest import ROOT
from oracle import blah2_oracle as O

PEAK_TOL = 1e-5  # tests/test_timed_kernels_gpu.py
IDS = [g.name for g in FC.GEOMS]
TABLE = {  # name: (delayMin, delayMax, fMax, nCorr, spare, SB)
    "min-pulse": (-8, 300, 10, 2056, 8, 2), "on-boundary": (-8, 300, 10, 4096, 8, 3), "past-5": (-8, 300, 10, 4101, 8, 3),
    "short-5": (-8, 300, 10, 4091, 8, 3), "block-fits-4104": (-8, 300, 10, 4104, 8, 3), "block-fits-4088": (-8, 300, 10, 4088, 8, 2),
    "long-walk": (-8, 300, 10, 9523, 8, 5), "dmin0": (0, 2048, 5, 10000, 3, 5), "dmin1": (-1, 40, 2, 2049, 1, 2),
    "head-block1": (-24, 2023, 15, 6149, 30, 4), "wide-dmin": (-260, 100, 131, 2400, 260, 2),
}


@pytest.mark.parametrize("g", FC.GEOMS, ids=IDS)
def test_dims_blocks_and_acceptance(g):
    assert tuple(g[1:7]) == TABLE[g.name]
    d = FC.dims_of(g)
    nD = 2 * g.f_max + 1
    assert (d.n_doppler_bins, d.n_corr, d.n_samples) == (nD, g.n_corr, nD * g.n_corr + g.spare)
    assert d.n_delay_bins == g.delay_max - g.delay_min + 1 and d.doppler_middle == 0
    assert -g.delay_min <= g.spare < nD
    assert g.sb == -(-(g.n_corr - g.delay_min) // FC.L)
    # one run of linear lags in the oracle's transform, so that lag of column c = delayMin + c
    assert d.nfft - d.n_corr >= max(abs(d.delay_min), abs(d.delay_max))
    assert FC.unfusable(d, FC.default_bins(g), g.delay_min) is None


def test_the_table_pins_what_it_says():
    G = FC.GEOM_BY_NAME
    assert G["min-pulse"].n_corr == FC.L - G["min-pulse"].delay_min and G["min-pulse"].spare == -G["min-pulse"].delay_min
    assert G["on-boundary"].n_corr == 2 * FC.L
    assert G["past-5"].n_corr == 2 * FC.L + 5 and G["short-5"].n_corr == 2 * FC.L - 5
    assert G["block-fits-4088"].n_corr - G["block-fits-4088"].delay_min == 2 * FC.L
    assert G["block-fits-4104"].n_corr - G["block-fits-4104"].delay_min == 2 * FC.L + 16
    assert FC.default_bins(G["dmin0"]) == 2048 and FC.dims_of(G["dmin0"]).n_delay_bins == 2049
    hb = G["head-block1"]  # `head` in block 1: nBins - 1 >= 2049 + delayMin
    assert FC.default_bins(hb) - 1 >= FC.L + 1 + hb.delay_min and hb.spare > -hb.delay_min
    assert -G["wide-dmin"].delay_min > 256 and -G["dmin1"].delay_min == 1


def test_the_acceptance_conditions_are_the_launchers():
    """FC.unfusable restates capi.hip's fir_unfusable(): the source still reads as it did when this was written, and the
    restatement refuses each boundary one past the accepted side."""
    src = open(os.path.join(ROOT, "blah2_amd", "csrc", "capi.hip")).read()
    body = src[src.index("const char *fir_unfusable("):]
    body = body[:body.index("\n}\n")]
    for cond in ("const int L = 2048;", "nBins < 1 || nBins > L + 1 || nDelay > L + 1", "firDmin != h->delayMin || h->delayMin > 0",
                 "nBins < -firDmin", "(int)h->dims.n_corr < L - h->delayMin",
                 "(uint64_t)h->dims.n_used + (uint64_t)(-h->delayMin) > h->dims.n_samples"):
        assert cond in body, cond
    assert len(re.findall(r"\breturn \"", body)) == 9  # no condition this file does not know of
    G = FC.GEOM_BY_NAME
    mp, d1, d0, p5 = G["min-pulse"], G["dmin1"], G["dmin0"], G["past-5"]
    for g, nb, want in ((mp._replace(n_corr=2055), 308, "shorter"), (mp._replace(spare=7), 308, "look-ahead"),
                        (d1._replace(spare=0), 41, "look-ahead"), (d0, 2050, "2049"), (p5, 7, "lag 0"),
                        (d0._replace(delay_max=2049), 2049, "2049")):
        d = FC.dims_of(g)
        assert d.n_corr == g.n_corr and d.n_samples - d.n_doppler_bins * d.n_corr == g.spare
        assert want in FC.unfusable(d, nb, g.delay_min), (g, nb)
    for g, nb in ((mp, 308), (d1, 41), (d0, 2049), (p5, 8)):
        assert FC.unfusable(FC.dims_of(g), nb, g.delay_min) is None


def test_the_helpers_filter_is_the_oracles():
    """FC.filtered with the oracle's own solved taps reproduces the oracle's filtered channel: the helper is tied to the
    restatement that the golden fixtures tie to the compiled reference."""
    for dmin, dmax, n, seed in ((-5, 40, 3000, 1), (0, 33, 2500, 2), (-1, 20, 2001, 3)):
        x, y = O.synth_iq(n, seed=seed, fs=n, targets=((7, 3.0, 0.1),))
        ok, yf, w, _, _ = O.wiener_hopf(x, y, dmin, dmax, return_filter=True)
        assert ok and w.shape == (dmax - dmin,) and np.count_nonzero(w) == w.size
        mine = FC.filtered(x, y, w, dmin)
        err = np.abs(mine - yf).max() / np.abs(y).max()
        print(f"\n[filter, delayMin {dmin}, {w.size} solved taps] {err:.2e} of max|y|")
        assert err <= 1e-12


def test_tap_sets_are_what_they_say():
    g = FC.GEOM_BY_NAME["past-5"]
    A, nb = 8, 308
    for cls in FC.TAP_SETS:
        w = FC.taps(g, cls, 3)
        assert w.shape == (3, nb) and np.array_equal(w * 8, np.rint(w.real * 8) + 1j * np.rint(w.imag * 8))
        assert np.array_equal(w.astype(np.complex64).astype(np.complex128), w)
        nz = np.abs(w[w != 0])
        if cls == "g":
            assert nz.size == 0
            continue
        assert nz.min() >= 0.375 and nz.max() <= 1.01 and np.count_nonzero(w) <= 3 * 16
        assert not np.array_equal(w[0], w[1]) and not np.array_equal(w[1], w[2])
        k0 = [FC.k0_of(w[c]) for c in range(3)]
        if cls in "af":
            assert k0 == [A] * 3
        if cls == "a":
            assert all(np.all(w[c, :A] != 0) and w[c, nb - 1] != 0 for c in range(3))
        if cls == "b":
            assert k0 == [0] * 3
        if cls == "c":
            assert k0 == [7, 1, 4]
        if cls == "d":
            assert k0 == [nb - 1] * 3
        if cls == "e":
            assert k0 == [255, 256, 255]
        if cls == "f":
            top = np.sort(np.abs(w[0]) ** 2)[-2:]
            assert top[0] == top[1] and abs(w[0, nb - 1]) ** 2 == top[1]
        if cls == "h":
            assert [np.count_nonzero(w[c]) for c in range(3)] == [1, 1, 1] and k0 == [0, A, nb - 1]
    assert [FC.k0_of(r) for r in FC.taps(FC.GEOM_BY_NAME["dmin0"], "e", 3)] == [255, 256, 2047]
    assert FC.k0_of(FC.taps(FC.GEOM_BY_NAME["dmin0"], "d", 1, 2049)[0]) == 2048
    assert [FC.k0_of(r) for r in FC.taps(g, "mixed", 4)] == [A, 1, nb - 1, 256]  # four classes of the largest tap in one batch
    wide = FC.taps(FC.GEOM_BY_NAME["wide-dmin"], "a", 1)[0]
    assert wide[255] != 0 and wide[256] != 0 and wide[259] != 0 and FC.k0_of(wide) == 260
    m = FC.multipath_taps(g, 2)
    for r in m:
        nz = np.abs(r[r != 0])
        assert 10 <= nz.size <= 12 and nz.min() >= 0.1 and nz.max() <= 0.6 and np.any(r[:A] != 0)
        assert np.array_equal(r.astype(np.complex64).astype(np.complex128), r)


@pytest.mark.parametrize("case", FC.CASES, ids=[FC.case_id(c) for c in FC.CASES])
def test_sparse_restatement_and_amplitude_condition(case):
    """filter_sparse == reference to 1e-12 of the peak on every case the GPU tests run, and every planted product is at least
    1e-3 of the map's peak there: one lost, extra or misplaced product misses the GPU tests' 1e-5 gate by 100 times."""
    name, cls, nb = case
    g = FC.GEOM_BY_NAME[name]
    b = FC.batch(g, cls, nb, B=4 if cls == "mixed" else 3)
    d = b["d"]
    used = d.n_doppler_bins * d.n_corr
    for c, (x, y, ref) in enumerate(zip(b["xs"], b["ys"], b["refs"])):
        for v in (x, y):
            assert np.array_equal(v.real, np.rint(v.real)) and np.array_equal(v.imag, np.rint(v.imag))
            nz = np.abs(v[v != 0])
            assert max(np.abs(v.real).max(), np.abs(v.imag).max()) <= 7 and nz.min() >= 5 - 1e-9
        assert (not y[:used].any()) == (c == FC.Y_ZERO_CPI)
        assert np.count_nonzero(x) <= 160
        peak = np.abs(ref).max()
        if not b["w"][c].any() and c == FC.Y_ZERO_CPI:
            assert peak == 0  # no taps, no surveillance channel: the map is zero
            continue
        sparse = FC.filter_sparse(d, x, y, b["w"][c], g.delay_min)
        agree = np.abs(sparse - ref).max() / peak
        ratio = FC.smallest_product(d, x, y, b["w"][c]) / peak
        print(f"\n[{FC.case_id(case)} cpi {c}] k0 {FC.k0_of(b['w'][c])}, {np.count_nonzero(b['w'][c])} taps, {np.count_nonzero(x)} x impulses: "
              f"peak {peak:.0f}, sparse - reference {agree:.1e}, smallest planted product / peak {ratio:.3e}")
        assert agree <= 1e-12
        assert ratio >= 1e-3


def test_census_population():
    """Pulses 0, 1, the middle one and the last carry the census; between them there are pulses without a single sample; the
    spare region's first |delayMin| samples are populated, and on head-block1 spare samples beyond them too."""
    for g in FC.GEOMS:
        d = FC.dims_of(g)
        nD, nC, A = d.n_doppler_bins, d.n_corr, -g.delay_min
        x, y = FC.census(g, FC.SEED0)
        assert [i for i in range(nD) if y[i * nC:(i + 1) * nC].any()] == FC.populated_pulses(nD)
        if nD > 5:
            assert any(not x[i * nC:(i + 1) * nC].any() and not y[i * nC:(i + 1) * nC].any() for i in range(nD))
        assert np.count_nonzero(x[nD * nC:nD * nC + A]) == len(FC.edge_offsets(A))
        assert np.count_nonzero(x[nD * nC + A:]) == (2 if g.spare > A else 0)
        assert np.count_nonzero(x[:A]) == len(FC.edge_offsets(A))


EMPTY = {"dmin0": ("notail", "nohead", "k0masked", "leak", "stride")}  # no anticipation: no look-ahead, no zero start


@pytest.mark.parametrize("mutant", FC.MUTANTS)
@pytest.mark.parametrize("g", FC.GEOMS, ids=IDS)
def test_wrong_kernels_would_fail_the_gate_by_1000_times(g, mutant):
    """Each wrong restatement moves every CPI's census map (tap set a) by more than 1000 x 1e-5 of its peak -- what the GPU
    tests would report for such a kernel -- or by nothing on the row where the term it gets wrong does not exist."""
    b = FC.batch(g, "a")
    d, B = b["d"], len(b["xs"])
    for c in range(B):
        if mutant == "taps0" and c == 0:
            continue  # CPI 0 with CPI 0's taps is right
        ref = b["refs"][c]
        bad = FC.filter_sparse(d, b["xs"][c], b["ys"][c], b["w"][c], g.delay_min, mutant, w_other=b["w"][0], x_next=b["xs"][(c + 1) % B])
        moved = np.abs(bad - ref).max() / np.abs(ref).max()
        print(f"\n[{g.name} cpi {c}] {mutant}: {moved:.3e} of the peak")
        if mutant in EMPTY.get(g.name, ()):
            assert moved <= 1e-12
        else:
            assert moved > 1000 * PEAK_TOL


@pytest.mark.parametrize("mutant", ["notail", "k0masked"])
def test_the_skipped_tap_of_the_tail_loop_is_covered(mutant):
    """Tap set c puts the largest tap at an anticipatory index: the kernel's `tail` loop must then skip it (it already runs
    on the true stream).  Both ways of getting that wrong show: the tap lost past the pulse's end (k0masked), and the whole
    look-ahead lost (notail)."""
    g = FC.GEOM_BY_NAME["past-5"]
    b = FC.batch(g, "c")
    for c in range(3):
        assert FC.k0_of(b["w"][c]) < -g.delay_min
        bad = FC.filter_sparse(b["d"], b["xs"][c], b["ys"][c], b["w"][c], g.delay_min, mutant)
        moved = np.abs(bad - b["refs"][c]).max() / np.abs(b["refs"][c]).max()
        print(f"\n[past-5 set c cpi {c}] {mutant}: {moved:.3e} of the peak")
        assert moved > 1000 * PEAK_TOL


def test_the_transform_model_reproduces_the_reference():
    """tools/proto/fir_range_fusion_model.fused_window_form -- the kernel's sequence transform for transform -- gives the range
    stage of FC.reference on two rows scaled down to 64-point transforms (as tests/test_fusion_model.py scales): past-5
    (delayMin -3, a pulse 5 past two blocks) and dmin0 (no anticipation, L taps, L + 1 lags)."""
    sys.path.insert(0, os.path.join(ROOT, "tools", "proto"))
    import fir_range_fusion_model as M
    F, Ls = 64, 32
    rng = np.random.default_rng(17)
    for dmin, dmax, f_max, n_corr, spare, n_taps in ((-3, 29, 2, 2 * Ls + 5, 4, 32), (0, 32, 1, 100, 2, 32)):
        nD = 2 * f_max + 1
        n = nD * n_corr + spare
        d = O.ambiguity_dims(dmin, dmax, -f_max, f_max, n, n, True)
        assert (d.n_doppler_bins, d.n_corr, d.n_delay_bins) == (nD, n_corr, Ls + 1)
        x = rng.integers(-7, 8, n) + 1j * rng.integers(-7, 8, n)
        y = rng.integers(-7, 8, n) + 1j * rng.integers(-7, 8, n)
        w = (rng.integers(-5, 6, n_taps) + 1j * rng.integers(-5, 6, n_taps)) / 8.0
        ref = FC.reference(d, x, y, w, dmin)
        D = np.empty_like(ref)
        D[(np.arange(nD) + nD // 2 + 1) % nD] = ref  # undo the Doppler stage (Ambiguity.cpp:152-169)
        R = np.fft.ifft(D, axis=0)
        Rf, _ = M.fused_window_form(x.astype(np.complex128), y.astype(np.complex128), w, dmin, n_corr, nD, np.arange(dmin, dmax + 1), F)
        err = np.abs(Rf - R).max() / np.abs(R).max()
        print(f"\n[transform model, delayMin {dmin}, nCorr {n_corr}] {err:.2e} of the range stage's peak")
        assert err <= 1e-12
