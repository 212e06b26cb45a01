"""CPU: randomized self-consistency of the oracle (hypothesis) -- the checker must be
right before it checks anything.  Fast forms against their definitional forms, and
the derived sizes against the invariants the reference's constructor guarantees."""
import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

import cfar_crafted as X
from oracle import blah2_oracle as O
from oracle import ref_lib as R

FAST = settings(max_examples=60, deadline=None)


def is_hamming(v):
    for p in (2, 3, 5):
        while v % p == 0:
            v //= p
    return v == 1


@FAST
@given(st.integers(min_value=0, max_value=200_000))
def test_next_hamming_is_the_smallest_5_smooth_number_above(v):
    # HammingNumber.cpp:38-48: strictly greater, 2^a 3^b 5^c, none in between
    h = O.next_hamming(v)
    assert h > v and is_hamming(h)
    assert not any(is_hamming(k) for k in range(v + 1, h))
    if R.available():
        assert R.next_hamming(v) == h


@FAST
@given(st.integers(-64, 1), st.integers(0, 200), st.integers(1, 300), st.integers(5_000, 400_000), st.booleans())
def test_ambiguity_dims_invariants(delay_min, span, doppler_max, n, round_hamming):
    # Ambiguity.cpp:11-82 for symmetric Doppler limits (every shipped configuration)
    fs = 200_000
    delay_max = max(delay_min + span, -1)
    n_doppler = 2 * (doppler_max * n // fs) + 1
    # nCorr is a uint16_t in the reference (Ambiguity.h:110): n / nDopplerBins wraps mod 65536,
    # and a wrapped value of 0 divides by zero at :43 -- outside any usable configuration
    if (n // n_doppler) & 0xFFFF == 0:
        return
    d = O.ambiguity_dims(delay_min, delay_max, -doppler_max, doppler_max, fs, n, round_hamming)
    assert d.n_delay_bins == delay_max - delay_min + 1
    assert d.n_doppler_bins % 2 == 1
    assert d.n_doppler_bins == n_doppler
    assert d.n_corr == (n // d.n_doppler_bins) & 0xFFFF and d.n_corr * d.n_doppler_bins <= n
    assert d.nfft == (O.next_hamming(2 * d.n_corr - 1) if round_hamming else 2 * d.n_corr - 1)
    assert d.delay[0] == delay_min and d.delay[-1] == delay_max
    assert abs(d.doppler[d.n_doppler_bins // 2]) < 1e-9  # centre bin is 0 Hz
    assert np.allclose(np.diff(d.doppler), 1.0 / d.cpi)


@settings(max_examples=25, deadline=None)
@given(st.integers(0, 2**32 - 1), st.integers(-6, 1), st.integers(2, 24), st.integers(1, 6))
def test_fft_form_equals_the_defining_sums(seed, delay_min, span, doppler_max):
    # the restatement used as the oracle (three FFTs per pulse) against the literal
    # double sum of Ambiguity.cpp:106-169 on small random problems
    rng = np.random.default_rng(seed)
    fs, n = 1000, int(rng.integers(300, 700))
    delay_max = max(delay_min + span, -1)
    d = O.ambiguity_dims(delay_min, delay_max, -doppler_max, doppler_max, fs, n, bool(seed & 1))
    if d.n_corr < 8 or d.n_delay_bins >= d.n_corr:
        return
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    y = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    a, b = O.ambiguity_process(d, x, y), O.ambiguity_process_direct(d, x, y)
    assert np.max(np.abs(a - b)) <= 1e-10 * np.max(np.abs(b))


@settings(max_examples=40, deadline=None)
@given(st.integers(0, 2**32 - 1), st.integers(0, 3), st.integers(1, 7), st.integers(0, 4))
def test_cfar_fast_forms_equal_their_definitions(seed, n_guard, n_train, min_delay):
    rng = np.random.default_rng(seed)
    nD, nC = int(rng.integers(3, 24)) | 1, int(rng.integers(4, 60))
    m = (rng.standard_normal((nD, nC)) + 1j * rng.standard_normal((nD, nC))) * rng.choice([1.0, 30.0], size=(nD, nC), p=[0.95, 0.05])
    delay = np.arange(-2, nC - 2)
    doppler = (np.arange(nD) - nD // 2) * 2.5
    noise, _ = O.map_metrics(m)
    pfa = float(rng.choice([1e-1, 1e-2, 1e-4]))
    a = O.cfar1d(m, delay, doppler, noise, pfa, n_guard, n_train, min_delay, 3.0)
    b = O.cfar1d_fast(m, delay, doppler, noise, pfa, n_guard, n_train, min_delay, 3.0)
    assert all(np.array_equal(u, v) for u, v in zip(a[:2], b[:2])) and np.allclose(a[2], b[2], rtol=0, atol=1e-12)
    ng_f, nt_f = int(rng.integers(0, 3)), int(rng.integers(0, 4))
    c = O.cfar2d_bruteforce(m, delay, doppler, noise, pfa, n_guard, n_train, ng_f, nt_f, min_delay, 3.0)
    e = O.cfar2d(m, delay, doppler, noise, pfa, n_guard, n_train, ng_f, nt_f, min_delay, 3.0)
    assert all(np.array_equal(u, v) for u, v in zip(c[:2], e[:2]))
    if ng_f == 0 and nt_f == 0:  # the 2-D extension collapses to CfarDetector1D.cpp:23-100
        assert all(np.array_equal(u, v) for u, v in zip(a[:2], e[:2]))


ADDITIVE_MAPS = {
    # name: (nD, nC, Doppler axis, map flavour)
    "small": (9, 21, np.arange(-4.0, 5.0), "floor"),
    "one-column": (7, 1, np.arange(-3.0, 4.0), "floor"),
    "fewer-rows-than-the-halo": (3, 30, np.arange(-1.0, 2.0), "floor"),
    "one-sided-axis": (12, 17, 11.5 + np.arange(-6.0, 6.0), "floor"),
    "dynamic-range": (10, 24, np.arange(-5.0, 5.0), "range"),
}


@pytest.mark.parametrize("window", X.WINDOWS, ids=lambda w: "w" + "_".join(map(str, w)))
@pytest.mark.parametrize("name", sorted(ADDITIVE_MAPS))
def test_cfar2d_additive_equals_the_bruteforce_definition(name, window):
    """The vectorised additive form (what the crafted detector tests compare against) returns the hit list of the
    four-loop definition: every stream-kernel window, two tile-only windows and a summed-area-only one, on a map of
    one column, one with fewer rows than the halo, a one-sided Doppler axis and cells from 1e-20 to 1e18."""
    nD, nC, doppler, kind = ADDITIVE_MAPS[name]
    rng = np.random.default_rng([nD, nC, *window])
    m = np.sqrt(rng.exponential(1.0, (nD, nC))) * np.exp(2j * np.pi * rng.uniform(0, 1, (nD, nC)))
    m[rng.integers(0, nD, 6), rng.integers(0, nC, 6)] *= 40.0
    if kind == "range":
        m *= 10.0 ** (-20.0 + 38.0 * np.arange(nD * nC).reshape(nD, nC) / (nD * nC - 1)) / np.abs(m).max()
    m = m.astype(np.complex64).astype(np.complex128)
    delay = np.arange(-2, nC - 2)
    for min_delay, min_doppler in ((-128, 0.0), (0, 2.0)):
        a = O.cfar2d_bruteforce(m, delay, doppler, 1.5, 0.05, *window, min_delay, min_doppler)
        b = O.cfar2d_additive(m, delay, doppler, 1.5, 0.05, *window, min_delay, min_doppler, return_margin=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.allclose(a[2], b[2], rtol=0, atol=1e-12)
        assert b[3].shape == (nD, nC)
        if nC > 1 and min_delay == -128:
            assert len(a[0]) > 0


@pytest.mark.parametrize("group", sorted(X.groups()))
def test_crafted_detector_inputs_keep_clear_of_the_threshold(group):
    """The conditions test_cfar_crafted_gpu.py rests on, for every input it runs: the oracle puts no tested cell within
    1e-9 of its threshold (so the additive kernels are compared by plain set equality), and at most 1 % of the hits lie
    inside the summed-area kernels' per-cell band."""
    n_hits = 0
    for case in X.groups()[group]:
        e = X.expected(case)
        assert e.in_band == 0, (case.name, e.in_band)
        if case.kind != "nonfinite" and "sat" in case.kernels():
            assert e.sat_share <= 0.01, (case.name, e.sat_share)
        n_hits += sum(len(h) for h in e.hits)
    assert n_hits > 0


@FAST
@given(st.integers(2_000, 300_000), st.sampled_from([400.0, 1896.0, 2000.0, 2001.0]))
def test_spectrum_dims_invariants(n, bw):
    # SpectrumAnalyser.cpp:16-18 (n < bandwidth makes the reference divide by a zero decimation)
    if n < bw:
        return
    dec, ns, nfft = O.spectrum_dims(n, bw)
    assert dec == int(n / bw) and dec >= 1
    assert ns == n // dec and nfft == ns * dec <= n and n - nfft < dec
