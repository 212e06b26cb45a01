"""CPU: what tests/spectrum_crafted.py claims, before tests/test_spectrum_crafted_gpu.py relies on it.

1. the table's (D, nS, N, c, hq) are the oracle's, and it holds the edges it says it holds; 2. the inputs mean what they
say: closed-form impulse spectra, tones peaking on their bin, the off-comb tone leaving crumbs only, the reference within
FLOOR of the long-double definition on the chosen bins, folded_restatement (direct, and chirp on the chirp-z rows) within
FLOOR of the reference on every input; 3. the figure is sensitive: every planted defect of folded_restatement exceeds
1000 GATE on every row where its term exists, on two rows at least, and stays at the floor where it does not; 4. every input
is exact in the formats it is sent in."""
import numpy as np
import pytest

import spectrum_crafted as SC

IDS = [g.name for g in SC.GEOMS]


def is_chirp(g):
    return SC.path_of(g) == "chirpz"


def test_table_against_the_oracle():
    assert len(set(IDS)) == len(IDS)
    for g in SC.GEOMS:
        assert SC.derive(g.n, g.bw) == (g.D, g.nS, g.N, g.c, g.hq), g.name
        assert g.hq * g.D + g.c == g.N // 2 + 1 and g.N == g.nS * g.D <= g.n
    nS = {g.nS for g in SC.GEOMS}
    assert {1, 4096, 4097, 65536, 65537, 131072, 131073} <= nS
    assert min(nS - {1}) < SC.DFT_SLICES and any(SC.DFT_SLICES < v < SC.DFT_BINS for v in nS)
    assert {33, 65, 257} <= nS                                    # one past the DFT block, the fold's lanes, the reduce block
    assert {1, 2, 3} <= {g.D for g in SC.GEOMS} and {0, 1, 2, 3} <= {g.c for g in SC.GEOMS}
    for path in ("staged", "l2", "chirpz"):
        assert any(SC.path_of(g) == path and g.D > 1 for g in SC.GEOMS)
    assert sum(g.n > g.N for g in SC.GEOMS) >= 4 and any(g.n > g.N and is_chirp(g) for g in SC.GEOMS)
    assert SC.chirp_len(131072) == 2 * 131072 and SC.chirp_len(131073) == 524288 and SC.chirp_len(65537) == 262144
    # chunks of the fold on 256 compute units (the GPU test asserts the same on the device it runs on)
    assert SC.fold_chunks(SC.BY_NAME["d16"], 256) == (4, 4)        # nJ <= D / 4 chunks of >= 4: none empty at D = 16
    nJ, per = SC.fold_chunks(SC.BY_NAME["empty-chunk"], 256)
    assert per * (nJ - 1) >= SC.BY_NAME["empty-chunk"].D
    nJ, per = SC.fold_chunks(SC.BY_NAME["n10030"], 256)
    assert nJ == 251 and 0 < SC.BY_NAME["n10030"].D - per * (nJ - 1) < per   # a ragged last chunk


@pytest.mark.parametrize("name", IDS)
def test_inputs_and_floors(name):
    g = SC.BY_NAME[name]
    ks = SC.chosen_bins(g, 64 if g.N <= 16384 else 12)
    assert len(ks) <= 64 and {0, g.nS - 1, (g.nS - g.hq) % g.nS} <= set(ks)
    worst = {"definition": 0.0, "direct": 0.0, "chirp": 0.0}
    for cs in SC.cases(name):
        assert cs.x.shape == (g.n,) and cs.ref.shape == (g.nS,)
        assert np.array_equal(cs.x, np.rint(cs.x.real) + 1j * np.rint(cs.x.imag))
        assert max(np.abs(cs.x.real).max(), np.abs(cs.x.imag).max()) <= 32767           # exact in fp32
        if g.n > g.N:
            assert np.all(np.abs(cs.x[g.N:].real) == SC.TAIL) and np.all(np.abs(cs.x[g.N:].imag) == SC.TAIL)
        kind, _, at = cs.tag.partition("@")
        if kind == "impulse" and at != "tail":
            x, closed = SC.impulse(g, int(at))
            assert np.array_equal(x, cs.x) and np.allclose(np.abs(closed), 5000.0, rtol=1e-14)
            assert SC.err(cs.ref, closed) <= 1e-12
        elif kind == "impulse":
            assert not cs.x[:g.N].any() and cs.x[g.N:].all() and not cs.ref.any()
        elif kind == "tone":
            k = int(at)
            assert int(np.argmax(np.abs(cs.ref))) == k
            assert abs(abs(cs.ref[k]) / (1000.0 * g.N) - 1) < 1e-3
            if g.nS > 1:
                assert np.max(np.abs(np.delete(cs.ref, k))) <= 2e-3 * abs(cs.ref[k])    # rounding crumbs
        elif kind == "off-comb":
            assert np.max(np.abs(cs.ref)) <= 2e-3 * 1000.0 * g.N
            full = np.fft.fft(cs.x[:g.N])
            assert int(np.argmax(np.abs(full))) == SC.off_comb_bin(g) and SC.off_comb_bin(g) % g.D != g.c
        kk = sorted(set(ks) | ({int(at)} if kind == "tone" else set()))
        den = 1000.0 * g.N if cs.zero_ref else np.sqrt(np.mean(np.abs(cs.ref) ** 2))
        worst["definition"] = max(worst["definition"], float(np.max(np.abs(cs.ref[kk] - SC.definition(cs.x, g, kk))) / den))
        worst["direct"] = max(worst["direct"], SC.case_err(SC.folded_restatement(cs.x, g), cs, g))
        if is_chirp(g):
            worst["chirp"] = max(worst["chirp"], SC.case_err(SC.folded_restatement(cs.x, g, chirp=True), cs, g))
    print(f"\n[{name}] " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"  (FLOOR {SC.FLOOR:.1e})")
    assert max(worst.values()) <= SC.FLOOR, worst


@pytest.mark.parametrize("defect", SC.DEFECTS)
def test_planted_defects_are_caught(defect):
    shown = []
    for g in SC.GEOMS:
        cs = SC.noise_case(g.name)
        for chirp in ((False, True) if is_chirp(g) else (False,)):
            e = SC.case_err(SC.folded_restatement(cs.x, g, chirp=chirp, defect=defect), cs, g)
            if SC.defect_applies(defect, g, chirp):
                assert e > 1000 * SC.GATE, f"{defect} on {g.name} (chirp={chirp}): {e:.2e} would pass"
                shown.append((g.name, e))
            else:
                assert e <= SC.FLOOR, f"{defect} on {g.name} (chirp={chirp}): {e:.2e} where its term does not exist"
    print(f"\n[{defect}] " + "  ".join(f"{n} {e:.1e}" for n, e in shown))
    assert len({n for n, _ in shown}) >= 2, shown


def test_format_inputs_are_exact():
    for g in SC.GEOMS:
        x = SC.noise_plus_tone(g, 11, 100)
        assert np.array_equal(x, np.rint(x.real) + 1j * np.rint(x.imag))
        for part in (x.real, x.imag):
            assert np.abs(part).max() <= 100 and np.array_equal(part.astype(np.int8), part)
            assert np.array_equal(part.astype(np.float16).astype(np.float64), part)     # |v| <= 2048: exact in fp16
            assert np.array_equal(part.astype(np.float32).astype(np.float64), part)
        x = SC.noise_plus_tone(g, 12, 32767)
        for part in (x.real, x.imag):
            assert np.array_equal(part.astype(np.int16), part)
        q = SC.quarters(g, 13)
        for part in (q.real, q.imag):
            assert np.abs(part).max() <= 2048 and np.array_equal(part.astype(np.float16).astype(np.float64), part)
        if g.n >= 64:
            assert np.any(q.real != np.rint(q.real)) and np.any(np.abs(q.real) > 512)
