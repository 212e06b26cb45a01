"""CPU suite: ``gocfar_hits``, the NumPy restatement of the greatest-of / smallest-of rule (include/blah2hip.h), against
the cell-by-cell statement ``rule`` of tests/gocfar_crafted.py on crafted maps; every deliberate mistake ``rule`` can make
(halves' counts swapped, a shared count, the averaging factor, and/or exchanged, column 0 training, k >= 0 in the leading
set, the guard or the row window off by one) changes the hit list of those maps; and the two scenes the detectors are for:
a 20 dB clutter edge, where the averaging detector reports the cells behind the step and greatest-of does not, and two
echoes five cells apart, which smallest-of keeps in every row."""
import numpy as np
import pytest

import gocfar_crafted as G

PFA = 0.02
WINDOWS = [(2, 6), (1, 4, 2)]


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    return blah2_amd


def axes(nD, nC):
    d = G.dims_of(G.geom(nD, nC))
    return d.delay, d.doppler


@pytest.mark.parametrize("kind", [G.GO, G.SO])
@pytest.mark.parametrize("window", WINDOWS + [(0, 127), (3, 0), (0, 2, 9)], ids=str)
def test_restatement_is_the_rule(b2, kind, window):
    """Noise with planted cells, a huge column 0, a NaN and a +Inf cell, with and without the skips; callable and dictionary."""
    nD, nC = 12, 40
    delay, doppler = axes(nD, nC)
    m = G.noise_map("go-model", nD, nC, 1, nonfinite=True)[0]
    al = G.factors(b2, PFA, kind)
    total = 0
    for skips in ({}, {"min_delay": int(delay[4]), "min_doppler": float(abs(doppler[3]))}):
        want = G.rule(m, delay, doppler, 3.0, al, kind, window, **skips)
        got = G.hits_dict(b2.gocfar_hits(m, delay, doppler, 3.0, al, kind, window, **skips))
        assert set(got) == set(want)
        assert all(got[c] == want[c] or abs(got[c] - want[c]) <= 1e-12 for c in want)
        total += len(want)
    a, b = b2.gocfar_counts(nD, nC, window)
    table = {(int(x), int(y)): al(int(x), int(y)) for x, y in zip(a.ravel(), b.ravel())}
    assert G.hits_dict(b2.gocfar_hits(m, delay, doppler, 3.0, table, kind, window)) == \
        G.hits_dict(b2.gocfar_hits(m, delay, doppler, 3.0, al, kind, window))
    assert total > 0 or window == (3, 0)
    assert (nD // 3, nC // 3) not in want  # the NaN cell
    assert len(b2.gocfar_hits(np.zeros_like(m), delay, doppler, 3.0, al, kind, window)[0]) == 0


@pytest.mark.parametrize("kind", [G.GO, G.SO])
@pytest.mark.parametrize("window", WINDOWS, ids=str)
def test_every_mistake_changes_the_hits(b2, kind, window):
    nD, nC = 12, 40
    delay, doppler = axes(nD, nC)
    al = G.factors(b2, PFA, kind)
    maps = [G.noise_map("go-model", nD, nC, 1)[0], G.flat_map(b2, PFA, kind, window, nD, nC)]
    right = [G.rule(m, delay, doppler, 3.0, al, kind, window) for m in maps]
    for m, r in zip(maps, right):
        assert G.hits_dict(b2.gocfar_hits(m, delay, doppler, 3.0, al, kind, window)) == pytest.approx(r, abs=1e-12)
    col = G.flat_col(window)
    assert ((1, col) in right[1]) == (kind == G.GO) and ((nD - 2, col) in right[1]) == (kind == G.GO)
    for variant in G.VARIANTS:
        if variant == "rows_minus_one" and len(window) == 2:
            continue  # the 1-D detector has no rows to lose
        wrong = [set(G.rule(m, delay, doppler, 3.0, al, kind, window, variant=variant)) for m in maps]
        changed = [len(w ^ set(r)) for w, r in zip(wrong, right)]
        print(kind, window, variant, changed)
        assert sum(changed) > 0, variant
        if variant in ("halves_swapped", "shared_count"):
            assert (1, col) in wrong[1] ^ set(right[1])
        if variant == "ca_factor":
            assert (nD - 2, col) in wrong[1] ^ set(right[1])


def behind_the_step(cells, step=64, n=10):
    return sum(1 for _, j in cells if step <= j < step + n)


def test_clutter_edge_scene(b2):
    """256 x 128 cells of complex Gaussian noise with a 20 dB power step at column 64; nGuard 2, nTrain 8, pfa 1e-3.  In the
    ten columns behind the step (2560 cells, 2.6 false alarms expected) the averaging detector reports many times that,
    greatest-of at most a third of it, smallest-of more."""
    rng = np.random.default_rng(20261021)
    m = G.step_scene(rng)
    delay, doppler = axes(256, 128)
    ca = G.ca_hits(b2, m, (2, 8), 1e-3)
    go = set(G.hits_dict(b2.gocfar_hits(m, delay, doppler, 0.0, G.factors(b2, 1e-3, G.GO), G.GO, (2, 8))))
    so = set(G.hits_dict(b2.gocfar_hits(m, delay, doppler, 0.0, G.factors(b2, 1e-3, G.SO), G.SO, (2, 8))))
    n_ca, n_go, n_so = behind_the_step(ca), behind_the_step(go), behind_the_step(so)
    print("behind the step: CA", n_ca, "GO", n_go, "SO", n_so, "| whole map: CA", len(ca), "GO", len(go), "SO", len(so))
    assert n_ca >= 10 and 3 * n_go <= n_ca and n_so > n_ca


def test_two_echoes_scene(b2):
    """The same noise without the step, two echoes of 17 dB over noise five cells apart in every row: smallest-of reports
    both columns in every row, the averaging detector and greatest-of do not."""
    rng = np.random.default_rng(20261022)
    m = G.pair_scene(rng)
    delay, doppler = axes(256, 128)
    ca = G.ca_hits(b2, m, (2, 8), 1e-3)
    go = set(G.hits_dict(b2.gocfar_hits(m, delay, doppler, 0.0, G.factors(b2, 1e-3, G.GO), G.GO, (2, 8))))
    so = set(G.hits_dict(b2.gocfar_hits(m, delay, doppler, 0.0, G.factors(b2, 1e-3, G.SO), G.SO, (2, 8))))
    kept = {name: [sum(1 for i in range(256) if (i, c) in cells) for c in (60, 65)] for name, cells in (("CA", ca), ("GO", go), ("SO", so))}
    print("rows of 256 that keep column 60 / 65:", kept)
    assert kept["SO"] == [256, 256]
    assert max(kept["CA"]) < 256 and max(kept["GO"]) < 256 and max(kept["GO"]) < min(kept["CA"])
