"""CPU: the crafted maps of tests/metrics_crafted.py for the Map::set_metrics epilogues of the Doppler kernels, checked
without a device, on every scene tests/test_metrics_crafted_gpu.py hands to the GPU.

The geometry (1 Hz rows, 25 / 26 / 3 columns, the ragged tiles); the cells (every risky row and column occurs); the planted
cell is the map's maximum with the margins metrics_crafted.py states and no cell is exactly zero; the small-sample scenes lie
below 0 dB throughout; the sensitivity proof -- six wrong epilogues each move noisePower or maxPower by ten times
WRITTEN_DB_GATE or more wherever they apply; the NumPy emulation of db_of stays inside the gate against written_metrics;
and the case tables reach every form of the issue's table with three tiles or more per workgroup of each persistent one.

Measured here (printed by the tests): the weakest mutant is the planted cell counted twice on the largest map, 2049 x 26,
1.7e-3 dB of noisePower (3.2e-3 .. 4.1e-1 dB on the smaller maps); dropping it moves maxPower by 9.3 dB or more; a padding
column 2.3 dB or more; a max started at -inf 14 dB or more on the small-sample maps and nothing elsewhere; a carried-over
max moves maxPower by 1.3 dB or more on the descending batch (1.55 dB per step, less the lag overlap's 183 .. 200 of 200
samples); a stale last-tile partial 0.057 dB or more in the CPI it moves most.  The db_of emulation differs from
written_metrics by 9.1e-7 dB (noisePower) and 4.8e-6 dB (maxPower) at most.

Two things the planted scene cannot do, and who does them instead.  On a small-sample map the planted cell lies 15 .. 45 dB
from 0 dB, where one cell weighs little in the sum: a cell lost or doubled there moves noisePower by 2.8e-4 dB on the largest
map, so these two mutants are the ordinary scenes' to catch, on the same forms.  And a target at the band's edge loses up to
1.96 dB to its rotation within a pulse, more than a step of the ladder, so the rows go from zero Doppler outwards
(metrics_crafted.risky_cells): the peaks then descend CPI by CPI until the row list wraps, one or two CPIs before the end."""
import numpy as np
import pytest

import metrics_crafted as MC
from oracle import blah2_oracle as O

KEYS = MC.scene_keys()
IDS = [f"{k[0].nD}-{k[0].window}-{k[1]}" + ("-small" if k[2] else "") + ("-ch1" if len(k) > 3 else "") for k in KEYS]


def batch_of_key(k):
    return MC.batch(k[0], k[1], small=k[2], channel=k[3] if len(k) > 3 else 0)


def test_gate_is_under_its_cap():
    assert 0 < MC.WRITTEN_DB_GATE <= MC.WRITTEN_DB_CAP == 5e-5


@pytest.mark.parametrize("nD", list(MC.FORMS))
def test_geometry(nD):
    for w, ncol in (("w25", 25), ("w26", 26), ("w3", 3)):
        g = MC.geom(nD, w)
        d = MC.dims_of(g)
        assert (d.n_doppler_bins, d.n_delay_bins, d.n_corr, d.n_samples, d.doppler_middle) == (nD, ncol, 200, 200 * nD, 0)
        assert d.n_samples <= 410_000
        # 1 Hz rows: the planted Doppler lies exactly on its row; row nD // 2 is zero Doppler for odd nD, (nD - 1) // 2 for 64
        assert np.array_equal(d.doppler, np.arange(nD, dtype=np.float64) - (nD - 1) // 2)
        assert np.array_equal(d.delay, np.arange(MC.WINDOWS[w][0], MC.WINDOWS[w][1] + 1))
        assert d.nfft - d.n_corr >= 18  # one run of linear lags
    # ragged last tiles of the 25-column window: 16 + 9, 3 x 8 + 1, 6 x 4 + 1; 26 columns: rows of 208 bytes, 16-byte aligned
    assert (25 % 16, 25 % 8, 25 % 4) == (9, 1, 1) and (26 * 8) % 16 == 0 and (25 * 8) % 16 == 8


@pytest.mark.parametrize("nD", list(MC.FORMS))
@pytest.mark.parametrize("ncol", [25, 26, 3])
def test_risky_cells_reach_every_row_and_column(nD, ncol):
    cells = MC.risky_cells(nD, ncol, MC.batch_size(nD))
    assert 7 <= len(cells) <= 12 and (ncol == 3 or len(cells) >= 9)
    rows, cols = {r for r, _ in cells}, {k for _, k in cells}
    want_rows = {min(max(v, 0), nD - 1) for v in (0, 1, 63, 64, nD // 2 - 1, nD // 2, nD // 2 + 1, nD - 65, nD - 64, nD - 2, nD - 1)}
    want_cols = {min(max(v, 0), ncol - 1) for v in (0, 3, 4, 7, 8, 15, 16, ncol - 2, ncol - 1)}
    assert rows == want_rows and cols == want_cols
    if nD > 1025:  # doppler_tilew2_kernel: 32 workgroups, 8 quarter tiles per CPI of 25 or 26 columns
        assert len(cells) == 12 and 12 * 8 >= 3 * 32


def test_ladders():
    down, up = MC.ladder(12), MC.ladder(12, "up")
    assert down[0] == 0.5 and up == down[::-1]
    assert all(abs(down[c + 1] / down[c] - 0.7) < 1e-12 for c in range(11))


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_planted_cell_is_the_maximum(key):
    b = batch_of_key(key)
    small = key[2]
    worst_mean, worst_second = np.inf, np.inf
    for c, ref in enumerate(b["refs"]):
        db = MC.db_values(ref)
        assert np.isfinite(db).all() and np.abs(ref).min() > 0, f"cpi {c}: a cell is exactly zero"
        top = tuple(int(v) for v in np.unravel_index(np.argmax(db), db.shape))
        assert top == tuple(b["cells"][c]), f"cpi {c}: the maximum is at {top}, planted at {b['cells'][c]}"
        s = np.sort(db.ravel())
        above_mean, above_second = s[-1] - db.mean(), s[-1] - s[-2]
        worst_mean, worst_second = min(worst_mean, above_mean), min(worst_second, above_second)
        assert above_mean >= MC.MARGIN_MEAN_DB and above_second >= MC.MARGIN_SECOND_DB, (c, above_mean, above_second)
        assert above_mean <= 30.0
        if b["amps"][c] == 0.5:
            assert above_mean >= MC.TOP_MARGIN_MEAN_DB and above_second >= MC.TOP_MARGIN_SECOND_DB, (c, above_mean, above_second)
        if small:  # every cell below 0 dB: the running max never leaves its start
            assert s[-1] < 0 and -60 < db.mean() < -40
            assert O.map_metrics(ref)[1] == -O.map_metrics(ref)[0]
        else:
            assert s[0] > 30
    print(f"\n[{key[0].nD} {key[0].window} {key[1]}] planted cell above the mean >= {worst_mean:.2f} dB, above the second cell >= {worst_second:.2f} dB")


def test_zero_cpi_scene():
    for nD in MC.ONE_PER_CLASS:
        g = MC.geom(nD)
        z = MC.zero_cpi_of(g)
        b, plain = MC.batch(g, zero_cpi=z), MC.batch(g)
        assert 0 < z < len(b["refs"]) - 1
        assert not b["ys"][z].any() and b["xs"][z].any() and not b["refs"][z].any()
        with np.errstate(divide="ignore"):
            assert O.map_metrics(b["refs"][z]) == (-np.inf, np.inf)
        for c in range(len(b["refs"])):
            if c != z:
                assert np.array_equal(b["refs"][c], plain["refs"][c]) and np.abs(b["refs"][c]).min() > 0


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_every_mutant_moves_a_metric_by_ten_gates(key):
    b = batch_of_key(key)
    g, order, small = key[0], b["amps"][0] > b["amps"][-1], key[2]
    need = 10 * MC.WRITTEN_DB_GATE
    dbs = [MC.db_values(r) for r in b["refs"]]
    nC = dbs[0].shape[1]
    n_rows = len({r for r, _ in b["cells"]})
    assert len(dbs) - n_rows <= 2  # at most two steps behind the wrap of the row list
    least = {}
    stale = {w: [] for w in MC.TILE_WIDTHS}
    for c, db in enumerate(dbs):
        cell = tuple(b["cells"][c])
        noise, mx = O.map_metrics(b["refs"][c])
        assert (noise, mx) == MC._finish(float(db.sum()), float(db.max()), db.size)

        def moved(which, **kw):
            n2, m2 = MC.mutant(which, db, cell, **kw)
            dn, dm = abs(n2 - noise), abs(m2 - mx)
            key2 = which if which != "max-carried" else which + " (maxPower)"
            if which != "max-carried" or (order and c < n_rows):
                least[key2] = min(least.get(key2, np.inf), dm if which == "max-carried" else max(dn, dm))
            return dn, dm

        for which in ("dropped", "twice"):
            dn, dm = moved(which)
            # (a small-sample map's planted cell lies 15 .. 45 dB from 0 dB, where a cell weighs nothing in the sum: these
            # two are the ordinary scenes' to catch, on the same forms)
            assert small or dn >= need, (which, c, dn)
        assert moved("dropped")[1] >= (0 if small else MC.MARGIN_SECOND_DB)  # small: the max stays at its start, 0
        for width in MC.TILE_WIDTHS:
            if nC % width:
                assert moved("padding", width=width)[0] >= need
        dn, dm = moved("max-inf")
        assert (dm >= 10.0) if small else (dn == 0 and dm == 0)  # only a map below 0 dB sees where the max starts
        if c == 0:
            continue
        for width in MC.TILE_WIDTHS:
            dn, dm = MC.mutant("last-tile-stale", db, cell, db_prev=dbs[c - 1], width=width)
            stale[width].append(max(abs(dn - noise), abs(dm - mx)))
        dn, dm = moved("max-carried", db_prev=dbs[c - 1])
        if order and not small and c < n_rows:
            # descending, up to where the row list wraps: the CPI before is 1.55 dB taller, less the lag overlaps' ratio
            # (>= 183 / 200: 0.39 dB), plus what its row nearer zero Doppler adds
            assert dn == 0 and dm >= 1.0, ("max-carried", c, dm)
    # a stale last-tile partial is the one mutant whose size depends on how far two neighbouring CPIs' levels differ, and at
    # the ladder's weak end, where the channel noise sets the level, they hardly do.  A kernel that has it fails the batch
    # by one CPI: asked here are the CPI that moves most, by a hundred gates, and half the batch by ten
    for width, moves in stale.items():
        least[f"last-tile-stale/{width} (largest)"] = max(moves)
        assert max(moves) >= 10 * need and sum(v >= need for v in moves) >= len(moves) // 2, (width, moves)
    print(f"\n[{g.nD} {g.window} {key[1]}{' small' if small else ''}] least move per mutant, dB: " + ", ".join(f"{k} {v:.2e}" for k, v in least.items()))


@pytest.mark.parametrize("nD", [65, 513, 2049])
def test_db_of_emulation_stays_inside_the_gate(nD):
    b = MC.batch(MC.geom(nD))
    worst = [0.0, 0.0]
    for ref in b["refs"]:
        m32 = ref.astype(np.complex64)
        n1, m1 = MC.db_of_emulated(m32)
        n2, m2 = MC.written_metrics(m32)
        worst = [max(worst[0], abs(n1 - n2)), max(worst[1], abs(m1 - m2))]
    print(f"\n[nD {nD}] db_of emulation against written_metrics: noisePower {worst[0]:.2e} dB, maxPower {worst[1]:.2e} dB")
    assert worst[0] <= MC.WRITTEN_DB_GATE and worst[1] <= MC.WRITTEN_DB_GATE


def test_second_channel_shares_the_reference():
    for nD in (513, 1027):
        a, b = MC.batch(MC.geom(nD)), MC.batch(MC.geom(nD), channel=1)
        assert all(np.array_equal(u, v) for u, v in zip(a["xs"], b["xs"]))
        assert all(p != q for p, q in zip(a["cells"], b["cells"])) and a["amps"] == b["amps"][::-1]
        assert [r for r, _ in a["cells"]] == [r for r, _ in b["cells"]][::-1]


# ---- the case tables ------------------------------------------------------------------------------------------------------
TABLE = {65: "tile8 tile8k tile16 tile16wg sub4 column direct", 513: "tile8 tile8k tile16 tile16wg sub4 column direct pfa513",
         64: "tile8 tile16 sub4", 515: "tilew tilem column direct", 1025: "tilew tilem column direct",
         1027: "tilew2 tilew4 tilem column direct", 2049: "tilew2 tilew4 tilem column direct"}


def tiles_and_grid(case):
    """(tiles of the launch, workgroups) as csrc/capi.hip amb_tail_stage plans a persistent form under a forced grid."""
    nC = MC.dims_of(MC.geom(case.nD, case.window)).n_delay_bins
    B = len(MC.batch_of(case)["refs"])
    if case.form == "tilew2":
        tiles = -(-nC // 16) * B * 4
        return tiles, max(32, (min(tiles, case.grid) + 31) & ~31)
    width = {"tile8": 8, "tile8k": 8, "tile16": 16, "tile16wg": 16, "pfa513": 16, "tilew": 8, "tilew4": 8}[case.form]
    tiles = -(-nC // width) * B
    return tiles, min(tiles, case.grid)


def test_case_tables_reach_every_form():
    assert {nD: " ".join(f) for nD, f in MC.FORMS.items()} == TABLE
    down = {(c.form, c.nD, c.window) for c in MC.DESCENDING}
    assert down == {(f, nD, w) for nD in TABLE for f in TABLE[nD].split() for w in MC.WINDOWS}
    forms = {f for v in TABLE.values() for f in v.split()}
    assert {c.form for c in MC.ASCENDING} == forms
    for cases in (MC.SMALL_CASES, MC.ZERO_CASES):
        assert {c.form for c in cases} == forms and {c.nD for c in cases} == set(MC.ONE_PER_CLASS)
    assert any(c.form == "pfa513" and c.grid == 8 for c in MC.DESCENDING)
    ids = [MC.case_id(c) for c in MC.DESCENDING + MC.ASCENDING + MC.SMALL_CASES + MC.ZERO_CASES + MC.FEATURE_CASES]
    assert len(ids) == len(set(ids))
    for form in MC.PERSISTENT:
        steady = [c for c in MC.DESCENDING if c.form == form and c.grid and tiles_and_grid(c)[0] >= 3 * tiles_and_grid(c)[1]]
        assert steady, form
    for c in MC.DESCENDING + MC.ASCENDING + MC.SMALL_CASES + MC.ZERO_CASES + MC.FEATURE_CASES:
        assert (c.grid != 0) == (c.form in MC.PERSISTENT)
