"""Shared by tests/test_migrate_model.py (CPU), tests/test_migrate_gpu.py and tests/test_migrate_replay_gpu.py: the
geometries, the tables, the impulse-reference CPIs and the moving-echo scene of the range-migration tests.  No test in here, no
GPU, no library call.

(a) Impulse-reference CPIs.  The reference channel is 1 at the first sample of every pulse and 0 elsewhere, the surveillance
channel has a modulus uniform in [0.5, 1.5] and a uniform phase at every sample, and delayMin is 0: the range map is then
R[i][d] = y[i nCorr + d] (times a phase per pulse where the Doppler limits are asymmetric) -- known, all cells different, all
of one size, so that a sum along a wrong walk misses by a large part of the peak.

(b) The moving-echo scene.  fs 200 kHz, n 40 000, delays -3 .. 40, Doppler +-160 Hz, roundHamming: a 65 x 44 map with nCorr
615.  A unit-power white reference; one echo of amplitude 0.05 on Doppler bin +30 (row 62, 150.09 Hz) whose delay is 20 samples
in the middle of the CPI and falls by 8 samples over it, pulse by pulse (a phase ramp on the FFT of the whole reference per
pulse); white noise of sigma 0.3.  fc = f nCorr nD / 8 makes the physical table walk those 8 samples.

(c) Geometries off the grid of 32 pulses (EDGE_GEOMS: 21 x 64, 48 x 65, 81 x 200, 95 x 64, 7 x 64, by explicit bin counts) with
the cases the GPU tests run on them; ``reach``, the window arithmetic of walk_sum_kernel's two shapes restated, which
says what blocks, runs and windows a (geometry, table) case makes the kernels run; and ``block_edge_sum``, the definition with
the five ways of getting a partial last block, a partial last row group or a strip seam wrong.
"""
import numpy as np

from oracle import blah2_oracle as O

MAX_MIGRATION = 512  # BLAH2HIP_MAX_MIGRATION

# (delayMin, delayMax, dopplerMin, dopplerMax, fs, n), n_doppler_bins -> nD x nDelay; every one with roundHamming
GEOMS = {
    "g65x44": ((0, 43, -160, 160, 200_000, 40_000), 0),
    "g65x45": ((0, 44, -160, 160, 200_000, 40_000), 0),       # odd cell count: CPI 1 sits 8 bytes off a 16-byte boundary
    "g129x111": ((0, 110, -320, 320, 200_000, 40_000), 0),    # two column strips; shifts cross tile and strip seams
    "g2049x40": ((0, 39, -5000, 5000, 1_000_000, 204_900), 0),  # 65 blocks of 32 pulses
    "g64x44": ((0, 43, -160, 160, 200_000, 40_000), 64),      # the explicit even bin count
    "gasym": ((0, 43, -100, 220, 200_000, 40_000), 0),        # asymmetric Doppler limits: the reference channel is rotated
    # Doppler lengths off the grid of 32 pulses, and strips that are whole, interior or one column wide (EDGE_GEOMS below)
    "g21x64": ((0, 63, -160, 160, 200_000, 40_000), 21),      # one block of 21 pulses; row groups of 21 and of 16 + 5; one strip
    "g48x65": ((0, 64, -160, 160, 200_000, 40_000), 48),      # blocks of 32 + 16; row groups of 32 + 16; a strip of one column
    "g81x200": ((0, 199, -160, 160, 200_000, 40_000), 81),    # blocks of 32, 32, 17; four strips, two of them interior
    "g95x64": ((0, 63, -160, 160, 200_000, 40_000), 95),      # last block of 31 pulses; last row groups of 31 and of 15
    "g7x64": ((0, 63, -160, 160, 200_000, 40_000), 7),        # the map smaller than any row group and any block
}
SHAPES = {"g65x44": (65, 44), "g65x45": (65, 45), "g129x111": (129, 111), "g2049x40": (2049, 40), "g64x44": (64, 44),
          "gasym": (65, 44), "g21x64": (21, 64), "g48x65": (48, 65), "g81x200": (81, 200), "g95x64": (95, 64), "g7x64": (7, 64)}
# the physical table's walk, in cells, at every geometry
CELLS = {"g65x44": 4, "g65x45": 4, "g129x111": 9, "g2049x40": 15, "g64x44": 4, "gasym": 4,
         "g21x64": 4, "g48x65": 4, "g81x200": 9, "g95x64": 4, "g7x64": 4}
# the geometries off the 32-pulse grid, and what the GPU tests run on them: tables of tests/test_migrate_gpu.py (groups of 32
# rows), (bank, table) of tests/test_rate_bank_gpu.py (groups of 16 rows; "none" is no table)
EDGE_GEOMS = ("g21x64", "g48x65", "g81x200", "g95x64", "g7x64")
EDGE_MIGRATE_CASES = [(g, t) for g, ts in (("g21x64", ("physical", "limit", "jagged")),
                                           ("g48x65", ("physical", "reversed", "beyond", "limit", "jagged")),
                                           ("g81x200", ("physical", "beyond", "jagged")),
                                           ("g95x64", ("physical", "reversed", "beyond", "limit", "jagged")),
                                           ("g7x64", ("physical", "limit", "jagged"))) for t in ts]
EDGE_RATE_CASES = [("g21x64", "m2to2", "jagged"), ("g21x64", "three", "none"), ("g48x65", "uneven16", "physical"),
                   ("g48x65", "dup", "limit"), ("g81x200", "m2to2", "physical"), ("g81x200", "uneven16", "jagged"),
                   ("g95x64", "uneven16", "limit"), ("g95x64", "p0.5", "none"), ("g7x64", "m2to2", "physical")]
DB_TOL = 1e-3  # the project's gate for noisePower and maxPower, dB


def dims_of(name):
    limits, bins = GEOMS[name]
    d = O.ambiguity_dims(*limits, True, bins)
    assert (d.n_doppler_bins, d.n_delay_bins) == SHAPES[name]
    return d


def impulse_cpis(dims, n_cpi, seed, gap=0):
    """(x, y, stride): complex64 planes of ``n_cpi`` CPIs, ``stride`` samples from one CPI to the next (``gap`` samples of
    NaN between the planes' CPIs, which no kernel may read)."""
    rng = np.random.default_rng(seed)
    used = dims.n_doppler_bins * dims.n_corr
    stride = used + gap
    x = np.full(n_cpi * stride, np.nan + 1j * np.nan, dtype=np.complex64)
    y = x.copy()
    for c in range(n_cpi):
        xc = np.zeros(used, dtype=np.complex64)
        xc[::dims.n_corr] = 1.0
        mod = rng.uniform(0.5, 1.5, used)
        ph = rng.uniform(0.0, 2.0 * np.pi, used)
        x[c * stride:c * stride + used] = xc
        y[c * stride:c * stride + used] = (mod * np.exp(1j * ph)).astype(np.complex64)
    return x, y, stride


def fc_for(dims, cells):
    """The carrier at which the physical table's outermost row walks ``cells`` cells from the middle of the CPI to its end
    (a quarter cell more, so that the figure does not sit on a rounding tie)."""
    return 0.5 * float(np.abs(dims.doppler).max()) * dims.n_corr * (dims.n_doppler_bins - 1) / (cells + 0.25)


def physical(dims, fc):
    return -0.5 * dims.doppler * float(dims.n_corr) / fc


def tables(dims, cells):
    """name -> half walks.  ``physical`` walks ``cells`` cells; ``beyond`` walks past the map's last column, so that its outer
    rows keep only the central pulses; ``limit`` runs from exactly -MAX_MIGRATION to exactly +MAX_MIGRATION; ``jagged`` gives
    neighbouring rows opposite walks of up to the limit (the widest window a workgroup can meet)."""
    nD = dims.n_doppler_bins
    phys = physical(dims, fc_for(dims, cells))
    jag = np.where(np.arange(nD) % 2 == 0, 1.0, -1.0) * np.linspace(0.0, MAX_MIGRATION, nD) / (nD - 1)
    return {
        "physical": phys,
        "reversed": -phys,
        "beyond": physical(dims, fc_for(dims, dims.n_delay_bins + 16)),
        "limit": np.linspace(-MAX_MIGRATION, MAX_MIGRATION, nD) / (nD - 1),
        "jagged": jag,
    }


def zero_rows(half, nD):
    """The rows the library copies: rint(h[j] (nD - 1)) == 0."""
    return np.rint(np.asarray(half, dtype=np.float64) * float(nD - 1)) == 0


def reach(nD, nDelay, half, rows_per_group, cols=64, blk=32, lds_cells=4096):
    """The window arithmetic of walk_sum_kernel<8, 1> (rows_per_group 32) and walk_sum_kernel<4, 2> (16) restated: one dict for every
    (strip, row group, block of pulses) with ``nb`` the block's pulses, ``t0`` and ``t1`` the first and last 16-column tile of
    its window, ``Wc = 16 (t1 - t0 + 1)`` the staged cells of one pulse, ``P = min(32, lds_cells // Wc)`` the pulses of a run and
    ``pn`` the run lengths; with ``nTiles``, ``interior`` (the strip touches neither edge of the map) and ``live`` (a row of
    the group lies in the map and has a shift: walk_sum_kernel<8, 1> stages nothing for a group of copied rows).  Rows behind the
    map take the last row's half walk, as in the kernels.  ``half`` None is no table: every shift is 0."""
    h = np.zeros(nD) if half is None else np.asarray(half, dtype=np.float64)
    assert h.shape == (nD,)
    t = (2 * np.arange(nD) - (nD - 1)).astype(np.float64)
    n_tiles = -(-nDelay // 16)
    n_strips = -(-nDelay // cols)
    out = []
    for strip in range(n_strips):
        c0 = strip * cols
        for group in range(-(-nD // rows_per_group)):
            rows = np.minimum(group * rows_per_group + np.arange(rows_per_group), nD - 1)
            s = np.rint(h[rows][:, None] * t[None, :]).astype(np.int64)
            live = bool((np.rint(h[rows] * float(nD - 1)) != 0).any())
            for block, ib in enumerate(range(0, nD, blk)):
                nb = min(blk, nD - ib)
                lo, hi = int(s[:, ib:ib + nb].min()), int(s[:, ib:ib + nb].max())
                t0, t1 = (c0 + lo) >> 4, (c0 + cols - 1 + hi) >> 4
                Wc = 16 * (t1 - t0 + 1)
                P = min(blk, lds_cells // Wc)
                assert P >= 1
                pn = tuple(min(P, nb - cs) for cs in range(0, nb, P))
                out.append(dict(strip=strip, group=group, block=block, nb=nb, t0=t0, t1=t1, Wc=Wc, P=P, pn=pn, nTiles=n_tiles,
                                interior=0 < strip < n_strips - 1, live=live))
    return out


# what the cases on EDGE_GEOMS have to run: name -> predicate on a dict of reach()
REACH_ITEMS = {
    **{f"nb {n}": (lambda b, n=n: b["nb"] == n) for n in (7, 16, 17, 21, 31)},
    "a run with 16 < pn < 32": lambda b: any(16 < p < 32 for p in b["pn"]),
    "P < nb with a shorter last run": lambda b: b["P"] < b["nb"] and b["pn"][-1] < b["P"],
    "t0 < 0 and t1 >= nTiles at once": lambda b: b["t0"] < 0 and b["t1"] >= b["nTiles"],
    "an interior strip's window inside the map": lambda b: b["interior"] and 0 <= b["t0"] and b["t1"] < b["nTiles"],
}


def reach_suppliers(cases, rows_per_group, live_only):
    """item of REACH_ITEMS -> the (geometry, table) of ``cases`` with a block that has it (``live_only``: in a group that
    stages, see reach).  ``cases`` holds (geometry, table) pairs; table "none" is no table."""
    found = {item: [] for item in REACH_ITEMS}
    for geom, table in cases:
        dims = dims_of(geom)
        half = None if table == "none" else tables(dims, CELLS[geom])[table]
        blocks = [b for b in reach(*SHAPES[geom], half, rows_per_group) if b["live"] or not live_only]
        for item, has in REACH_ITEMS.items():
            if any(has(b) for b in blocks):
                found[item].append((geom, table))
    return found


BLOCK_EDGE_MUTANTS = ("last-block-dropped", "last-pulse-repeated", "upper-half-dropped", "tail-rows-clamped", "seam-zero")


def block_edge_sum(R, s, which=None, rows=None, chirp=None, rows_per_group=32, blk=32, cols=64):
    """M'[j][d] of the definition in fp64 (times ``chirp`` [nD] per pulse where given) for an integer shift table s[j][i], or
    one of BLOCK_EDGE_MUTANTS: what a kernel that sums in blocks of ``blk`` pulses, groups of ``rows_per_group`` rows and strips
    of ``cols`` columns gives when it mistreats a partial last block, a partial last group or a strip seam.  The rows not in
    ``rows`` stay zero."""
    assert which is None or which in BLOCK_EDGE_MUTANTS
    nD, nDelay = R.shape
    c = np.ones(nD, dtype=np.complex128) if chirp is None else np.asarray(chirp, dtype=np.complex128)
    d = np.arange(nDelay)
    ib, nb = (nD // blk) * blk, nD % blk  # the partial last block (nb 0: there is none)
    pulse = np.arange(nD)  # the pulse whose cell, shift and chirp a term takes
    turn = np.arange(nD)   # the pulse whose twiddle it takes
    if nb and which == "last-block-dropped":
        pulse = turn = np.arange(ib)
    elif nb and which == "last-pulse-repeated":
        pulse = np.r_[pulse, np.full(blk - nb, nD - 1)]
        turn = np.arange(ib + blk)
    elif nb > 16 and which == "upper-half-dropped":
        pulse = turn = np.arange(ib + 16)
    tail = (nD // rows_per_group) * rows_per_group if nD % rows_per_group else nD  # first row of a partial last group
    out = np.zeros((nD, nDelay), dtype=np.complex128)
    for j in (range(nD) if rows is None else np.flatnonzero(rows)):
        w = np.exp(-2j * np.pi * ((turn * ((j + nD // 2 + 1) % nD)) % nD) / nD)
        walk = s[nD - 1] if which == "tail-rows-clamped" and j >= tail else s[j]
        col = d[None, :] + walk[pulse][:, None]
        ok = (col >= 0) & (col < nDelay)
        if which == "seam-zero":
            ok &= col // cols == d[None, :] // cols
        out[j] = np.sum(np.where(ok, R[pulse[:, None], np.clip(col, 0, nDelay - 1)], 0.0) * (c[pulse] * w)[:, None], axis=0)
    return out


def block_edge_identity(which, s, nDelay, rows=None, rows_per_group=32, blk=32, cols=64):
    """The explicit conditions under which block_edge_sum's mutant ``which`` cannot differ from the truth on ``rows`` (all rows
    where None): it changes no read that lands in the map."""
    nD = s.shape[0]
    rows = np.ones(nD, bool) if rows is None else np.asarray(rows, bool)
    ib, nb = (nD // blk) * blk, nD % blk
    d = np.arange(nDelay)

    def lands(pulses):  # a read of these pulses by a summed row lands in the map
        col = d[None, None, :] + s[rows][:, pulses, None]
        return bool(((col >= 0) & (col < nDelay)).any())

    if which == "last-block-dropped":
        return nb == 0 or not lands(np.arange(ib, nD))
    if which == "last-pulse-repeated":
        return nb == 0 or not lands(np.arange(nD - 1, nD))
    if which == "upper-half-dropped":
        return nb <= 16 or not lands(np.arange(ib + 16, nD))  # no pulse 16 .. 31 in the partial block, or none that reads
    if which == "tail-rows-clamped":  # no partial last group, or its summed rows walk as the last row does
        tail = np.arange((nD // rows_per_group) * rows_per_group, nD) if nD % rows_per_group else np.arange(0)
        return all(np.array_equal(s[j], s[nD - 1]) for j in tail if rows[j])
    if which == "seam-zero":  # no read lands in the map and in another strip than its cell
        col = d[None, None, :] + s[rows][:, :, None]
        return not ((col >= 0) & (col < nDelay) & (col // cols != d // cols)).any()
    raise AssertionError(which)


def set_metrics64(z):
    """Map::set_metrics (Map.cpp:187-206) in fp64: (noisePower, maxPower) of one map."""
    with np.errstate(divide="ignore", invalid="ignore"):
        db = 10.0 * np.log10(np.abs(np.asarray(z).astype(np.complex128)))
    noise = db.mean()
    return noise, max(0.0, db.max()) - noise


# ---- (b) the moving-echo scene ----------------------------------------------------------------------------------------------
SCENE_LIMITS = (-3, 40, -160, 160, 200_000, 40_000)
SCENE_BIN, SCENE_ROW, SCENE_DELAY, SCENE_COL = 30, 62, 20, 23
SCENE_WALK, SCENE_AMP, SCENE_SIGMA = 8.0, 0.05, 0.3


def scene_dims():
    d = O.ambiguity_dims(*SCENE_LIMITS, True)
    assert (d.n_doppler_bins, d.n_delay_bins, d.n_corr) == (65, 44, 615)
    return d


def scene_fc(dims):
    return float(dims.doppler[SCENE_ROW]) * dims.n_corr * dims.n_doppler_bins / SCENE_WALK


def scene(seed=5, walk=SCENE_WALK):
    """(x, y) complex128 of SCENE_LIMITS[5] samples; ``walk`` 0 is the same echo at a fixed delay."""
    dims = scene_dims()
    n, nD, nC = dims.n_samples, dims.n_doppler_bins, dims.n_corr
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    noise = SCENE_SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    X = np.fft.fft(x)
    k = np.fft.fftfreq(n)  # cycles per sample
    f = float(dims.doppler[SCENE_ROW])
    t = np.arange(n) / dims.fs
    echo = np.zeros(n, dtype=np.complex128)
    for i in range(nD):
        tau = SCENE_DELAY - walk * (i - (nD - 1) / 2.0) / nD  # approaching: the delay falls
        seg = slice(i * nC, (i + 1) * nC if i + 1 < nD else n)
        echo[seg] = np.fft.ifft(X * np.exp(-2j * np.pi * k * tau))[seg]
    y = SCENE_AMP * echo * np.exp(2j * np.pi * f * t) + noise
    return x, y


def level_db(m, row, col):
    return 20.0 * np.log10(np.abs(m[row, col]))
