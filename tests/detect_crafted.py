"""Crafted maps and hit lists for detect_finish_kernel (csrc/detect_kernels.hpp), shared by the CPU pin in
test_detect_inputs.py and by test_detect_dev_gpu.py: what the CPU test checks on these inputs (no interpolation
candidate within 1e-9 dB of a drop decision, every kept one curved by at least 1e-3 dB) is the condition under which the
GPU module may demand identical sets from the kernel and the host functions.

A case is a map shape with its axes (the arguments of ``Ambiguity``), a batch of seeded maps with distinct noisePower,
and per CPI a hit list in arbitrary order.  Nothing comes from the ambiguity engine or a detector: blah2hip_detect_dev
takes any device map and any list.  The reference is the host pair blah2hip_centroid / blah2hip_interpolate.
"""
from __future__ import annotations

import ctypes as C
import zlib
from dataclasses import dataclass

import numpy as np

import cfar_crafted as X

TILE = 1024                     # DET_TILE of csrc/detect_kernels.hpp: caps up to it run one workgroup per CPI
DECISION = 1e-9                 # dB: no candidate's peak test is closer to a tie than this ...
CURVATURE = 1e-3                # ... and every kept candidate's |s0 - 2 s1 + s2| is at least this
FLAGS = [(0, 0), (1, 0), (0, 1), (1, 1)]  # (do_delay, do_doppler)

SMALL = X.geom(41, 60, -3)      # 1 Hz steps; delays -3 ... 56: negative ones, and ones below nCentroid (uint16 wrap)
WIDE = X.geom(129, 300, -10)    # room for several thousand hits
ASYM, MIRROR = X.ASYM, X.MIRROR  # one-sided Doppler axes whose step is not a round number; delays from -10


@dataclass(frozen=True)
class Case:
    name: str
    geom: tuple = SMALL
    counts: tuple = (40,)       # hits per CPI (the batch is len(counts))
    cap: int = TILE             # records per CPI in the hit buffer; above TILE: the multi-workgroup form
    cap_out: int = 0            # 0 = cap
    over: int = 0               # added to the count WORD of every CPI whose list fills the cap (count > cap)
    n_centroid: tuple = (6, 6)  # nDelay, nDoppler
    res: str = "nominal"        # resolutionDoppler: "nominal" = fs / n like blah2.cpp:176-181, "step" = 1 / cpi, what the axis is built from
    features: bool = False      # the planted sites below come first in every list
    dense: bool = False         # the random hits of a CPI crowd into three eighths of the map

    @property
    def B(self):
        return len(self.counts)


def dims(case):
    return X.dims_of(case.geom)


def resolution(case):
    d = dims(case)
    if case.res == "step":
        return 1.0 / d.cpi
    return 1.0 / (float(case.geom[5]) / float(case.geom[4]))


def cell_db(z, noise):
    """10 log10|z| - noisePower of complex64 cells, in fp64 (Interpolate.cpp:50-52)."""
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(np.abs(np.asarray(z).astype(np.complex128))) - noise


def _plant(rng, m, nD, nC, nd, nf):
    """Sites far enough apart that no box of one reaches another; returns the cells to report as hits."""
    pitch = 2 * max(nd, nf) + 2
    sites = [(r, c) for r in range(3, nD - nf - 2, pitch) for c in range(3, nC - nd - 2, pitch)]
    hits = []
    for k, (r, c) in enumerate(sites):
        a = m[r, c] * 30.0
        kind = k % 10
        m[r, c] = a
        hits.append((r, c))
        if kind == 0:    # the :80 slip: lopsided along delay (estimate well above the cell), near-symmetric along Doppler
            m[r, c - 1], m[r, c + 1] = a * 0.9, a * 0.05
            m[r - 1, c], m[r + 1, c] = a * 0.5, a * 0.48
        elif kind == 1:  # flat along delay: 0/0
            m[r, c - 1] = m[r, c + 1] = a
        elif kind == 2:  # flat along Doppler
            m[r - 1, c] = m[r + 1, c] = a
        elif kind == 3:  # equal snr inside each other's box: both stay
            m[r + 1, c + 2] = a
            hits.append((r + 1, c + 2))
        elif kind == 4:  # exactly nd columns / nf rows / both away, weaker and stronger: on the box's edge
            for dr, dc, g in ((0, nd, 0.5), (nf, 0, 2.0), (nf, nd, 0.7), (nf - 1, nd - 1, 0.6)):
                m[r + dr, c + dc] = a * g
                hits.append((r + dr, c + dc))
        elif kind == 5:  # not a peak along delay
            m[r, c + 1] = a * 3.0
        elif kind == 6:  # not a peak along Doppler
            m[r - 1, c] = a * 3.0
        elif kind == 7:  # a weaker hit strictly inside the box
            m[r + 2, c - 2] = a * 0.5
            hits.append((r + 2, c - 2))
        # 8, 9: a clean peak
    edges = [(0, 5), (nD - 1, 7), (6, 0), (9, nC - 1), (0, 0), (nD - 1, nC - 1), (0, nC - 1), (nD - 1, 0), (1, 1), (nD - 2, nC - 2)]
    for r, c in edges:
        m[r, c] *= 25.0
    return hits + edges


def make(case):
    """-> maps complex64 [B, nD, nC], metrics float64 [B, 2], hits (row, col, snr) [B, cap], count words uint32 [B].
    Slots behind a list hold copies of its cells with an snr of 1e300: a kernel that read them would drop everything."""
    from blah2_amd.process import HIT_DTYPE
    d = dims(case)
    nD, nC, B = d.n_doppler_bins, d.n_delay_bins, case.B
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    maps = (np.sqrt(rng.exponential(1.0, (B, nD, nC))) * np.exp(2j * np.pi * rng.random((B, nD, nC)))).astype(np.complex64)
    metrics = np.stack([rng.uniform(-8.0, 8.0, B), rng.uniform(30.0, 60.0, B)], axis=1)
    hits = np.zeros((B, case.cap), dtype=HIT_DTYPE)
    words = np.zeros(B, dtype=np.uint32)
    for b, k in enumerate(case.counts):
        assert k <= case.cap and k <= nD * nC
        cells = _plant(rng, maps[b], nD, nC, *case.n_centroid) if case.features else []
        cells = cells[:k]
        if len(cells) < k:
            if case.dense:
                hr, hc = nD // 2, 3 * nC // 4
                r0, c0 = rng.integers(0, nD - hr + 1), rng.integers(0, nC - hc + 1)
                pool = [(r, c) for r in range(r0, r0 + hr) for c in range(c0, c0 + hc)]
            else:
                pool = [(r, c) for r in range(nD) for c in range(nC)]
            taken = set(cells)
            pool = [p for p in pool if p not in taken]
            for i in rng.permutation(len(pool))[:k - len(cells)]:
                cells.append(pool[i])
        assert len(cells) == k and len(set(cells)) == k
        order = rng.permutation(k)
        rr = np.array([cells[i][0] for i in order], dtype=np.int32)
        cc = np.array([cells[i][1] for i in order], dtype=np.int32)
        hits["row"][b, :k], hits["col"][b, :k] = rr, cc
        hits["snr"][b, :k] = cell_db(maps[b][rr, cc], metrics[b, 0])
        if 0 < k < case.cap:
            fill = np.arange(case.cap - k) % k
            hits["row"][b, k:], hits["col"][b, k:], hits["snr"][b, k:] = rr[fill], cc[fill], 1e300
        words[b] = k + (case.over if k == case.cap else 0)
    return maps, metrics, hits, words


def candidates(case, maps, metrics, hits, b, do_centroid=True):
    """The detections Interpolate is handed for CPI b (rows, cols, snr), by the host's blah2hip_centroid."""
    import blah2_amd
    d = dims(case)
    k = int(case.counts[b])
    h = hits[b, :k]
    if not do_centroid or k == 0:
        return h["row"].copy(), h["col"].copy(), h["snr"].copy()
    det = blah2_amd.Detection(h["col"].astype(np.float64) + float(d.delay[0]), d.doppler[h["row"]], h["snr"])
    out = blah2_amd.Centroid(case.n_centroid[0], case.n_centroid[1], resolution(case)).process(det)
    # Centroid keeps the order and the values of what it keeps: walk both lists
    key = list(zip(det.delay.tolist(), det.doppler.tolist(), det.snr.tolist()))
    keep, j = [], 0
    kept = list(zip(out.delay.tolist(), out.doppler.tolist(), out.snr.tolist()))
    for i, v in enumerate(key):
        if j < len(kept) and kept[j] == v:
            keep.append(i)
            j += 1
    assert j == len(kept)
    keep = np.array(keep, dtype=np.int64)
    return h["row"][keep].copy(), h["col"][keep].copy(), h["snr"][keep].copy()


def expected(case, maps, metrics, hits, b, do_centroid, do_delay, do_doppler):
    """{(row, col): (delay, doppler, snr)} of CPI b by the host functions, one blah2hip_interpolate call per candidate so
    that a survivor is known by the cell it came from."""
    from blah2_amd import _lib
    L = _lib.load()
    d = dims(case)
    rows, cols, snr = candidates(case, maps, metrics, hits, b, do_centroid)
    m = np.ascontiguousarray(maps[b])
    dax = np.ascontiguousarray(d.delay, dtype=np.int32)
    fax = np.ascontiguousarray(d.doppler, dtype=np.float64)
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    i3, o3, n = np.zeros(3), np.zeros(3), C.c_uint32(0)
    out = {}
    for r, c, s in zip(rows.tolist(), cols.tolist(), snr.tolist()):
        i3[:] = float(c + dax[0]), fax[r], s
        _lib.check(L.blah2hip_interpolate(vp(i3[0:]), vp(i3[1:]), vp(i3[2:]), 1, vp(m), m.shape[0], m.shape[1], vp(dax), vp(fax),
                                          float(metrics[b, 0]), int(do_delay), int(do_doppler), vp(o3[0:]), vp(o3[1:]), vp(o3[2:]),
                                          C.byref(n)))
        if n.value:
            out[(r, c)] = (float(o3[0]), float(o3[1]), float(o3[2]))
    return out


def triples(m, noise, rows, cols, along):
    """(s0, s1, s2, eq01, eq12) of the interior candidates along ``along`` ("delay" / "doppler"); eq: the two cells hold one
    bit pattern (then every implementation gets two equal values: that comparison cannot flip; all three: 0/0 everywhere)."""
    nD, nC = m.shape
    ok = (cols > 0) & (cols < nC - 1) if along == "delay" else (rows > 0) & (rows < nD - 1)
    r, c = rows[ok], cols[ok]
    dr, dc = (0, 1) if along == "delay" else (1, 0)
    z0, z1, z2 = m[r - dr, c - dc], m[r, c], m[r + dr, c + dc]
    return cell_db(z0, noise), cell_db(z1, noise), cell_db(z2, noise), z0 == z1, z1 == z2, ok


def margins(m, noise, rows, cols):
    """Smallest distance of a peak test from a tie, smallest curvature of a kept candidate, and the number of kept
    candidates whose delay-branch estimate lies above their Doppler-branch estimate (the :80 slip shows)."""
    tie, curv = np.inf, np.inf
    est = {}
    for along in ("delay", "doppler"):
        s0, s1, s2, eq01, eq12, ok = triples(m, noise, rows, cols, along)
        tie = min([tie] + np.abs(s1 - s0)[~eq01].tolist() + np.abs(s1 - s2)[~eq12].tolist())
        kept = ~(eq01 & eq12) & ~(s1 < s0) & ~(s1 < s2)
        if kept.any():
            curv = min(curv, np.abs(s0 - 2 * s1 + s2)[kept].min())
        with np.errstate(invalid="ignore", divide="ignore"):
            e = s1 - ((s0 - s2) * ((s0 - s2) / (2 * (s0 - 2 * s1 + s2)))) / 4
        idx = np.flatnonzero(ok)
        est[along] = {int(i): float(v) for i, v, k in zip(idx, e, kept) if k}
    slips = sum(1 for i, v in est["delay"].items() if i in est["doppler"] and v > est["doppler"][i] + 0.1)
    return tie, curv, slips


def cases():
    out = [Case("features", features=True, counts=(140,)),
           Case("features-step", features=True, counts=(140,), res="step", geom=ASYM, n_centroid=(6, 5)),
           Case("features-mirror", features=True, counts=(140,), res="step", geom=MIRROR, n_centroid=(4, 3)),
           Case("features-tiled", features=True, counts=(140,), cap=3000),
           Case("asym-nominal", geom=ASYM, counts=(900,), n_centroid=(6, 6)),
           Case("asym-step-dense", geom=ASYM, counts=(1000,), res="step", dense=True, n_centroid=(3, 5)),
           Case("mirror-step-dense", geom=MIRROR, counts=(1000,), res="step", dense=True, cap=2048, n_centroid=(6, 5))]
    for k in (0, 1, 255, 256, 257, TILE - 1, TILE):
        out.append(Case(f"count-{k}", counts=(k,), features=k >= 255))
        out.append(Case(f"count-{k}-tiled", counts=(k,), cap=2 * TILE, features=k >= 255))
    out += [Case(f"count-{TILE + 1}", counts=(TILE + 1,), cap=2 * TILE, features=True),
            Case("thousands", geom=WIDE, counts=(5000,), cap=8192, features=True),
            Case("thousands-dense", geom=WIDE, counts=(6000, 3000), cap=6000, dense=True, over=500),
            Case("overflow", counts=(TILE, 300), over=77, features=True),
            Case("overflow-tiled", geom=WIDE, counts=(2500, 10), cap=2500, over=1, features=True),
            Case("cap-out", counts=(400, 30, 0), features=True, cap_out=25),
            Case("cap-out-tiled", geom=WIDE, counts=(3000, 0, 40), cap=4096, features=True, cap_out=60)]
    return out


def batch_case(cap):
    rng = np.random.default_rng(64)
    counts = tuple(int(v) for v in rng.integers(0, 400, 72))
    counts = tuple(0 if i % 9 == 4 else k for i, k in enumerate(counts))
    return Case(f"batch-{cap}", counts=counts, cap=cap, features=True)
