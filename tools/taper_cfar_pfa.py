#!/usr/bin/env python3
"""False-alarm rates of the cell-averaging detectors on tapered noise (CPU only: the oracle's detectors on fp64 maps).

    python tools/taper_cfar_pfa.py [--maps 12] [--pfa 1e-3] [--out profiles/r17_taper_cfar_pfa.json]

Maps of unit-variance complex white noise, 513 x 411, through ``blah2_amd.taper_maps`` with each named window.  The stencil
runs along Doppler only: along delay the cells of a tapered map stay independent and identically distributed, so the 1-D
detector (which trains along delay) keeps its design pfa.  Along Doppler the cells within P bins of each other are
correlated: a 2-D training window that holds Doppler neighbours of the cell under test averages cells that move with it,
and averages fewer independent cells than it counts.  The table shows the measured rate over the design rate for the 1-D
detector (guard 2, train 6) and for the 2-D detector (delay guard 2, train 6; Doppler train 3) with a Doppler guard of 1
and with a Doppler guard of max(1, P).  Not a gate: figures for INTEGRATION.md."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS = ("none", "hann", "hamming", "blackman", "blackmanharris", "nuttall", "flattop")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=12)
    ap.add_argument("--pfa", type=float, default=1e-3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_taper_cfar_pfa.json"))
    a = ap.parse_args()
    from blah2_amd.process import doppler_taper, taper_gains, taper_maps
    from oracle import blah2_oracle as O
    nD, nC = 513, 411
    delay, doppler = np.arange(nC), np.arange(nD) - 256.0
    rng = np.random.default_rng(20261020)
    noise = [(rng.standard_normal((nD, nC)) + 1j * rng.standard_normal((nD, nC))) / math.sqrt(2.0) for _ in range(a.maps)]
    res = {"map": f"{nD} x {nC}", "maps": a.maps, "pfa": a.pfa, "cells": a.maps * nD * nC, "rows": []}
    for name in WINDOWS:
        taps = doppler_taper(name)
        P = taps.size - 1
        counts = {"1d": 0, "2d_guard1": 0, "2d_guardP": 0}
        for m in noise:
            t = taper_maps(m, taps)
            level = O.map_metrics(t)[0]
            counts["1d"] += O.cfar1d_fast(t, delay, doppler, level, a.pfa, 2, 6, 0, 0.0)[0].size
            counts["2d_guard1"] += O.cfar2d(t, delay, doppler, level, a.pfa, 2, 6, 1, 3, 0, 0.0)[0].size
            counts["2d_guardP"] += O.cfar2d(t, delay, doppler, level, a.pfa, 2, 6, max(1, P), 3, 0, 0.0)[0].size
        expect = a.pfa * res["cells"]
        row = {"window": name, "n_side": P, "enbw_bins": taper_gains(taps)[2], "expected_alarms": expect,
               **{k: v for k, v in counts.items()}, **{k + "_over_design": v / expect for k, v in counts.items()},
               "sigma_of_the_ratio": 1.0 / math.sqrt(expect)}
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
