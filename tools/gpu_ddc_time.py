#!/usr/bin/env python3
"""Time per launch of the down-converter's kernel (ddc_kernel) against the copy rates measured in the same process and
against the fp32 issue floor of its multiply-adds.

    python tools/gpu_ddc_time.py [--launches 20] [--warmup 5] [--out profiles/r24_ddc_time.json]

N = 2 * 10^7 input samples per row, rows 1 and 16, FMT_C32 planes and FMT_I16 words, (D, T, C) in (10, 80, 1),
(10, 160, 1), (10, 160, 4), (10, 160, 8), (50, 800, 1), (50, 800, 8).  The kernel's time is its slot of
blah2hip_ddc_get_timing (an event pair around the launch), read after every call: the median of `--launches` calls behind
`--warmup` untimed ones.

ALGORITHMIC bytes: every input sample read once (16 bytes a sample pair as fp32 planes, 8 as .rspduo words), every output
written once (16 C / D bytes a sample pair).  Two yardsticks over the call's bytes: blah2hip_stream_read_dev (loads only)
and blah2hip_deblock_c32_dev (a bit-exact copy kernel: half read, half written).  Multiply-adds: 8 C T / D per sample
pair; the floor is those over the vector ALU's 78.6 T fused multiply-adds a second.  There is no pass/fail time: the
fractions are the result, against the copy kernels and the floor, never against this kernel's own earlier runs.
One process; run it under a time limit."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, FS = 20_000_000, 20_000_000.0
ROWS = (1, 16)
CASES = ((10, 80, 1), (10, 160, 1), (10, 160, 4), (10, 160, 8), (50, 800, 1), (50, 800, 8))
FMA_PER_S = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_ddc_time.json"))
    a = ap.parse_args()
    if a.launches < 10:
        sys.exit("at least 10 launches")
    import torch

    import blah2_amd as b2
    L = b2.load()
    st = torch.cuda.current_stream().cuda_stream
    res = {"n_in": N, "launches": a.launches, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "arch": torch.cuda.get_device_properties(0).gcnArchName, "cases": []}

    def median_us(enqueue):
        for _ in range(a.warmup):
            enqueue()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            enqueue()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(us)

    Rmax, Cmax, Dmin = max(ROWS), max(c[2] for c in CASES), min(c[0] for c in CASES)
    x = torch.randn((Rmax, N, 2), dtype=torch.float32, device="cuda")
    y = torch.randn((Rmax, N, 2), dtype=torch.float32, device="cuda")
    iq = torch.randint(-32768, 32768, (Rmax, N, 4), dtype=torch.int16, device="cuda")
    ox = torch.empty((Cmax * Rmax * (N // Dmin), 2), dtype=torch.float32, device="cuda")
    oy = torch.empty((Cmax * Rmax * (N // Dmin), 2), dtype=torch.float32, device="cuda")
    yard = {}

    def yardsticks(nbytes):
        """(read GB/s, copy GB/s) over nbytes, measured once per byte count."""
        if nbytes not in yard:
            block = 4096
            n_s = max(block, nbytes // 32 // block * block)
            raw = torch.randn((2 * n_s, 2), dtype=torch.float32, device="cuda")
            cx = torch.empty((n_s, 2), dtype=torch.float32, device="cuda")
            cy = torch.empty((n_s, 2), dtype=torch.float32, device="cuda")
            us_c = median_us(lambda: b2.deblock_c32_dev(raw.data_ptr(), block, 0, n_s, 1, cx.data_ptr(), cy.data_ptr(), n_s, st))
            us_r = median_us(lambda: b2._lib.check(L.blah2hip_stream_read_dev(raw.data_ptr(), 16 * n_s, None, st)))
            yard[nbytes] = (16 * n_s / us_r / 1e3, 32 * n_s / us_c / 1e3)
            del raw, cx, cy
        return yard[nbytes]

    for D, T, Cn in CASES:
        h = b2.ddc_design(D, T)
        offs = [FS * (0.37 * (c + 1) / (Cn + 1) - 0.2) for c in range(Cn)]
        ch = b2.Channelizer(FS, D, h, offs, N, max_rows=Rmax)
        n_out = N // D
        for rows in ROWS:
            for name, fmt, px, py, in_b in (("C32", b2.FMT_C32, x.data_ptr(), y.data_ptr(), 16), ("I16", b2.FMT_I16, iq.data_ptr(), None, 8)):
                launch = lambda: ch.process_dev(fmt, px, py, N, rows, N, ox.data_ptr(), oy.data_ptr(), n_out, rows * n_out, st)  # noqa: E731
                for _ in range(a.warmup):
                    launch()
                torch.cuda.synchronize()
                ch.set_timing(True)
                ch.get_timing()
                t = {"ddc": [], "ddc_tail": []}
                for _ in range(a.launches):
                    launch()
                    got = ch.get_timing()  # synchronises
                    for k in t:
                        assert got[k][1] == 1
                        t[k].append(got[k][0] * 1e3)
                ch.set_timing(False)
                us = {k: statistics.median(v) for k, v in t.items()}
                nbytes = rows * (N * in_b + 16 * Cn * n_out)
                read_gbs, copy_gbs = yardsticks(nbytes)
                fma = 8 * Cn * T * n_out * rows
                case = {"decim": D, "taps": T, "carriers": Cn, "rows": rows, "format": name, "tile": ch.tile, "ct_over_d": Cn * T / D,
                        "ddc_us_median": us["ddc"], "tail_us_median": us["ddc_tail"], "bytes": nbytes, "ddc_gbs": nbytes / us["ddc"] / 1e3,
                        "copy_gbs_same_bytes": copy_gbs, "read_gbs_same_bytes": read_gbs, "fma": fma,
                        "issue_floor_us": fma / FMA_PER_S * 1e6}
                case["over_copy_rate"] = case["ddc_gbs"] / copy_gbs
                case["over_read_rate"] = case["ddc_gbs"] / read_gbs
                case["issue_floor_over_time"] = case["issue_floor_us"] / us["ddc"]
                case["bound"] = "vector ALU issue" if case["issue_floor_over_time"] > case["over_copy_rate"] else "memory"
                print(json.dumps(case), flush=True)
                res["cases"].append(case)
        ch.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
