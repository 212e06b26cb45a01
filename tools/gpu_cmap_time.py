#!/usr/bin/env python3
"""Time per launch of cmap_kernel (the clutter-map detector) against nci_kernel on the same maps and against what plain copy
and read kernels reach, all in the same process.

    python tools/gpu_cmap_time.py [--launches 100] [--warmup 50] [--out profiles/r22_cmap_time.json]

configs[1] map size (513 x 411), n_cpi 24 and 256 per call, with and without the exceed plane (no hit list: the gate's
use), memory 8, normalised, on noise maps.  The kernel's time is the ambiguity handle's "cfar" slot (an event pair around
the launch), read after every call: the median of `--launches` calls behind `--warmup` untimed ones.  ALGORITHMIC bytes per
call: every map cell read once (8 n_cpi), b read and written (8), and n_cpi more with the exceed plane.

The yardsticks run in the same process: nci_kernel with W = 1 and one channel on the same maps (blah2hip_nci_set_timing's
slot; it reads the same bytes and writes a map per CPI), and the kernel's bytes through blah2hip_deblock_c32_dev (a
bit-exact copy kernel: half read, half written) and blah2hip_stream_read_dev (all read), an event pair per launch, median
of as many launches.  Nothing is compared with this code's own earlier runs.  One process; run it under a time limit."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG2 = (-10, 400, -256, 256, 2_000_000, 2_000_000)
MEMORY, PFA = 8, 1e-3
CASES = [(24, False), (24, True), (256, False), (256, True)]  # (n_cpi, exceed plane)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_cmap_time.json"))
    a = ap.parse_args()
    if a.launches < 50:
        sys.exit("at least 50 launches")
    import torch

    import blah2_amd as b2
    L = b2.load()
    max_cpi = max(n for n, _ in CASES)
    amb = b2.Ambiguity(*CFG2, True, max_batch=max_cpi)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    cells = nD * nC
    st = torch.cuda.current_stream().cuda_stream
    res = {"geometry": f"configs[1]: {nD} x {nC}", "memory": MEMORY, "launches": a.launches, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "cases": []}

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
        return statistics.median(us), min(us)

    maps = torch.randn((max_cpi, nD, nC, 2), dtype=torch.float32, device="cuda")
    met = torch.zeros((max_cpi, 2), dtype=torch.float64, device="cuda")
    met[:, 0] = -1.25  # the level of the noise: the mean of 10 log10 |z| of unit Gaussians
    out = torch.empty((max_cpi, nD, nC, 2), dtype=torch.float32, device="cuda")
    omet = torch.empty((max_cpi, 2), dtype=torch.float64, device="cuda")
    exc = torch.empty((max_cpi, nD, nC), dtype=torch.uint8, device="cuda")
    for n_cpi, plane in CASES:
        det = b2.ClutterMapDetector(amb, PFA, MEMORY, -128, 0.0)
        det.prepare()
        launch = lambda: det.process_dev(n_cpi, None, 0, None, maps.data_ptr(), met.data_ptr(), exc.data_ptr() if plane else None,  # noqa: E731
                                         None, st)
        for _ in range(a.warmup):
            launch()
        torch.cuda.synchronize()
        amb.set_timing(True)
        amb.get_timing()
        us = []
        for _ in range(a.launches):
            launch()
            ms, n = amb.get_timing()["cfar"]  # synchronises
            assert n == 1
            us.append(ms * 1e3)
        amb.set_timing(False)
        det.close()

        integ = b2.MapIntegrator(amb, 1, 1, 1)
        nlaunch = lambda: integ.process_dev(maps.data_ptr(), n_cpi, out.data_ptr(), omet.data_ptr(), n_cpi, None, st)  # noqa: E731
        for _ in range(a.warmup):
            nlaunch()
        torch.cuda.synchronize()
        integ.set_timing(True)
        integ.get_timing()
        nci = []
        for _ in range(a.launches):
            nlaunch()
            ms, n = integ.get_timing()["nci"]
            assert n == 1
            nci.append(ms * 1e3)
        integ.close()

        nbytes = cells * (8 * n_cpi + 8 + (n_cpi if plane else 0))
        block = 4096
        n_s = nbytes // 32 // block * block
        raw = torch.randn((2 * n_s, 2), dtype=torch.float32, device="cuda")
        x = torch.empty((n_s, 2), dtype=torch.float32, device="cuda")
        y = torch.empty((n_s, 2), dtype=torch.float32, device="cuda")
        copy_us, copy_min = median_us(lambda: b2.deblock_c32_dev(raw.data_ptr(), block, 0, n_s, 1, x.data_ptr(), y.data_ptr(), n_s, st))
        read_bytes = nbytes // 16 * 16
        src = torch.randn((read_bytes // 4,), dtype=torch.float32, device="cuda")
        read_us, read_min = median_us(lambda: b2._lib.check(L.blah2hip_stream_read_dev(src.data_ptr(), read_bytes, None, st)))
        cmap_us, nci_us = statistics.median(us), statistics.median(nci)
        case = {"n_cpi": n_cpi, "exceed_plane": plane, "cmap_us_median": cmap_us, "cmap_us_min": min(us), "cmap_bytes": nbytes,
                "cmap_gbs": nbytes / cmap_us / 1e3, "nci_us_median": nci_us, "nci_us_min": min(nci),
                "nci_bytes": cells * 16 * n_cpi, "cmap_over_nci_time": cmap_us / nci_us,
                "copy_kernel": "blah2hip_deblock_c32_dev", "copy_bytes": 32 * n_s, "copy_us_median": copy_us, "copy_us_min": copy_min,
                "copy_gbs": 32 * n_s / copy_us / 1e3, "read_us_median": read_us, "read_us_min": read_min,
                "read_gbs": read_bytes / read_us / 1e3}
        case["cmap_over_copy_rate"] = case["cmap_gbs"] / case["copy_gbs"]
        case["cmap_over_read_rate"] = case["cmap_gbs"] / case["read_gbs"]
        print(json.dumps(case), flush=True)
        res["cases"].append(case)
        del raw, x, y, src
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
