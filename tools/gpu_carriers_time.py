#!/usr/bin/env python3
"""Time per launch of carrier_sum_kernel against what a plain read-plus-write kernel reaches in the same process.

    python tools/gpu_carriers_time.py [--launches 100] [--warmup 50] [--out profiles/carriers_time.json]

configs[1] map size (513 x 411), C = 4 and 8 carriers, n_cpi = 64, both interpolations, the ratios (1, 1.004, 0.996, 1.02)
repeated.  The kernel's time is blah2hip_amb_set_timing's BLAH2HIP_K_BEAM (an event pair around the one launch; its
metrics_kernel counts under BLAH2HIP_K_METRICS), read after every launch.  Its ALGORITHMIC bytes per launch: every input map
read once and every output map written once, (C + 1) * cells * 8 per CPI (with linear interpolation a source row is read
by two output rows: the second read is L2's, not counted).

The yardstick moves the same bytes in the same process: blah2hip_deblock_c32_dev (a bit-exact copy kernel: half the bytes
read, half written) and blah2hip_stream_read_dev (all of them read), each bracketed by an event pair per launch.  The three
ALTERNATE: two rounds of (kernel, copy, read), each `--launches` / 2 timed launches behind `--warmup` / 2 untimed ones, the
median over both rounds.  The kernel's rate is reported as a fraction of the copy kernel's; it is never compared with its
own earlier runs.  One process; run it under a time limit."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG2 = (-10, 400, -256, 256, 2_000_000, 2_000_000)
RATIOS = (1.0, 1.004, 0.996, 1.02)
N_CPI = 64
CASES = [(4, "nearest"), (4, "linear"), (8, "nearest"), (8, "linear")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "carriers_time.json"))
    a = ap.parse_args()
    if a.launches < 50:
        sys.exit("at least 50 launches")
    import torch

    import blah2_amd as b2
    L = b2.load()
    amb = b2.Ambiguity(*CFG2, True, max_batch=8 * N_CPI)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    cells = nD * nC
    st = torch.cuda.current_stream().cuda_stream
    res = {"geometry": f"configs[1]: {nD} x {nC}", "n_cpi": N_CPI, "launches": a.launches, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "cases": []}

    def timed(enqueue, n):
        us = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            enqueue()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        return us

    out = torch.empty((N_CPI, nD, nC, 2), dtype=torch.float32, device="cuda")
    met = torch.empty((N_CPI, 2), dtype=torch.float64, device="cuda")
    for C_, interp in CASES:
        maps = torch.randn((C_, N_CPI, nD, nC, 2), dtype=torch.float32, device="cuda")
        amb.set_carriers([RATIOS[c % len(RATIOS)] for c in range(C_)], interp)
        nbytes = (C_ + 1) * cells * 8 * N_CPI
        block = 4096
        n_s = nbytes // 32 // block * block  # complex samples per channel: 2 channels x 8 bytes, read and written
        raw = torch.randn((2 * n_s, 2), dtype=torch.float32, device="cuda")
        x = torch.empty((n_s, 2), dtype=torch.float32, device="cuda")
        y = torch.empty((n_s, 2), dtype=torch.float32, device="cuda")
        read_bytes = nbytes // 16 * 16
        src = torch.randn((read_bytes // 4,), dtype=torch.float32, device="cuda")

        def fuse():
            amb.fuse_carriers_dev(maps.data_ptr(), N_CPI, out.data_ptr(), met.data_ptr(), None, st)

        def copy():
            b2.deblock_c32_dev(raw.data_ptr(), block, 0, n_s, 1, x.data_ptr(), y.data_ptr(), n_s, st)

        def read():
            b2._lib.check(L.blah2hip_stream_read_dev(src.data_ptr(), read_bytes, None, st))

        fuse_us, copy_us, read_us = [], [], []
        for _ in range(2):
            for _ in range(a.warmup // 2):
                fuse()
            torch.cuda.synchronize()
            amb.set_timing(True)
            amb.get_timing()
            for _ in range(a.launches // 2):
                fuse()
                ms, n = amb.get_timing()["beam"]  # synchronises
                assert n == 1
                fuse_us.append(ms * 1e3)
            amb.set_timing(False)
            for fn, dst in ((copy, copy_us), (read, read_us)):
                for _ in range(a.warmup // 2):
                    fn()
                torch.cuda.synchronize()
                dst += timed(fn, a.launches // 2)
        med = statistics.median
        case = {"carriers": C_, "interp": interp, "bytes": nbytes, "grid_per_map": amb.info(b2._lib.INFO_CARRIER_GRID),
                "fuse_us_median": med(fuse_us), "fuse_us_min": min(fuse_us), "fuse_gbs": nbytes / med(fuse_us) / 1e3,
                "copy_kernel": "blah2hip_deblock_c32_dev", "copy_bytes": 32 * n_s, "copy_us_median": med(copy_us),
                "copy_us_min": min(copy_us), "copy_gbs": 32 * n_s / med(copy_us) / 1e3,
                "read_us_median": med(read_us), "read_us_min": min(read_us), "read_gbs": read_bytes / med(read_us) / 1e3}
        case["fuse_over_copy_rate"] = case["fuse_gbs"] / case["copy_gbs"]
        case["fuse_over_read_rate"] = case["fuse_gbs"] / case["read_gbs"]
        print(json.dumps(case), flush=True)
        res["cases"].append(case)
        del maps, raw, x, y, src
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
