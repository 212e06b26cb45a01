#!/usr/bin/env python3
"""Time per launch of taper_kernel against what a plain read-plus-write kernel reaches in the same process.

    python tools/gpu_taper_time.py [--launches 100] [--warmup 50] [--out profiles/r17_taper_time.json]

Two map sets: configs[1]'s 513 x 411 maps, 256 a call, and configs[2]'s 1025 x 2048 maps, 16 a call; each with stencils
of half width P = 1 (Hann), 2 (Blackman) and 4 (flat top).  The kernel's time is blah2hip_amb_set_timing's BLAH2HIP_K_BEAM
(an event pair around the one launch; its metrics_kernel counts under BLAH2HIP_K_METRICS and is reported beside it), read
after every launch: the median of `--launches` launches behind `--warmup` untimed ones.  Its ALGORITHMIC bytes per launch:
every map read once and written once (2 * n_maps * cells * 8); the halo rows a segment shares with its neighbours are not
counted, so they show as a lower rate.

The yardstick moves the same number of bytes in the same process: blah2hip_deblock_c32_dev (a bit-exact copy kernel: half
the bytes read, half written) and blah2hip_stream_read_dev (all of them read), each bracketed by an event pair per launch,
median of as many launches.  The kernel's rate is reported as a fraction of the copy kernel's; it is never compared with
its own earlier runs.  `us_per_map` is what the taper adds to a chain per CPI.  One process; run it under a time limit."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("configs[1]", (-10, 400, -256, 256, 2_000_000, 2_000_000), 256),
         ("configs[2]", (-24, 2023, -512, 512, 10_000_000, 10_000_000), 16)]
WINDOWS = ("hann", "blackman", "flattop")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_taper_time.json"))
    ap.add_argument("--seg-rows", type=int, default=0, help="BLAH2HIP_OPT_TAPER_SEG_ROWS (0: the launch's own choice)")
    a = ap.parse_args()
    if a.launches < 50:
        sys.exit("at least 50 launches")
    import torch

    import blah2_amd as b2
    from blah2_amd import _lib
    L = b2.load()
    st = torch.cuda.current_stream().cuda_stream
    res = {"launches": a.launches, "warmup": a.warmup, "seg_rows_option": a.seg_rows, "device": torch.cuda.get_device_name(0),
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
        return statistics.median(us), min(us)

    for tag, geom, n_maps in CASES:
        amb = b2.Ambiguity(*geom, True, max_batch=n_maps)
        amb.set_taper_seg_rows(a.seg_rows)
        nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
        cells = nD * nC
        nbytes = 2 * n_maps * cells * 8
        maps = torch.randn((n_maps, nD, nC, 2), dtype=torch.float32, device="cuda")
        out = torch.empty_like(maps)
        met = torch.empty((n_maps, 2), dtype=torch.float64, device="cuda")

        # the same bytes through the copy kernel (half read, half written) and through the read kernel: complex samples
        # per channel (2 channels x 8 bytes, read and written), whole blocks only
        block = 4096
        n_s = nbytes // 32 // block * block
        raw = torch.randn((2 * n_s, 2), dtype=torch.float32, device="cuda")
        x = torch.empty((n_s, 2), dtype=torch.float32, device="cuda")
        y = torch.empty((n_s, 2), dtype=torch.float32, device="cuda")
        copy_us, copy_min = median_us(lambda: b2.deblock_c32_dev(raw.data_ptr(), block, 0, n_s, 1, x.data_ptr(), y.data_ptr(), n_s, st))
        del raw, x, y
        read_bytes = nbytes // 16 * 16
        src = torch.randn((read_bytes // 4,), dtype=torch.float32, device="cuda")
        read_us, read_min = median_us(lambda: _lib.check(L.blah2hip_stream_read_dev(src.data_ptr(), read_bytes, None, st)))
        del src
        copy_gbs, read_gbs = 32 * n_s / copy_us / 1e3, read_bytes / read_us / 1e3

        for name in WINDOWS:
            taps = b2.doppler_taper_f32(name)

            def launch():
                amb.taper_dev(maps.data_ptr(), n_maps, taps, out.data_ptr(), met.data_ptr(), st)
            for _ in range(a.warmup):
                launch()
            torch.cuda.synchronize()
            amb.set_timing(True)
            amb.get_timing()
            us, mus = [], []
            for _ in range(a.launches):
                launch()
                t = amb.get_timing()  # synchronises
                assert t["beam"][1] == 1 and t["metrics"][1] == 1
                us.append(t["beam"][0] * 1e3)
                mus.append(t["metrics"][0] * 1e3)
            amb.set_timing(False)
            taper_us = statistics.median(us)
            case = {"config": tag, "map": f"{nD} x {nC}", "n_maps": n_maps, "window": name, "n_side": len(taps) - 1,
                    "workgroups_per_map": amb.info(_lib.INFO_TAPER_GRID), "bytes": nbytes,
                    "taper_us_median": taper_us, "taper_us_min": min(us), "taper_gbs": nbytes / taper_us / 1e3,
                    "metrics_us_median": statistics.median(mus), "us_per_map": (taper_us + statistics.median(mus)) / n_maps,
                    "copy_kernel": "blah2hip_deblock_c32_dev", "copy_bytes": 32 * n_s, "copy_us_median": copy_us, "copy_us_min": copy_min,
                    "copy_gbs": copy_gbs, "read_us_median": read_us, "read_us_min": read_min, "read_gbs": read_gbs}
            case["taper_over_copy_rate"] = case["taper_gbs"] / copy_gbs
            case["taper_over_read_rate"] = case["taper_gbs"] / read_gbs
            print(json.dumps(case), flush=True)
            res["cases"].append(case)
        del maps, out, met
        amb.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
