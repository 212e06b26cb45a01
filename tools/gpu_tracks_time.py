#!/usr/bin/env python3
"""Time per launch of track_power_kernel and track_sum_kernel (integration along tracks) against nci_kernel on the same case
and against what plain copy and read kernels reach, all in the same process.

    python tools/gpu_tracks_time.py [--launches 100] [--warmup 50] [--out profiles/r20_tracks_time.json]

configs[1] map size (513 x 411).  The three (n_surv, window, hop, n_cpi) cases of tools/gpu_nci_time.py with a zero walk and
the bank {0} -- there the output maps are nci_kernel's bit for bit, so nci_kernel's median on the same case is the
yardstick -- and (1, 8, 1, 24) under the physical walk table for 204.64 MHz with banks of 1, 5 and 16 rates.  The kernels'
times are blah2hip_nci_set_timing's slots (an event pair around each launch), read after every call: the median of
`--launches` calls behind `--warmup` untimed ones, which also fill the ring.  ALGORITHMIC bytes of the sum kernel per
call: 4 * window * K_bank gathered per output cell plus the 8-byte store (no index plane here), taken call by call because
n_out may differ; of the power kernel: every input cell read once, 4 bytes written per cell and CPI.

The byte yardsticks move the sum kernel's mean bytes in the same process: blah2hip_deblock_c32_dev (a bit-exact copy kernel:
half read, half written) and blah2hip_stream_read_dev (all read), an event pair per launch, median of as many launches.
Nothing is compared with this code's own earlier runs.  One process; run it under a time limit."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG2 = (-10, 400, -256, 256, 2_000_000, 2_000_000)
FC = 204.64e6
# (n_surv, window, hop, n_cpi, table, rates in the bank)
CASES = [(4, 1, 1, 6, "zero", 1), (1, 4, 1, 24, "zero", 1), (4, 4, 4, 6, "zero", 1),
         (1, 8, 1, 24, "physical", 1), (1, 8, 1, 24, "physical", 5), (1, 8, 1, 24, "physical", 16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_tracks_time.json"))
    a = ap.parse_args()
    if a.launches < 50:
        sys.exit("at least 50 launches")
    import numpy as np
    import torch

    import blah2_amd as b2
    L = b2.load()
    amb = b2.Ambiguity(*CFG2, True, max_batch=24)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    cells = nD * nC
    st = torch.cuda.current_stream().cuda_stream
    physical = b2.nci_walk_table(amb, FC)
    res = {"geometry": f"configs[1]: {nD} x {nC}", "fc": FC, "walk_cells_per_cpi_max": float(np.abs(physical).max()),
           "launches": a.launches, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
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

    for K, W, H, n_cpi, table, n_rates in CASES:
        maps = torch.randn((K, n_cpi, nD, nC, 2), dtype=torch.float32, device="cuda")
        out = torch.empty((n_cpi, nD, nC, 2), dtype=torch.float32, device="cuda")
        met = torch.empty((n_cpi, 2), dtype=torch.float64, device="cuda")
        bank = None if n_rates == 1 else np.linspace(-2.0, 2.0, n_rates)
        tracks, plain = b2.MapIntegrator(amb, K, W, H), b2.MapIntegrator(amb, K, W, H)
        tracks.set_tracks(None if table == "zero" else physical, bank, n_cpi)

        def timed(integ, launch, slots):
            for _ in range(a.warmup):
                launch()
            torch.cuda.synchronize()
            integ.set_timing(True)
            integ.get_timing()
            us, outs = {s: [] for s in slots}, []
            for _ in range(a.launches):
                outs.append(launch())
                t = integ.get_timing()  # synchronises
                for s in slots:
                    assert t[s][1] == (1 if s != "track_sum" or outs[-1] else 0)
                    us[s].append(t[s][0] * 1e3)
            return us, outs

        us, n_outs = timed(tracks, lambda: tracks.process_tracks_dev(maps.data_ptr(), n_cpi, out.data_ptr(), None, met.data_ptr(),
                                                                     n_cpi, None, st)[0], ("track_power", "track_sum"))
        nci, _ = timed(plain, lambda: plain.process_dev(maps.data_ptr(), n_cpi, out.data_ptr(), met.data_ptr(), n_cpi, None, st)[0],
                       ("nci",))
        shift = amb.info(b2._lib.INFO_TRACK_MAX_SHIFT)
        grid = amb.info(b2._lib.INFO_TRACK_GRID)
        tracks.close()
        plain.close()
        sum_bytes = [n * cells * (4 * W * n_rates + 8) for n in n_outs]
        pow_bytes = K * n_cpi * cells * 8 + n_cpi * cells * 4
        pairs = [(b, u) for b, u in zip(sum_bytes, us["track_sum"]) if b]
        mean_bytes = int(statistics.mean(b for b, _ in pairs))

        block = 4096
        n_s = mean_bytes // 32 // block * block
        raw = torch.randn((2 * n_s, 2), dtype=torch.float32, device="cuda")
        x = torch.empty((n_s, 2), dtype=torch.float32, device="cuda")
        y = torch.empty((n_s, 2), dtype=torch.float32, device="cuda")
        copy_us, copy_min = median_us(lambda: b2.deblock_c32_dev(raw.data_ptr(), block, 0, n_s, 1, x.data_ptr(), y.data_ptr(), n_s, st))
        read_bytes = mean_bytes // 16 * 16
        src = torch.randn((read_bytes // 4,), dtype=torch.float32, device="cuda")
        read_us, read_min = median_us(lambda: b2._lib.check(L.blah2hip_stream_read_dev(src.data_ptr(), read_bytes, None, st)))
        power_us, sum_us, nci_us = (statistics.median(us["track_power"]), statistics.median(u for _, u in pairs),
                                    statistics.median(nci["nci"]))
        case = {"n_surv": K, "window": W, "hop": H, "n_cpi": n_cpi, "table": table, "rates": n_rates, "max_shift": shift,
                "sum_grid_per_map": grid, "n_out_mean": statistics.mean(n_outs),
                "track_power_us_median": power_us, "track_power_us_min": min(us["track_power"]),
                "track_power_bytes": pow_bytes, "track_power_gbs": pow_bytes / power_us / 1e3,
                "track_sum_us_median": sum_us, "track_sum_us_min": min(u for _, u in pairs), "track_sum_bytes_mean": mean_bytes,
                "track_sum_gbs": statistics.median(b / u / 1e3 for b, u in pairs),
                "nci_us_median": nci_us, "nci_us_min": min(nci["nci"]),
                "tracks_over_nci_time": (power_us + sum_us) / nci_us,
                "copy_kernel": "blah2hip_deblock_c32_dev", "copy_bytes": 32 * n_s, "copy_us_median": copy_us, "copy_us_min": copy_min,
                "copy_gbs": 32 * n_s / copy_us / 1e3, "read_us_median": read_us, "read_us_min": read_min,
                "read_gbs": read_bytes / read_us / 1e3}
        case["track_sum_over_copy_rate"] = case["track_sum_gbs"] / case["copy_gbs"]
        case["track_sum_over_read_rate"] = case["track_sum_gbs"] / case["read_gbs"]
        print(json.dumps(case), flush=True)
        res["cases"].append(case)
        del maps, out, met, raw, x, y, src
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
