#!/usr/bin/env python3
"""Time per launch of walk_sum_kernel<4, 2> (the rate bank) against walk_sum_kernel<8, 1> (migrate_dev) on the same handle and range map, in the same process.

    python tools/gpu_rate_time.py [--launches 100] [--warmup 50] [--out profiles/r19_rate_time.json]

Two geometries: configs[1]'s 513 x 411 maps, 256 CPIs a call, and configs[2]'s 1025 x 2048 maps, 16 a call, each with the
physical migration table for fc = 204.64 MHz set, and banks of K = 1 ({0}: migrate_dev's own sums with the chirp multiply
added), 5 (-2 .. 2) and 16 (-8 .. 7).  The kernel's time is blah2hip_amb_set_timing's BLAH2HIP_K_DOPPLER around the one launch of
blah2hip_amb_rate_bank_dev (its metrics_kernel counts under BLAH2HIP_K_METRICS and is reported beside it), read after every
launch: the median of `--launches` launches behind `--warmup` untimed ones, out of place, with the index plane, on the range
map one process call left on the handle.

The yardstick is walk_sum_kernel<8, 1> (blah2hip_amb_migrate_dev) timed the same way on that handle and range map, scaled to the same
number of row sums: the bank sums K nD rows less the copied ones (a zero rate in a zero-shift row), migrate_dev its migrated
rows.  `per_row_sum_over_migrate` is (rate_us / row_sums) / (migrate_us / migrated_rows); above 1.0 is a finding to explain
from the source and the resource report.  The kernel is never compared with its own earlier runs.  `us_per_map` is what the
stage adds to a chain per CPI.  One process; run it under a time limit."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("configs[1]", (-10, 400, -256, 256, 2_000_000, 2_000_000), 256),
         ("configs[2]", (-24, 2023, -512, 512, 10_000_000, 10_000_000), 16)]
FC = 204.64e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_rate_time.json"))
    a = ap.parse_args()
    if a.launches < 50:
        sys.exit("at least 50 launches")
    import numpy as np
    import torch

    import blah2_amd as b2
    from blah2_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    res = {"launches": a.launches, "warmup": a.warmup, "fc": FC, "device": torch.cuda.get_device_name(0),
           "arch": torch.cuda.get_device_properties(0).gcnArchName, "cases": []}
    banks = [np.zeros(1), b2.rate_bank(2), np.arange(-8.0, 8.0)]

    for tag, geom, n_maps in CASES:
        amb = b2.Ambiguity(*geom, True, max_batch=n_maps)
        amb.set_hot_columns(0)
        amb.set_leak_compensation(0)
        nD, nC, n = amb.get_n_doppler_bins(), amb.get_n_delay_bins(), geom[5]
        table = amb.migration_table(FC)
        migrated = int((np.rint(table * (nD - 1)) != 0).sum())
        amb.set_migration(table)
        gen = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randint(-100, 101, (n_maps * n, 2), dtype=torch.int8, device="cuda", generator=gen)
        y = torch.randint(-100, 101, (n_maps * n, 2), dtype=torch.int8, device="cuda", generator=gen)
        maps = torch.empty((n_maps, nD, nC), dtype=torch.complex64, device="cuda")
        out = torch.empty_like(maps)
        index = torch.empty((n_maps, nD, nC), dtype=torch.uint8, device="cuda")
        met = torch.empty((n_maps, 2), dtype=torch.float64, device="cuda")
        amb.process_dev(b2.FMT_I8, x.data_ptr(), y.data_ptr(), n_maps, n, maps.data_ptr(), met.data_ptr(), st)
        torch.cuda.synchronize()

        def migrate():
            amb.migrate_dev(maps.data_ptr(), n_maps, out.data_ptr(), met.data_ptr(), st)

        def bank():
            amb.rate_bank_dev(maps.data_ptr(), n_maps, out.data_ptr(), index.data_ptr(), met.data_ptr(), st)

        def timed(launch):
            for _ in range(a.warmup):
                launch()
            torch.cuda.synchronize()
            amb.set_timing(True)
            amb.get_timing()
            us = {"doppler": [], "metrics": []}
            for _ in range(a.launches):
                launch()
                t = amb.get_timing()  # synchronises
                for k in us:
                    assert t[k][1] == 1
                    us[k].append(t[k][0] * 1e3)
            amb.set_timing(False)
            return us

        mig = timed(migrate)
        mig_us = statistics.median(mig["doppler"])
        for q in banks:
            amb.set_rates(q)
            t = timed(bank)
            rate_us, met_us = statistics.median(t["doppler"]), statistics.median(t["metrics"])
            row_sums = q.size * nD - int((q == 0).sum()) * (nD - migrated)
            case = {"config": tag, "map": f"{nD} x {nC}", "n_maps": n_maps, "rates": q.size, "bank": [float(v) for v in q],
                    "row_sums": row_sums, "workgroups_per_map": amb.info(_lib.INFO_RATE_GRID),
                    "rate_us_median": rate_us, "rate_us_min": min(t["doppler"]), "metrics_us_median": met_us,
                    "us_per_map": (rate_us + met_us) / n_maps, "rate_tflops": 16.0 * nD * row_sums * nC * n_maps / rate_us / 1e6,
                    "yardstick_kernel": "walk_sum_kernel<8, 1>", "migrate_us_median": mig_us, "migrate_us_min": min(mig["doppler"]),
                    "migrated_rows": migrated, "migrate_workgroups_per_map": amb.info(_lib.INFO_MIGRATE_GRID),
                    "per_row_sum_over_migrate": (rate_us / row_sums) / (mig_us / migrated)}
            print(json.dumps(case), flush=True)
            res["cases"].append(case)
        del x, y, maps, out, index, met
        amb.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
