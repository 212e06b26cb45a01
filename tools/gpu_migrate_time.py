#!/usr/bin/env python3
"""Time per launch of walk_sum_kernel<8, 1> (blah2hip_amb_migrate_dev) against the direct Doppler kernel of the same handle, in the same process.

    python tools/gpu_migrate_time.py [--launches 100] [--warmup 50] [--out profiles/r18_migrate_time.json]

Two geometries: configs[1]'s 513 x 411 maps, 256 CPIs a call, and configs[2]'s 1025 x 2048 maps, 16 a call, each with the
physical table for fc = 204.64 MHz.  The kernel's time is blah2hip_amb_set_timing's BLAH2HIP_K_DOPPLER around the one launch
of blah2hip_amb_migrate_dev (its metrics_kernel counts under BLAH2HIP_K_METRICS and is reported beside it), read after every
launch: the median of `--launches` launches behind `--warmup` untimed ones, out of place, on the range map one process call
left on the handle.

The yardstick is doppler_dft_kernel (BLAH2HIP_DOP_DIRECT forced, hot columns and leak compensation off, so that the Doppler
bracket holds that one kernel) over the same CPIs on the same handle: the same complex multiply-adds per cell -- nD of them
-- without the walk.  The kernel sums only the rows that are not zero-shift rows, so the yardstick's time is scaled by
their share.  `migrate_over_yardstick` above 1.5 is a finding to explain.  The kernel is never compared with its own earlier
runs.  `us_per_map` is what the stage adds to a chain per CPI.  One process; run it under a time limit."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_migrate_time.json"))
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

    for tag, geom, n_maps in CASES:
        amb = b2.Ambiguity(*geom, True, max_batch=n_maps)
        amb.set_hot_columns(0)
        amb.set_leak_compensation(0)
        amb.set_doppler_kernel(_lib.DOP_DIRECT)
        nD, nC, n = amb.get_n_doppler_bins(), amb.get_n_delay_bins(), geom[5]
        table = amb.migration_table(FC)
        shifts = b2.migration_shifts(table, nD)
        migrated = int((np.rint(table * (nD - 1)) != 0).sum())
        amb.set_migration(table)
        gen = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randint(-100, 101, (n_maps * n, 2), dtype=torch.int8, device="cuda", generator=gen)
        y = torch.randint(-100, 101, (n_maps * n, 2), dtype=torch.int8, device="cuda", generator=gen)
        maps = torch.empty((n_maps, nD, nC), dtype=torch.complex64, device="cuda")
        out = torch.empty_like(maps)
        met = torch.empty((n_maps, 2), dtype=torch.float64, device="cuda")

        def process():
            amb.process_dev(b2.FMT_I8, x.data_ptr(), y.data_ptr(), n_maps, n, maps.data_ptr(), met.data_ptr(), st)

        def migrate():
            amb.migrate_dev(maps.data_ptr(), n_maps, out.data_ptr(), met.data_ptr(), st)

        def timed(launch, slots):
            for _ in range(a.warmup):
                launch()
            torch.cuda.synchronize()
            amb.set_timing(True)
            amb.get_timing()
            us = {k: [] for k in slots}
            for _ in range(a.launches):
                launch()
                t = amb.get_timing()  # synchronises
                for k in slots:
                    assert t[k][1] == 1
                    us[k].append(t[k][0] * 1e3)
            amb.set_timing(False)
            return us

        direct = timed(process, ("doppler",))["doppler"]
        assert amb.last_doppler_kernel() == _lib.DOPPLER_KERNEL_NAMES[_lib.DOP_DIRECT]
        mig = timed(migrate, ("doppler", "metrics"))
        direct_us, mig_us, met_us = statistics.median(direct), statistics.median(mig["doppler"]), statistics.median(mig["metrics"])
        yard_us = direct_us * migrated / nD
        flop = 8.0 * nD * migrated * nC * n_maps  # a complex multiply-add is 8 flop
        case = {"config": tag, "map": f"{nD} x {nC}", "n_maps": n_maps, "largest_shift": int(np.abs(shifts).max()),
                "migrated_rows": migrated, "rows": nD, "workgroups_per_map": amb.info(_lib.INFO_MIGRATE_GRID),
                "migrate_us_median": mig_us, "migrate_us_min": min(mig["doppler"]), "metrics_us_median": met_us,
                "us_per_map": (mig_us + met_us) / n_maps, "migrate_tflops": flop / mig_us / 1e6,
                "direct_kernel": "doppler_dft_kernel", "direct_us_median": direct_us, "direct_us_min": min(direct),
                "yardstick_us": yard_us, "migrate_over_yardstick": mig_us / yard_us}
        print(json.dumps(case), flush=True)
        res["cases"].append(case)
        del x, y, maps, out, met
        amb.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
