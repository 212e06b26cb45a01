#!/usr/bin/env python3
"""Time per launch of nci_kernel against what a plain read-plus-write kernel reaches in the same process.

    python tools/gpu_nci_time.py [--launches 100] [--warmup 50] [--out profiles/r15_nci_time.json]

configs[1] map size (513 x 411); (n_surv, window, hop, n_cpi) = (4, 1, 1, 6): the channels of six CPIs summed, (1, 4, 1,
24): a sliding window over one channel, and (4, 4, 4, 6): both, a window every fourth CPI.  The kernel's time is
blah2hip_nci_set_timing's BLAH2HIP_NK_NCI (an event pair around the one launch; its metrics_kernel counts under the
ambiguity handle's BLAH2HIP_K_METRICS), read after every launch: the median of `--launches` launches behind `--warmup`
untimed ones, which also fill the history.  Its ALGORITHMIC bytes per launch: every input map read once (n_surv * n_cpi * cells * 8), every
output map written once (n_out * cells * 8; with a hop that does not divide n_cpi n_out differs from launch to launch, so
the rate is taken launch by launch) and the history planes read and written once each (2 * (window - 1) * cells * 4).

The yardstick moves the mean number of those bytes in the same process: blah2hip_deblock_c32_dev (a bit-exact copy
kernel: half the bytes read, half written) and blah2hip_stream_read_dev (all of them read), each bracketed by an event
pair per launch, median of as many launches.  The kernel's rate is reported as a fraction of the copy kernel's; it is
never compared with its own earlier runs.  One process; run it under a time limit."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG2 = (-10, 400, -256, 256, 2_000_000, 2_000_000)
CASES = [(4, 1, 1, 6), (1, 4, 1, 24), (4, 4, 4, 6)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_nci_time.json"))
    a = ap.parse_args()
    if a.launches < 50:
        sys.exit("at least 50 launches")
    import torch

    import blah2_amd as b2
    L = b2.load()
    amb = b2.Ambiguity(*CFG2, True, max_batch=24)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    cells = nD * nC
    st = torch.cuda.current_stream().cuda_stream
    res = {"geometry": f"configs[1]: {nD} x {nC}", "launches": a.launches, "warmup": a.warmup,
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

    for K, W, H, n_cpi in CASES:
        maps = torch.randn((K, n_cpi, nD, nC, 2), dtype=torch.float32, device="cuda")
        out = torch.empty((n_cpi, nD, nC, 2), dtype=torch.float32, device="cuda")
        met = torch.empty((n_cpi, 2), dtype=torch.float64, device="cuda")
        integ = b2.MapIntegrator(amb, K, W, H)

        def launch():
            return integ.process_dev(maps.data_ptr(), n_cpi, out.data_ptr(), met.data_ptr(), n_cpi, None, st)[0]
        for _ in range(a.warmup):
            launch()
        torch.cuda.synchronize()
        integ.set_timing(True)
        integ.get_timing()
        us, nbytes = [], []
        for _ in range(a.launches):
            n_out = launch()
            ms, n = integ.get_timing()["nci"]  # synchronises
            assert n == 1
            us.append(ms * 1e3)
            nbytes.append((K * n_cpi + n_out) * cells * 8 + 2 * (W - 1) * cells * 4)
        integ.close()
        nci_us = statistics.median(us)
        nci_gbs = statistics.median(b / u / 1e3 for b, u in zip(nbytes, us))
        mean_bytes = int(statistics.mean(nbytes))

        # the same bytes through the copy kernel (half read, half written) and through the read kernel
        # complex samples per channel (2 channels x 8 bytes, read and written), whole blocks only: the buffer ends with one
        block = 4096
        n_s = mean_bytes // 32 // block * block
        raw = torch.randn((2 * n_s, 2), dtype=torch.float32, device="cuda")
        x = torch.empty((n_s, 2), dtype=torch.float32, device="cuda")
        y = torch.empty((n_s, 2), dtype=torch.float32, device="cuda")
        copy_us, copy_min = median_us(lambda: b2.deblock_c32_dev(raw.data_ptr(), block, 0, n_s, 1, x.data_ptr(), y.data_ptr(), n_s, st))
        read_bytes = mean_bytes // 16 * 16
        src = torch.randn((read_bytes // 4,), dtype=torch.float32, device="cuda")
        read_us, read_min = median_us(lambda: b2._lib.check(L.blah2hip_stream_read_dev(src.data_ptr(), read_bytes, None, st)))
        case = {"n_surv": K, "window": W, "hop": H, "n_cpi": n_cpi, "bytes_mean": mean_bytes, "bytes_min": min(nbytes),
                "bytes_max": max(nbytes), "nci_us_median": nci_us, "nci_us_min": min(us), "nci_gbs": nci_gbs,
                "copy_kernel": "blah2hip_deblock_c32_dev", "copy_bytes": 32 * n_s, "copy_us_median": copy_us, "copy_us_min": copy_min,
                "copy_gbs": 32 * n_s / copy_us / 1e3, "read_us_median": read_us, "read_us_min": read_min,
                "read_gbs": read_bytes / read_us / 1e3}
        case["nci_over_copy_rate"] = case["nci_gbs"] / case["copy_gbs"]
        case["nci_over_read_rate"] = case["nci_gbs"] / case["read_gbs"]
        print(json.dumps(case), flush=True)
        res["cases"].append(case)
        del maps, out, met, raw, x, y, src
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
