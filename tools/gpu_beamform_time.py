#!/usr/bin/env python3
"""Time per launch of beamform_kernel against what a plain read-plus-write kernel reaches in the same process.

    python tools/gpu_beamform_time.py [--launches 100] [--warmup 50] [--out profiles/r09_beamform_time.json]

configs[1] map size (513 x 411), K = n_beams = 4, at n_cpi = 64 and at n_cpi = 1.  The beam kernel's time is
blah2hip_amb_set_timing's BLAH2HIP_K_BEAM (an event pair around the one launch; its metrics_kernel counts under
BLAH2HIP_K_METRICS), read after every launch: the median of `--launches` launches behind `--warmup` untimed ones.
Its bytes are (K + n_beams) * cells * 8 * n_cpi: every channel map read once, every beam map written once.

The yardstick moves the SAME number of bytes in the same process: blah2hip_deblock_c32_dev (a bit-exact copy kernel:
half the bytes read, half written) and blah2hip_stream_read_dev (all of them read), each bracketed by an event pair
per launch, median of as many launches.  The beam kernel's rate is reported as a fraction of the copy kernel's; it is
never compared with its own earlier runs.  One process; run it under a time limit."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG2 = (-10, 400, -256, 256, 2_000_000, 2_000_000)
K = NB = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_beamform_time.json"))
    a = ap.parse_args()
    if a.launches < 50:
        sys.exit("at least 50 launches")
    import torch

    import blah2_amd as b2
    L = b2.load()
    amb = b2.Ambiguity(*CFG2, True, max_batch=K * 64)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    cells = nD * nC
    st = torch.cuda.current_stream().cuda_stream
    w = b2.ula_weights(K, 0.5, [0.0, 15.0, 30.0, 45.0])
    res = {"geometry": f"configs[1]: {nD} x {nC}", "n_surv": K, "n_beams": NB, "launches": a.launches, "warmup": a.warmup,
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

    for n_cpi in (64, 1):
        maps = torch.randn((K, n_cpi, nD, nC, 2), dtype=torch.float32, device="cuda")
        out = torch.empty((NB, n_cpi, nD, nC, 2), dtype=torch.float32, device="cuda")
        met = torch.empty((NB, n_cpi, 2), dtype=torch.float64, device="cuda")
        nbytes = (K + NB) * cells * 8 * n_cpi

        def beam():
            amb.beamform_dev(maps.data_ptr(), K, n_cpi, w, out.data_ptr(), met.data_ptr(), st)
        for _ in range(a.warmup):
            beam()
        torch.cuda.synchronize()
        amb.set_timing(True)
        amb.get_timing()
        us = []
        for _ in range(a.launches):
            beam()
            ms, n = amb.get_timing()["beam"]  # synchronises
            assert n == 1
            us.append(ms * 1e3)
        amb.set_timing(False)
        beam_us = statistics.median(us)

        # the same bytes through the copy kernel (half read, half written) and through the read kernel
        # complex samples per channel (2 channels x 8 bytes, read and written), whole blocks only: the buffer ends with one
        block = 4096
        n_s = nbytes // 32 // block * block
        raw = torch.randn((2 * n_s, 2), dtype=torch.float32, device="cuda")
        x = torch.empty((n_s, 2), dtype=torch.float32, device="cuda")
        y = torch.empty((n_s, 2), dtype=torch.float32, device="cuda")
        copy_us, copy_min = median_us(lambda: b2.deblock_c32_dev(raw.data_ptr(), block, 0, n_s, 1, x.data_ptr(), y.data_ptr(), n_s, st))
        src = torch.randn((nbytes // 4,), dtype=torch.float32, device="cuda")
        read_us, read_min = median_us(lambda: b2._lib.check(L.blah2hip_stream_read_dev(src.data_ptr(), nbytes, None, st)))
        case = {"n_cpi": n_cpi, "bytes": nbytes, "beam_us_median": beam_us, "beam_us_min": min(us), "beam_gbs": nbytes / beam_us / 1e3,
                "copy_kernel": "blah2hip_deblock_c32_dev", "copy_bytes": 32 * n_s, "copy_us_median": copy_us, "copy_us_min": copy_min,
                "copy_gbs": 32 * n_s / copy_us / 1e3, "read_us_median": read_us, "read_us_min": read_min, "read_gbs": nbytes / read_us / 1e3}
        case["beam_over_copy_rate"] = case["beam_gbs"] / case["copy_gbs"]
        case["beam_over_read_rate"] = case["beam_gbs"] / case["read_gbs"]
        print(json.dumps(case), flush=True)
        res["cases"].append(case)
        del maps, out, met, raw, x, y, src
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
