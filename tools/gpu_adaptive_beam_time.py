#!/usr/bin/env python3
"""Time per call of the array covariance, and of the whole adaptive-beam sequence, against a plain read of the same bytes
in the same process.

    python tools/gpu_adaptive_beam_time.py [--launches 100] [--warmup 50] [--out profiles/r10_adaptive_beam_time.json]

configs[1] map size (513 x 411), K = n_beams = 4 and K = n_beams = 8, at n_cpi = 16 and at n_cpi = 1; the covariance is
taken over the whole map.  The covariance's time is blah2hip_amb_set_timing's BLAH2HIP_K_COV (an event pair around
array_cov_kernel + cov_fold_kernel), read after every call: the median of `--launches` calls behind `--warmup` untimed
ones.  Its bytes are K * cells * 8 * n_cpi: every channel map read once.  The sequence covariance -> weights -> beams
(Ambiguity.adaptive_beamform_dev) is bracketed by an event pair per call; its bytes are (2 K + n_beams) * cells * 8 * n_cpi,
the channel maps read twice and the beam maps written once.

The yardstick is blah2hip_stream_read_dev over the SAME number of bytes as the covariance reads, in the same process,
bracketed by an event pair per launch, median of as many launches.  The covariance's rate is reported as a fraction of that
read rate; it is never compared with its own earlier runs.  One process; run it under a time limit."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG2 = (-10, 400, -256, 256, 2_000_000, 2_000_000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_adaptive_beam_time.json"))
    a = ap.parse_args()
    if a.launches < 50:
        sys.exit("at least 50 launches")
    import torch

    import blah2_amd as b2
    L = b2.load()
    amb = b2.Ambiguity(*CFG2, True, max_batch=8 * 16)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    cells = nD * nC
    st = torch.cuda.current_stream().cuda_stream
    res = {"geometry": f"configs[1]: {nD} x {nC}", "region": "the whole map", "loading": 1e-3, "launches": a.launches,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "cases": []}

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

    for K in (4, 8):
        NB = K
        steer = b2.ula_steering(K, 0.5, [-60.0 + 120.0 * b / (NB - 1) for b in range(NB)])
        for n_cpi in (16, 1):
            maps = torch.randn((K, n_cpi, nD, nC, 2), dtype=torch.float32, device="cuda")
            cov = torch.empty((n_cpi, K, K, 2), dtype=torch.float64, device="cuda")
            w = torch.empty((n_cpi, NB, K, 2), dtype=torch.float32, device="cuda")
            ok = torch.empty((n_cpi,), dtype=torch.int32, device="cuda")
            out = torch.empty((NB, n_cpi, nD, nC, 2), dtype=torch.float32, device="cuda")
            met = torch.empty((NB, n_cpi, 2), dtype=torch.float64, device="cuda")
            cov_bytes = K * cells * 8 * n_cpi
            seq_bytes = (2 * K + NB) * cells * 8 * n_cpi

            def covariance():
                amb.covariance_dev(maps.data_ptr(), K, n_cpi, cov.data_ptr(), None, st)

            def sequence():
                amb.adaptive_beamform_dev(maps.data_ptr(), K, n_cpi, steer, 1e-3, cov.data_ptr(), w.data_ptr(), ok.data_ptr(),
                                          out.data_ptr(), met.data_ptr(), None, st)
            for _ in range(a.warmup):
                covariance()
            torch.cuda.synchronize()
            amb.set_timing(True)
            amb.get_timing()
            us = []
            for _ in range(a.launches):
                covariance()
                ms, n = amb.get_timing()["cov"]  # synchronises
                assert n == 1
                us.append(ms * 1e3)
            amb.set_timing(False)
            cov_us = statistics.median(us)
            seq_us, seq_min = median_us(sequence)
            assert bool((ok == 1).all())

            src = torch.randn((cov_bytes // 4,), dtype=torch.float32, device="cuda")
            read_us, read_min = median_us(lambda: b2._lib.check(L.blah2hip_stream_read_dev(src.data_ptr(), cov_bytes, None, st)))
            case = {"n_surv": K, "n_beams": NB, "n_cpi": n_cpi, "cov_bytes": cov_bytes, "cov_us_median": cov_us, "cov_us_min": min(us),
                    "cov_gbs": cov_bytes / cov_us / 1e3, "read_kernel": "blah2hip_stream_read_dev", "read_us_median": read_us,
                    "read_us_min": read_min, "read_gbs": cov_bytes / read_us / 1e3, "sequence_bytes": seq_bytes,
                    "sequence_us_median": seq_us, "sequence_us_min": seq_min, "sequence_gbs": seq_bytes / seq_us / 1e3}
            case["cov_over_read_rate"] = case["cov_gbs"] / case["read_gbs"]
            print(json.dumps(case), flush=True)
            res["cases"].append(case)
            del maps, cov, w, ok, out, met, src
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
