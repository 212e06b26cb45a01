#!/usr/bin/env python3
"""Time per launch of the ordered-statistic detector kernels against the cell-averaging kernels of the same window and
against a plain read of the map's bytes, on one handle in one process.

    python tools/gpu_oscfar_time.py [--launches 100] [--warmup 50] [--out profiles/r16_oscfar_time.json]

  1-D   oscfar1d_kernel against cfar1d_kernel at 513 x 411, window (2, 6), 256 CPIs per call
  2-D   oscfar2d_kernel against blah2hip_cfar2d_dev's AUTO choice at 1025 x 2048, window (2, 6, 1, 3), 16 CPIs per call

Maps of complex Gaussian noise (exponential powers), pfa 1e-3, rank 750 per mille.  A kernel's time is the handle's
BLAH2HIP_K_CFAR (an event pair around the launch), read after every launch; the two detectors alternate, and the figure is
the median of `--launches` launches behind `--warmup` untimed ones.  Beside them the map's bytes through
blah2hip_stream_read_dev, bracketed by an event pair per launch.  The yardsticks are the averaging kernel and that read,
never the new kernels' own earlier runs.  One process; run it under a time limit."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, n_doppler, n_delay, window, CPIs per call)
CASES = [("1d", 513, 411, (2, 6), 256), ("2d", 1025, 2048, (2, 6, 1, 3), 16)]
PFA, CAP = 1e-3, 1 << 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_oscfar_time.json"))
    a = ap.parse_args()
    if a.launches < 50:
        sys.exit("at least 50 launches")
    import torch

    import blah2_amd as b2
    L = b2.load()
    st = torch.cuda.current_stream().cuda_stream
    res = {"launches": a.launches, "warmup": a.warmup, "pfa": PFA, "rank_permille": 750,
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "cases": []}
    for name, nD, nC, w, n_cpi in CASES:
        n = nD * 1024  # pulses of 1024 samples: the handle only gives the shape and the axes
        amb = b2.Ambiguity(-3, nC - 4, -1000, 1000, n, n, False, max_batch=n_cpi, n_doppler_bins=nD)
        assert (amb.get_n_doppler_bins(), amb.get_n_delay_bins()) == (nD, nC)
        torch.manual_seed(16)
        maps = torch.randn((n_cpi, nD, nC, 2), dtype=torch.float32, device="cuda") * 0.7071
        met = torch.zeros((n_cpi, 2), dtype=torch.float64, device="cuda")
        hits = torch.zeros((n_cpi, CAP, 2), dtype=torch.float64, device="cuda")
        cnt = torch.zeros(n_cpi, dtype=torch.int32, device="cuda")
        if len(w) == 2:
            ca, os_ = b2.CfarDetector1D(PFA, *w, -128, 0.0), b2.OsCfarDetector1D(PFA, *w, -128, 0.0)
        else:
            ca, os_ = b2.CfarDetector2D(PFA, *w, -128, 0.0), b2.OsCfarDetector2D(PFA, *w, -128, 0.0)
        us, counts = {"ca": [], "os": []}, {}
        amb.set_timing(True)
        for it in range(a.warmup + a.launches):
            for key, det in (("ca", ca), ("os", os_)):
                amb.get_timing()
                det.process_dev(amb, n_cpi, hits.data_ptr(), CAP, cnt.data_ptr(), maps.data_ptr(), met.data_ptr(), st)
                ms, k = amb.get_timing()["cfar"]  # synchronises
                assert k == 1, k
                if it >= a.warmup:
                    us[key].append(ms * 1e3)
                counts[key] = int(cnt.sum().cpu())
        amb.set_timing(False)
        nbytes = n_cpi * nD * nC * 8
        src = maps.view(-1)
        read = []
        for it in range(a.warmup + a.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            b2._lib.check(L.blah2hip_stream_read_dev(src.data_ptr(), nbytes, None, st))
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                read.append(e0.elapsed_time(e1) * 1e3)
        gw = w if len(w) == 4 else (w[0], w[1], 0, 0)
        n_train = (2 * (gw[0] + gw[1]) + 1) * (2 * (gw[2] + gw[3]) + 1) - (2 * gw[0] + 1) * (2 * gw[2] + 1)
        case = {"case": name, "n_doppler": nD, "n_delay": nC, "window": list(w), "n_cpi": n_cpi, "map_bytes": nbytes,
                "training_cells": n_train,
                "ca_kernel": "cfar1d_kernel" if len(w) == 2 else "blah2hip_cfar2d_dev AUTO",
                "ca_us_median": statistics.median(us["ca"]), "ca_us_min": min(us["ca"]),
                "os_us_median": statistics.median(us["os"]), "os_us_min": min(us["os"]),
                "read_us_median": statistics.median(read), "read_us_min": min(read),
                "ca_hits": counts["ca"], "os_hits": counts["os"]}
        case["os_over_ca"] = case["os_us_median"] / case["ca_us_median"]
        case["os_over_read"] = case["os_us_median"] / case["read_us_median"]
        case["os_us_per_cpi"] = case["os_us_median"] / n_cpi
        case["ca_us_per_cpi"] = case["ca_us_median"] / n_cpi
        case["os_compares_per_ns"] = n_cpi * nD * nC * n_train / case["os_us_median"] / 1e3
        print(json.dumps(case), flush=True)
        res["cases"].append(case)
        del maps, met, hits, cnt, src
        amb.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
