#!/usr/bin/env python3
"""Time per launch of the greatest-of / smallest-of detector kernels against the cell-averaging and ordered-statistic
kernels of the same window's extent, on one handle in one process.

    python tools/gpu_gocfar_time.py [--launches 100] [--warmup 50] [--out profiles/r27_gocfar_time.json]

  1-D   gocfar1d_kernel (go, so) against cfar1d_kernel and oscfar1d_kernel at 513 x 411, nGuard 2, nTrain 8, 256 CPIs per call
  2-D   gocfar2d_kernel (go, so; hR 4, nGd 2, nTd 6: the 17 x 9 window's extent) against blah2hip_cfar2d_dev's stream and tile
        kernels and oscfar2d_kernel on the window (2, 6, 1, 3) at 1025 x 2048, 16 CPIs per call

Maps of complex Gaussian noise (exponential powers), pfa 1e-3.  A kernel's time is the handle's BLAH2HIP_K_CFAR (an event
pair around the launch), read after every launch; the variants alternate, and the figure is the median of `--launches`
launches behind `--warmup` untimed ones.  The yardsticks are the averaging kernel (1-D) and the ordered-statistic tile kernel
(2-D, the same LDS fill), never the new kernels' own earlier runs.  One process; run it under a time limit."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PFA, CAP = 1e-3, 1 << 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_gocfar_time.json"))
    a = ap.parse_args()
    if a.launches < 50:
        sys.exit("at least 50 launches")
    import torch

    import blah2_amd as b2
    from blah2_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    res = {"launches": a.launches, "warmup": a.warmup, "pfa": PFA, "device": torch.cuda.get_device_name(0),
           "arch": torch.cuda.get_device_properties(0).gcnArchName, "cases": []}
    one = [("ca", lambda: b2.CfarDetector1D(PFA, 2, 8, -128, 0.0), None), ("os", lambda: b2.OsCfarDetector1D(PFA, 2, 8, -128, 0.0), None),
           ("go", lambda: b2.GoCfarDetector1D(PFA, 2, 8, -128, 0.0, kind="go"), None),
           ("so", lambda: b2.GoCfarDetector1D(PFA, 2, 8, -128, 0.0, kind="so"), None)]
    two = [("ca_stream", lambda: b2.CfarDetector2D(PFA, 2, 6, 1, 3, -128, 0.0), _lib.CFAR2D_STREAM),
           ("ca_tile", lambda: b2.CfarDetector2D(PFA, 2, 6, 1, 3, -128, 0.0), _lib.CFAR2D_TILE),
           ("os", lambda: b2.OsCfarDetector2D(PFA, 2, 6, 1, 3, -128, 0.0), None),
           ("go", lambda: b2.GoCfarDetector2D(PFA, 2, 6, 4, -128, 0.0, kind="go"), None),
           ("so", lambda: b2.GoCfarDetector2D(PFA, 2, 6, 4, -128, 0.0, kind="so"), None)]
    for name, nD, nC, n_cpi, variants in (("1d", 513, 411, 256, one), ("2d", 1025, 2048, 16, two)):
        n = nD * 1024  # pulses of 1024 samples: the handle only gives the shape and the axes
        amb = b2.Ambiguity(-3, nC - 4, -1000, 1000, n, n, False, max_batch=n_cpi, n_doppler_bins=nD)
        assert (amb.get_n_doppler_bins(), amb.get_n_delay_bins()) == (nD, nC)
        torch.manual_seed(30)
        maps = torch.randn((n_cpi, nD, nC, 2), dtype=torch.float32, device="cuda") * 0.7071
        met = torch.zeros((n_cpi, 2), dtype=torch.float64, device="cuda")
        hits = torch.zeros((n_cpi, CAP, 2), dtype=torch.float64, device="cuda")
        cnt = torch.zeros(n_cpi, dtype=torch.int32, device="cuda")
        dets = [(key, make(), force) for key, make, force in variants]
        us, counts = {key: [] for key, _, _ in dets}, {}
        amb.set_timing(True)
        for it in range(a.warmup + a.launches):
            for key, det, force in dets:
                amb.set_cfar2d_kernel(force if force is not None else _lib.CFAR2D_AUTO)
                amb.get_timing()
                det.process_dev(amb, n_cpi, hits.data_ptr(), CAP, cnt.data_ptr(), maps.data_ptr(), met.data_ptr(), st)
                ms, k = amb.get_timing()["cfar"]  # synchronises
                assert k == 1, k
                if it >= a.warmup:
                    us[key].append(ms * 1e3)
                counts[key] = int(cnt.sum().cpu())
        amb.set_timing(False)
        case = {"case": name, "n_doppler": nD, "n_delay": nC, "n_cpi": n_cpi, "map_bytes": n_cpi * nD * nC * 8, "hits": counts}
        for key in us:
            case[key + "_us_median"], case[key + "_us_min"] = statistics.median(us[key]), min(us[key])
        yard = "ca" if name == "1d" else "os"
        for key in ("go", "so"):
            case[f"{key}_over_{yard}"] = case[key + "_us_median"] / case[yard + "_us_median"]
            case[key + "_us_per_cpi"] = case[key + "_us_median"] / n_cpi
        print(json.dumps(case), flush=True)
        res["cases"].append(case)
        del maps, met, hits, cnt
        amb.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
