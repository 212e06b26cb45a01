#!/usr/bin/env python3
"""Time per call of the bearing scan against the snapshot gather on the same detection lists, in the same process.

    python tools/gpu_bearing_time.py [--launches 100] [--warmup 50] [--out profiles/r11_bearing_time.json]

configs[1] map size (513 x 411), K = 4 and 8 channels, steering tables of G = 181 and 360 points, n_cpi = 16 lists of 16 and
of 256 detections on random cells, Bartlett (no covariance) and adaptive (the covariance blah2hip_amb_covariance_dev leaves,
loading 1e-3).  The bearing's time is blah2hip_amb_set_timing's BLAH2HIP_K_BEARING (an event pair around bearing_kernel),
read after every call: the median of `--launches` calls behind `--warmup` untimed ones.

The yardstick is blah2hip_amb_snapshot_dev on the SAME lists -- the gather a host-side bearing needs before anything is
computed -- bracketed by an event pair per call (it has no timing slot), median of as many calls.  The bearing is reported
as a multiple of that gather's time; it is never compared with its own earlier runs.  One process; run it under a time
limit."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG2 = (-10, 400, -256, 256, 2_000_000, 2_000_000)
N_CPI = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_bearing_time.json"))
    a = ap.parse_args()
    if a.launches < 50:
        sys.exit("at least 50 launches")
    import torch

    import blah2_amd as b2
    from blah2_amd import _lib
    amb = b2.Ambiguity(*CFG2, True, max_batch=8 * N_CPI)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    st = torch.cuda.current_stream().cuda_stream
    res = {"geometry": f"configs[1]: {nD} x {nC}", "n_cpi": N_CPI, "loading": 1e-3, "launches": a.launches, "warmup": a.warmup,
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

    def slot_us(enqueue):
        for _ in range(a.warmup):
            enqueue()
        torch.cuda.synchronize()
        amb.set_timing(True)
        amb.get_timing()
        us = []
        for _ in range(a.launches):
            enqueue()
            ms, n = amb.get_timing()["bearing"]  # synchronises
            assert n == 1
            us.append(ms * 1e3)
        amb.set_timing(False)
        return statistics.median(us), min(us)

    rng = np.random.default_rng(11)
    for K in (4, 8):
        maps = torch.randn((K, N_CPI, nD, nC, 2), dtype=torch.float32, device="cuda")
        cov = torch.empty((N_CPI, K, K, 2), dtype=torch.float64, device="cuda")
        amb.covariance_dev(maps.data_ptr(), K, N_CPI, cov.data_ptr(), None, st)
        for n_det in (16, 256):
            dets = np.zeros((N_CPI, n_det), dtype=b2.DET_DTYPE)
            dets["row"], dets["col"] = rng.integers(0, nD, dets.shape), rng.integers(0, nC, dets.shape)
            d_dets = torch.from_numpy(dets.view(np.uint8).reshape(-1)).cuda()
            d_cnt = torch.full((N_CPI,), n_det, dtype=torch.int32, device="cuda")
            snap = torch.empty((N_CPI, n_det, K, 2), dtype=torch.float32, device="cuda")
            out = torch.empty((N_CPI * n_det * b2.BEARING_DTYPE.itemsize,), dtype=torch.uint8, device="cuda")
            snap_us, snap_min = median_us(lambda: amb.snapshot_dev(maps.data_ptr(), K, N_CPI, d_dets.data_ptr(), n_det,
                                                                   d_cnt.data_ptr(), N_CPI, snap.data_ptr(), st))
            for G in (181, 360):
                steer = b2.ula_steering(K, 0.5, np.linspace(-90.0, 90.0, G)).astype(np.complex64)
                d_steer = torch.from_numpy(steer.view(np.float32)).cuda()
                for mode, d_cov in (("bartlett", None), ("adaptive", cov.data_ptr())):
                    us, us_min = slot_us(lambda: amb.bearing_dev(maps.data_ptr(), K, N_CPI, d_dets.data_ptr(), n_det, d_cnt.data_ptr(),
                                                                  N_CPI, d_steer.data_ptr(), G, out.data_ptr(), d_cov, 1e-3, False, st))
                    rec = out.cpu().numpy().view(b2.BEARING_DTYPE)
                    assert (rec["index"] >= 0).all() and (rec["adaptive"] == (d_cov is not None)).all()
                    case = {"n_surv": K, "n_grid": G, "detections_per_list": n_det, "mode": mode,
                            "workgroups_per_list": amb.info(_lib.INFO_BEARING_GRID), "bearing_us_median": us, "bearing_us_min": us_min,
                            "snapshot_kernel": "blah2hip_amb_snapshot_dev", "snapshot_us_median": snap_us, "snapshot_us_min": snap_min,
                            "bearing_over_snapshot_time": us / snap_us}
                    print(json.dumps(case), flush=True)
                    res["cases"].append(case)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
