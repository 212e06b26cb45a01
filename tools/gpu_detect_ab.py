#!/usr/bin/env python3
"""Replay with the reference's default detector chain (nCentroid: 6): Centroid and Interpolate on the host against
the device kernel (GpuChain(detect="host") / detect="device"), interleaved pairs on one box.

    python tools/gpu_detect_ab.py [--configs cfg2,cfg3] [--pairs 3] [--batch 8] [--out profiles/r08_detect_ab.json]

Per geometry: a synthetic capture in /dev/shm (tools/replay_bench.py's), the pinned host-to-device rate measured beside
it, then `pairs` times (host, device), each leg a fresh chain, an untimed stretch and passes over the capture until
--min-seconds.  Reports CPIs/s, the fraction of the pinned-copy rate, the host CPU seconds per CPI and the detections per
CPI of either leg, and per pair device / host.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

import bench
from blah2_amd import replay as R
from replay_bench import h2d_rate, make_capture


def leg(cfg, path, n, batch, detect, min_seconds, warm_cpis):
    chain = R.GpuChain(cfg, 0, batch, detect=detect)
    cap = R.RspduoFile(path, n)
    R.replay(cap, chain, batch, limit=warm_cpis, emit=lambda r: None)
    chain.release_all()
    cap.close()
    done = dets = 0
    cpu0, t0 = time.process_time(), time.perf_counter()
    while not done or time.perf_counter() - t0 < min_seconds:
        cap = R.RspduoFile(path, n)
        cnt = [0, 0]

        def emit(r):
            cnt[0] += 1
            cnt[1] += len(r.get("delay", ()))

        R.replay(cap, chain, batch, emit=emit)
        chain.release_all()
        cap.close()
        done, dets = done + cnt[0], dets + cnt[1]
    el, cpu = time.perf_counter() - t0, time.process_time() - cpu0
    busy = chain.busy_ms / max(chain.batches_done, 1)
    chain.close()
    return {"detect": detect, "cpis_per_s": done / el, "host_cpu_s_per_cpi": cpu / done, "detections_per_cpi": dets / done,
            "cpis_timed": done, "seconds": el, "gpu_busy_ms_per_batch": busy}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--cpis", type=int, default=512, help="CPIs in the capture (cut down to what /dev/shm holds)")
    ap.add_argument("--min-seconds", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_detect_ab.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    numa = R.pin_to_device_node(torch, 0)
    out = {"pairs": a.pairs, "batch": a.batch, "pinned_to_gpu_numa_node": numa, "geometries": []}
    for name in a.configs.split(","):
        (dmin, dmax, fmin, fmax, fs, n), desc = bench.CONFIGS[name]
        bytes_per_cpi = n * R.BYTES_PER_SAMPLE
        st = os.statvfs("/dev/shm")
        fit = int(st.f_bavail * st.f_frsize * 0.5 / bytes_per_cpi) // a.batch * a.batch
        cpis = max(2 * a.batch, min(a.cpis, fit))
        path = f"/dev/shm/blah2_detect_ab_{name}.rspduo"
        make_capture(path, n, cpis, fs)
        try:
            rate = h2d_rate(dev)
            bound = rate / bytes_per_cpi
            cfg = {"fs": fs, "n_samples": n,
                   "ambiguity": {"delayMin": dmin, "delayMax": dmax, "dopplerMin": fmin, "dopplerMax": fmax},
                   "clutter": {"enable": False},
                   "detection": {"enable": True, "pfa": 1e-5, "nGuard": 2, "nTrain": 6, "minDelay": 5, "minDoppler": 15.0,
                                 "nCentroid": 6}}
            geo = {"config": name, "workload": desc, "cpis": cpis, "bytes_per_cpi": bytes_per_cpi, "pinned_h2d_GBps": rate / 1e9,
                   "pcie_bound_cpis_per_s": bound, "pairs": []}
            for k in range(a.pairs):
                pair = {}
                for detect in ("host", "device"):
                    r = leg(cfg, path, n, a.batch, detect, a.min_seconds, min(cpis, 4 * a.batch))
                    r["frac_of_pcie_bound"] = r["cpis_per_s"] / bound
                    pair[detect] = r
                pair["device_over_host"] = pair["device"]["cpis_per_s"] / pair["host"]["cpis_per_s"]
                print(json.dumps({"config": name, "pair": k, **pair}), flush=True)
                geo["pairs"].append(pair)
            out["geometries"].append(geo)
        finally:
            os.remove(path)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
