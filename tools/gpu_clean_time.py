#!/usr/bin/env python3
"""Time per launch of the echo canceller's kernels (clean_gram_kernel, clean_fold_kernel, clean_solve_kernel,
clean_subtract_kernel) against the copy rate measured in the same process and against the fp32 issue floor of their
multiply-adds.

    python tools/gpu_clean_time.py [--launches 20] [--warmup 5] [--out profiles/r23_clean_time.json]

N = 2 * 10^6 samples per CPI, P in {1, 3, 9, 32} atoms, batches of 1 and 64 CPIs, delays in [-10, 100], FMT_C32, noise
planes.  A kernel's time is its slot of blah2hip_clean_get_timing (an event pair around the launch), read after every
call: the median of `--launches` calls behind `--warmup` untimed ones.

ALGORITHMIC bytes: the fit reads x and y once (16 N per CPI), the subtraction reads both and writes y (24 N).  The copy
yardstick moves the same bytes through blah2hip_deblock_c32_dev (a bit-exact copy kernel: half read, half written).
Multiply-adds: the fit forms P (P + 3) / 2 complex products a sample, 4 fused multiply-adds each; the subtraction per atom
and sample two complex products for the replica (8 instructions) and the chain's 4.  The floor is those over the vector
ALU's 78.6 T fused multiply-adds a second (157.3 TFLOP/s fp32).  There is no pass/fail time: the fractions are the result.
One process; run it under a time limit."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, FS, DLO, DHI = 2_000_000, 2_000_000.0, -10, 100
ATOMS = (1, 3, 9, 32)
BATCHES = (1, 64)
FMA_PER_S = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_clean_time.json"))
    a = ap.parse_args()
    if a.launches < 10:
        sys.exit("at least 10 launches")
    import torch

    import blah2_amd as b2
    st = torch.cuda.current_stream().cuda_stream
    res = {"n_samples": N, "delays": [DLO, DHI], "launches": a.launches, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
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
        return statistics.median(us)

    Bmax = max(BATCHES)
    x = torch.randn((Bmax, N, 2), dtype=torch.float32, device="cuda")
    y = torch.randn((Bmax, N, 2), dtype=torch.float32, device="cuda")
    out = torch.empty((Bmax, N, 2), dtype=torch.float32, device="cuda")
    copy_gbs = {}
    for B in BATCHES:  # the copy yardstick at the subtraction's bytes (the fit's are two thirds of them: one more point)
        for name, nbytes in (("fit", 16 * N * B), ("subtract", 24 * N * B)):
            block = 4096
            n_s = nbytes // 32 // block * block
            raw = torch.randn((2 * n_s, 2), dtype=torch.float32, device="cuda")
            cx = torch.empty((n_s, 2), dtype=torch.float32, device="cuda")
            cy = torch.empty((n_s, 2), dtype=torch.float32, device="cuda")
            us = median_us(lambda: b2.deblock_c32_dev(raw.data_ptr(), block, 0, n_s, 1, cx.data_ptr(), cy.data_ptr(), n_s, st))
            copy_gbs[(B, name)] = 32 * n_s / us / 1e3
            del raw, cx, cy
    for B in BATCHES:
        ec = b2.EchoCanceller(N, FS, DLO, DHI, max_batch=B)
        for P in ATOMS:
            at = np.zeros((B, P), dtype=b2.ATOM_DTYPE)
            at["delay"] = (DLO + 3 * np.arange(P))[None, :]
            at["doppler"] = (17.3 * np.arange(P) - 200.0)[None, :]
            d_at = torch.from_numpy(at.view(np.uint8).reshape(-1).copy()).cuda()
            d_cnt = torch.full((B,), P, dtype=torch.int32, device="cuda")
            d_amp = torch.zeros((B, P, 2), dtype=torch.float64, device="cuda")
            d_ok = torch.zeros(B, dtype=torch.int32, device="cuda")
            launch = lambda: ec.process_dev(b2.FMT_C32, x.data_ptr(), y.data_ptr(), B, N, d_at.data_ptr(), P, d_cnt.data_ptr(), 1e-6,  # noqa: E731
                                            d_amp.data_ptr(), d_ok.data_ptr(), out.data_ptr(), N, st)
            for _ in range(a.warmup):
                launch()
            torch.cuda.synchronize()
            ec.set_timing(True)
            ec.get_timing()
            t = {k: [] for k in ("clean_gram", "clean_fold", "clean_solve", "clean_subtract")}
            for _ in range(a.launches):
                launch()
                got = ec.get_timing()  # synchronises
                for k in t:
                    assert got[k][1] == 1
                    t[k].append(got[k][0] * 1e3)
            ec.set_timing(False)
            assert int(d_ok.sum()) == B
            us = {k: statistics.median(v) for k, v in t.items()}
            fit_fma = P * (P + 3) // 2 * 4 * N * B
            sub_fma = 12 * P * N * B
            case = {"n_cpi": B, "atoms": P, "gram_grid": ec.get_info(b2._lib.CLEAN_INFO_GRAM_GRID),
                    "subtract_grid": ec.get_info(b2._lib.CLEAN_INFO_SUBTRACT_GRID), **{k + "_us_median": v for k, v in us.items()},
                    "gram_bytes": 16 * N * B, "gram_gbs": 16 * N * B / us["clean_gram"] / 1e3, "copy_gbs_fit_bytes": copy_gbs[(B, "fit")],
                    "gram_fma": fit_fma, "gram_issue_floor_us": fit_fma / FMA_PER_S * 1e6,
                    "subtract_bytes": 24 * N * B, "subtract_gbs": 24 * N * B / us["clean_subtract"] / 1e3,
                    "copy_gbs_subtract_bytes": copy_gbs[(B, "subtract")], "subtract_fma": sub_fma,
                    "subtract_issue_floor_us": sub_fma / FMA_PER_S * 1e6}
            case["gram_over_copy_rate"] = case["gram_gbs"] / case["copy_gbs_fit_bytes"]
            case["gram_issue_floor_over_time"] = case["gram_issue_floor_us"] / us["clean_gram"]
            case["subtract_over_copy_rate"] = case["subtract_gbs"] / case["copy_gbs_subtract_bytes"]
            case["subtract_issue_floor_over_time"] = case["subtract_issue_floor_us"] / us["clean_subtract"]
            case["gram_bound"] = "vector ALU issue" if case["gram_issue_floor_over_time"] > case["gram_over_copy_rate"] else "memory"
            case["subtract_bound"] = "vector ALU issue" if case["subtract_issue_floor_over_time"] > case["subtract_over_copy_rate"] else "memory"
            print(json.dumps(case), flush=True)
            res["cases"].append(case)
        ec.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
