#!/usr/bin/env python3
"""Several surveillance channels per reference: the shared-reference range kernel against the per-channel path.

    python tools/gpu_multi_surv_ab.py [--pairs 3] [--steps 200] [--warmup 20] [--out profiles/r08_multi_surv_ab.json]
                                      [--kernel-resources FILE]
    python tools/gpu_multi_surv_ab.py --dump-resources FILE      # no GPU: the kernels' registers / LDS / occupancy

configs[1] geometry (2 MS/s, 1 s, 513 x 411), 256 virtual CPIs per step (K = 2 x 128, K = 4 x 64), FMT_C32 and FMT_I8.
The range stage's time is blah2hip_amb_set_timing's BLAH2HIP_K_RANGE; the two modes are forced with
BLAH2HIP_OPT_MULTI_SURV_RANGE on ONE handle and run interleaved (per-channel, shared, per-channel, shared, ...).  The
per-channel mode runs rangew1k_kernel, untouched: the yardstick.  A leg is `--warmup` untimed and `--steps` timed steps
(200 x 2.3 ms: half a second; legs of 6 steps measured the clock ramp of a fresh process, its first leg 12 % slow), and
before the first pair both modes run untimed for `--prewarm` steps each.

Every (format, K) case is one child process under its own `timeout -k 10`; the parent never opens the GPU, stops at the
first non-zero status and retries nothing.

A case is a WIN only if every pair favours the shared kernel by more than the run's same-mode spread, the larger of the
two modes' (max - min) / median over the pairs.  Beside the measured ratio stands the transform-count prediction: per
segment 1 + K forward transforms instead of 2K (0.75 at K = 2, 0.625 at K = 4), and what the kernel as built -- pairs
of channels, so 3 transforms per pair instead of 4 -- can reach at most (0.75 at any even K)."""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG2 = (-10, 400, -256, 256, 2_000_000, 2_000_000)
CASES = [("FMT_C32", 2, 128), ("FMT_C32", 4, 64), ("FMT_I8", 2, 128), ("FMT_I8", 4, 64)]


def child(fmt_name, K, B, pairs, steps, warmup, prewarm):
    import torch

    import blah2_amd as b2
    from blah2_amd import _lib
    fmt = getattr(b2, fmt_name)
    n = CFG2[5]
    torch.manual_seed(K * 7 + B)

    def plane(ref=None):
        if fmt == b2.FMT_I8:
            return torch.randint(-128, 128, (B, n, 2), dtype=torch.int8, device="cuda")
        t = 30.0 * torch.randn((B, n, 2), dtype=torch.float32, device="cuda")
        return t if ref is None else t * 0.1 + 0.8 * ref

    x = plane()
    ys = [plane(x) for _ in range(K)]
    amb = b2.Ambiguity(*CFG2, True, max_batch=K * B)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    out = torch.empty((K * B, nD, nC), dtype=torch.complex64, device="cuda")
    met = torch.empty((K * B, 2), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    pys = [y.data_ptr() for y in ys]

    def leg(mode):
        amb.set_multi_surv_range(mode)
        for _ in range(warmup):
            amb.process_multi_dev(fmt, x.data_ptr(), pys, B, n, out.data_ptr(), met.data_ptr(), st)
        torch.cuda.synchronize()
        amb.set_timing(True)
        amb.get_timing()
        for _ in range(steps):
            amb.process_multi_dev(fmt, x.data_ptr(), pys, B, n, out.data_ptr(), met.data_ptr(), st)
        torch.cuda.synchronize()
        t = amb.get_timing()
        amb.set_timing(False)
        return {"range_ms_per_step": t["range"][0] / steps, "range_launches_per_step": t["range"][1] / steps,
                "doppler_ms_per_step": t["doppler"][0] / steps, "range_kernel": amb.info(_lib.INFO_LAST_RANGE_KERNEL),
                "doppler_kernel": amb.last_doppler_kernel()}

    for mode in ("per_channel", "shared"):  # a fresh process: code objects, the leak calibration, the clocks
        amb.set_multi_surv_range(mode)
        for _ in range(prewarm):
            amb.process_multi_dev(fmt, x.data_ptr(), pys, B, n, out.data_ptr(), met.data_ptr(), st)
        torch.cuda.synchronize()
    res = {"format": fmt_name, "n_surv": K, "n_cpi": B, "virtual_cpis": K * B, "fft_len": amb.dims.fft_len,
           "n_seg": amb.dims.n_seg, "seg_len": amb.dims.seg_len, "pairs": []}
    for p in range(pairs):
        pc, sh = leg("per_channel"), leg("shared")
        assert pc["range_kernel"] == _lib.RANGE_WAVE1K and sh["range_kernel"] == _lib.RANGE_SHARED, (pc, sh)
        res["pairs"].append({"per_channel": pc, "shared": sh, "shared_over_per_channel": sh["range_ms_per_step"] / pc["range_ms_per_step"]})
    res["device"] = torch.cuda.get_device_name(0)
    res["arch"] = torch.cuda.get_device_properties(0).gcnArchName
    print("RESULT " + json.dumps(res), flush=True)


def verdict(case):
    def spread(mode):
        v = [p[mode]["range_ms_per_step"] for p in case["pairs"]]
        return (max(v) - min(v)) / statistics.median(v)
    case["same_mode_spread"] = {m: spread(m) for m in ("per_channel", "shared")}
    s = max(case["same_mode_spread"].values())
    ratios = [p["shared_over_per_channel"] for p in case["pairs"]]
    case["ratio_median"] = statistics.median(ratios)
    K = case["n_surv"]
    case["predicted_ratio_transform_count"] = (1 + K) / (2 * K)
    case["predicted_ratio_pairs_as_built"] = (3 * (K // 2) + 2 * (K % 2)) / (2 * K)
    if all(r < 1.0 - s for r in ratios):
        case["verdict"] = "win"
    elif all(r > 1.0 + s for r in ratios):
        case["verdict"] = "loss"
    else:
        case["verdict"] = "tie"
    return case


def dump_resources(path):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), os.path.join(ROOT, "blah2_amd", "csrc", "capi.hip"), "rangew1k"]
    lines = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout.splitlines()
    keep = [ln.strip() for ln in lines if ("rangew1k_shared_kernel" in ln or "rangew1k_kernel" in ln) and ("InC32" in ln or "InI8," in ln)]
    json.dump({"tool": "tools/kernel_resources.py blah2_amd/csrc/capi.hip rangew1k",
               "lds_bytes_per_workgroup": {"rangew1k_kernel (12 waves)": 7680 + 12 * 8704, "rangew1k_shared_kernel (8 waves)": 7680 + 8 * 8704},
               "kernels": keep}, open(path, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--prewarm", type=int, default=150)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a case's process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_multi_surv_ab.json"))
    ap.add_argument("--kernel-resources", help="JSON written by --dump-resources (a cross-compile, no GPU)")
    ap.add_argument("--dump-resources")
    ap.add_argument("--child", nargs=3, metavar=("FMT", "K", "B"))
    a = ap.parse_args()
    if a.dump_resources:
        return dump_resources(a.dump_resources)
    if a.child:
        return child(a.child[0], int(a.child[1]), int(a.child[2]), a.pairs, a.steps, a.warmup, a.prewarm)
    if a.pairs < 3:
        sys.exit("at least three pairs")
    out = {"geometry": "configs[1]: 2 MS/s, 1 s, 513 x 411", "timer": "blah2hip_amb_set_timing, BLAH2HIP_K_RANGE, ms per step of 256 virtual CPIs",
           "pairs": a.pairs, "steps_per_leg": a.steps, "warmup_per_leg": a.warmup, "prewarm_per_mode": a.prewarm, "host": socket.gethostname(), "cases": [],
           "win_rule": "every pair's shared / per-channel ratio below 1 - the larger same-mode spread ((max - min) / median over the pairs)"}
    if a.kernel_resources:
        out["kernel_resources"] = json.load(open(a.kernel_resources))
    for fmt, K, B in CASES:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", fmt, str(K), str(B),
               "--pairs", str(a.pairs), "--steps", str(a.steps), "--warmup", str(a.warmup), "--prewarm", str(a.prewarm)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:  # a fault, an abort, a time limit: nothing more is started on the GPU
            sys.exit(f"{fmt} K={K}: exit status {r.returncode}; stopping")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        case = verdict(json.loads(line[7:]))
        out["device"], out["arch"] = case.pop("device"), case.pop("arch")
        print(json.dumps({k: case[k] for k in ("format", "n_surv", "ratio_median", "same_mode_spread", "verdict")}), flush=True)
        out["cases"].append(case)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)  # after every case: a later stop keeps what was measured


if __name__ == "__main__":
    main()
