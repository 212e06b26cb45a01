#!/usr/bin/env python3
"""Clutter filter for several surveillance channels: the shared-reference call against K per-channel calls.

    python tools/gpu_multi_clutter_ab.py [--pairs 3] [--steps 200] [--warmup 20] [--out profiles/r09_multi_clutter_ab.json]

configs[1] filter (410 taps, 2 MS/s, 1 s CPIs: the windowed correlation on F = 2048), FMT_C32 and FMT_I8, K = 2 and K = 4 with
K x n_cpi = 256, and a lone CPI per channel (n_cpi = 1).  Two paths on one box in one process, interleaved (per-channel,
multi, per-channel, multi, ...), each on a handle of its own:
  multi        blah2hip_clutter_process_multi_dev_fmt: r and the reference's spectra once per pass, one recursion per CPI with
               K right-hand sides (always the one-workgroup kernel), the FIR per channel;
  per_channel  the path in front of it: K blah2hip_clutter_process_dev_fmt calls with the handle's default solve form
               (the look-ahead solve where its planner picks it).
Per step the four BLAH2HIP_CK_* slots (blah2hip_clutter_set_timing) and their sum.  A leg is `--warmup` untimed and `--steps`
timed steps; before the first pair both paths run untimed for `--prewarm` steps each.

Every case is one child process under its own `timeout -k 10`; the parent never opens the GPU, stops at the first non-zero
status and retries nothing.

A case is a WIN only if every pair's multi / per-channel ratio (of the summed slots) is below 1 minus the run's same-mode
spread, the larger of the two paths' (max - min) / median over the pairs.  Beside it stands the operation-count prediction:
correlation transforms per segment (2 + K) / 3K with every channel in one pass, and as built -- r with the first channel, the
others in pairs -- (3 + (K - 1) + ceil((K - 1) / 2)) / 3K; one recursion instead of K."""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DMIN, DMAX, N = -10, 400, 2_000_000
CASES = [("FMT_C32", 2, 128), ("FMT_C32", 4, 64), ("FMT_I8", 2, 128), ("FMT_I8", 4, 64),
         ("FMT_C32", 2, 1), ("FMT_C32", 4, 1), ("FMT_I8", 2, 1), ("FMT_I8", 4, 1)]
SLOTS = ("clutter_corr", "clutter_reduce", "clutter_solve", "clutter_fir")


def child(fmt_name, K, B, pairs, steps, warmup, prewarm):
    import torch

    import blah2_amd as b2
    fmt = getattr(b2, fmt_name)
    torch.manual_seed(K * 7 + B)

    def plane(ref=None, gain=0.8):
        if fmt == b2.FMT_I8:
            t = 30.0 * torch.randn((B, N, 2), dtype=torch.float32, device="cuda")
            if ref is not None:
                t = t * 0.1 + gain * ref.float()
            return t.round().clamp(-128, 127).to(torch.int8)
        t = 30.0 * torch.randn((B, N, 2), dtype=torch.float32, device="cuda")
        return t if ref is None else t * 0.1 + gain * ref

    x = plane()
    ys = [plane(x, 0.8 - 0.15 * k) for k in range(K)]
    outs = [torch.empty((B, N), dtype=torch.complex64, device="cuda") for _ in range(K)]
    ok = torch.zeros((K, B), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    pys, pouts = [y.data_ptr() for y in ys], [o.data_ptr() for o in outs]
    whm = b2.WienerHopf(DMIN, DMAX, N, max_batch=B)
    whs = b2.WienerHopf(DMIN, DMAX, N, max_batch=B)

    def step(mode):
        if mode == "multi":
            whm.process_multi_dev(fmt, x.data_ptr(), pys, B, N, pouts, N, ok.data_ptr(), st)
        else:
            for k in range(K):
                whs.process_dev_fmt(fmt, x.data_ptr(), pys[k], B, N, pouts[k], N, ok[k].data_ptr(), st)

    def leg(mode):
        wh = whm if mode == "multi" else whs
        for _ in range(warmup):
            step(mode)
        torch.cuda.synchronize()
        wh.set_timing(True)
        wh.get_timing()
        for _ in range(steps):
            step(mode)
        torch.cuda.synchronize()
        t = wh.get_timing()
        wh.set_timing(False)
        assert bool(ok.all()), mode
        r = {s + "_ms_per_step": t[s][0] / steps for s in SLOTS}
        r["launch_brackets_per_step"] = {s: t[s][1] / steps for s in SLOTS}
        r["total_ms_per_step"] = sum(t[s][0] for s in SLOTS) / steps
        r["solve"] = wh.solve_info()
        return r

    for mode in ("per_channel", "multi"):  # a fresh process: code objects, buffers, the clocks
        for _ in range(prewarm):
            step(mode)
        torch.cuda.synchronize()
    res = {"format": fmt_name, "n_surv": K, "n_cpi": B, "virtual_cpis": K * B, "taps": whm.nBins, "fft_len": whm.fft_len, "pairs": []}
    for p in range(pairs):
        pc, mu = leg("per_channel"), leg("multi")
        res["pairs"].append({"per_channel": pc, "multi": mu, "multi_over_per_channel": mu["total_ms_per_step"] / pc["total_ms_per_step"],
                             "by_slot": {s: mu[s + "_ms_per_step"] / pc[s + "_ms_per_step"] for s in SLOTS}})
    res["device"] = torch.cuda.get_device_name(0)
    res["arch"] = torch.cuda.get_device_properties(0).gcnArchName
    print("RESULT " + json.dumps(res), flush=True)


def verdict(case):
    def spread(mode):
        v = [p[mode]["total_ms_per_step"] for p in case["pairs"]]
        return (max(v) - min(v)) / statistics.median(v)
    case["same_mode_spread"] = {m: spread(m) for m in ("per_channel", "multi")}
    s = max(case["same_mode_spread"].values())
    ratios = [p["multi_over_per_channel"] for p in case["pairs"]]
    case["ratio_median"] = statistics.median(ratios)
    case["ratio_median_by_slot"] = {k: statistics.median(p["by_slot"][k] for p in case["pairs"]) for k in SLOTS}
    K = case["n_surv"]
    case["predicted_corr_ratio_transform_count"] = (2 + K) / (3 * K)
    case["predicted_corr_ratio_as_built"] = (3 + (K - 1) + K // 2) / (3 * K)  # ceil((K - 1) / 2) = K // 2
    case["predicted_recursions"] = f"1 instead of {K}"
    if all(r < 1.0 - s for r in ratios):
        case["verdict"] = "win"
    elif all(r > 1.0 + s for r in ratios):
        case["verdict"] = "loss"
    else:
        case["verdict"] = "tie"
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--prewarm", type=int, default=40)
    ap.add_argument("--lone-steps", type=int, default=200, help="steps per leg of the n_cpi = 1 cases")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds a case's process may take")
    ap.add_argument("--cases", default="", help="comma-separated indices into CASES (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_multi_clutter_ab.json"))
    ap.add_argument("--child", nargs=3, metavar=("FMT", "K", "B"))
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), int(a.child[2]), a.pairs, a.steps, a.warmup, a.prewarm)
    if a.pairs < 3:
        sys.exit("at least three pairs")
    out = {"geometry": "configs[1] filter: 410 taps (-10 ... 400), 2 MS/s, CPIs of 2 000 000 samples",
           "timer": "blah2hip_clutter_set_timing, the four BLAH2HIP_CK_* slots and their sum, ms per step of K x n_cpi filtered CPIs",
           "paths": {"multi": "blah2hip_clutter_process_multi_dev_fmt", "per_channel": "K x blah2hip_clutter_process_dev_fmt, default solve form"},
           "pairs": a.pairs, "steps_per_leg": a.steps, "warmup_per_leg": a.warmup, "prewarm_per_mode": a.prewarm, "host": socket.gethostname(), "cases": [],
           "win_rule": "every pair's multi / per-channel ratio below 1 - the larger same-mode spread ((max - min) / median over the pairs)"}
    if os.path.exists(a.out) and a.cases:  # a run in several visits: keep what the earlier ones measured
        out = json.load(open(a.out))
    pick = [int(i) for i in a.cases.split(",")] if a.cases else range(len(CASES))
    for i in pick:
        fmt, K, B = CASES[i]
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", fmt, str(K), str(B),
               "--pairs", str(a.pairs), "--steps", str(a.steps if B > 1 else a.lone_steps), "--warmup", str(a.warmup), "--prewarm", str(a.prewarm)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:  # a fault, an abort, a time limit: nothing more is started on the GPU
            sys.exit(f"{fmt} K={K} n_cpi={B}: exit status {r.returncode}; stopping")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        case = verdict(json.loads(line[7:]))
        out["device"], out["arch"] = case.pop("device"), case.pop("arch")
        print(json.dumps({k: case[k] for k in ("format", "n_surv", "n_cpi", "ratio_median", "ratio_median_by_slot", "same_mode_spread", "verdict")}), flush=True)
        out["cases"].append(case)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)  # after every case: a later stop keeps what was measured


if __name__ == "__main__":
    main()
