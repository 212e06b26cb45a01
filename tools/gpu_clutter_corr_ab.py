#!/usr/bin/env python3
"""Clutter correlations: the tree's library (B) against the parent commit's (A), bit for bit and on the BLAH2HIP_CK_CORR slot.

    git worktree add ../parent HEAD~1 && (cd ../parent && bash tools/build_variant.sh parent) \\
        && mkdir -p tools/ab && cp ../parent/tools/ab/libblah2hip_parent.so tools/ab/
    python tools/gpu_clutter_corr_ab.py --bits
    python tools/gpu_clutter_corr_ab.py --speed [--out profiles/r16_clutter_corr_unify.json]

Written for the change that made the per-channel correlation kernels and the first pass of the shared-reference call one
kernel pair (clutter_corr_kernel / clutter_corr_half_kernel <R3, In, WITH_R, NB>): nothing a caller can read may change.

Library A is selected with BLAH2HIP_LIBRARY (blah2_amd/_lib.py), B is the product library.  Every case and library is one
child process under its own `timeout -k 10`; the parent never opens the GPU, stops at the first non-zero status and retries
nothing.  `--lib-b FILE` takes B from a file as well: with a copy of A's file it is the control of what the speed rule
resolves, one code object against itself (profiles/r16_clutter_corr_control.json).

--bits   per case the child fills the inputs from a fixed seed (integer-valued samples, so that FMT_C32, FMT_I16 and FMT_I8
         carry the same numbers), runs process (and estimate where the case says so) and prints SHA-256 digests of the ok
         flags with the slots around them, of r, b and the taps (read_last) and of the output planes with their gaps.  The
         plan every handle reports must be the one the case names.  A's and B's lines must be equal.
--speed  N = 2 000 000, 32 CPIs per call, FMT_C32 / FMT_I8 / FMT_I16 one after the other in a child, 20 untimed and 200
         timed process_dev_fmt steps each, three interleaved A / B pairs of children per case.  B is as fast as A in a case
         if every pair's B / A ratio is at most 1 + the same-library spread, the larger of A's and B's (max - min) / median
         over the three legs (DESIGN.md section 7 item 6's rule)."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_BITS, B_BITS, GAP = 20011, 3, 5
FMTS = ("FMT_C32", "FMT_I16", "FMT_I8")
FILL = 7777.0

# name -> (kind, ((first lag, last lag), ...), forced F (0: planner), forced form (None: planner), the plan the handle must report)
BIT_CASES = {}
for _F in (1024, 2048, 4096):
    for _form in ("window", "half"):
        BIT_CASES[f"f{_F}_{_form}"] = ("single", ((-10, 100), (0, 60)), _F, _form, (_F, _form))
BIT_CASES["positive_first_lag"] = ("single", ((700, 1000),), 0, None, (2048, "window"))  # first and last windows: the element path
BIT_CASES["lone_cpi_stride_0"] = ("lone", ((-10, 100),), 0, None, (2048, "window"))
BIT_CASES["multi_k3_window"] = ("multi", ((-10, 100),), 0, None, (2048, "window"))
BIT_CASES["multi_k3_half"] = ("multi", ((-10, 100),), 1024, "half", (1024, "half"))
BIT_CASES["blocks_4_groups"] = ("blocks", ((0, 16),), 1024, None, (1024, "window"))  # two CPIs, stride > N: one launch per CPI
BIT_CASES["long_9000_taps"] = ("long", ((0, 9000),), 0, None, None)  # 5 chunks of 2048 taps on 40 000 samples

# name -> (first lag, last lag, forced F, the plan the handle must report)
SPEED_CASES = {
    "410_taps_f2048_window": (-10, 400, 0, (2048, "window")),   # the bench's filter
    "1015_taps_f2048_half": (0, 1015, 0, (2048, "half")),
    "1800_taps_f4096_half": (0, 1800, 0, (4096, "half")),
    "2500_taps_f4096_window": (0, 2500, 0, (4096, "window")),   # the one-workgroup instantiation
    "410_taps_f1024_forced_half": (-10, 400, 1024, (1024, "half")),
}
N_SPEED, B_SPEED = 2_000_000, 32


def sha(a):
    return hashlib.sha256(a.tobytes()).hexdigest()[:24]


def scene(n, rows, seed, n_surv=1):
    """Integer-valued channels within int8: a white reference, surveillance = delayed copies of it + noise."""
    import numpy as np
    rng = np.random.default_rng(seed)
    x = rng.integers(-60, 61, (rows, n, 2)).astype(np.int16)
    ys = []
    for k in range(n_surv):
        y = (np.roll(x, 3 + k, axis=1) // 2) + (np.roll(x, 40 + 5 * k, axis=1) // 4) + rng.integers(-20, 21, (rows, n, 2))
        ys.append(np.clip(y, -128, 127).astype(np.int16))
    return x, ys


def to_device(torch, b2, fmt, x, ys, stride):
    """(pointer of x, [pointers of y], the tensors that keep them alive); rows `stride` apart, filler in the gaps."""
    import numpy as np
    rows, n = x.shape[:2]
    if fmt == b2.FMT_I16:
        host = np.full((rows, max(stride, n), 4), 777, dtype=np.int16)
        host[:, :n, 0:2], host[:, :n, 2:4] = x, ys[0]
        t = torch.from_numpy(host).cuda()
        return t.data_ptr(), [0], [t]
    planes = []
    for ch in [x] + list(ys):
        if fmt == b2.FMT_I8:
            host = np.full((rows, max(stride, n), 2), 77, dtype=np.int8)
            host[:, :n] = ch
        else:
            host = np.full((rows, max(stride, n)), FILL + 1j * FILL, dtype=np.complex64)
            host[:, :n] = ch[..., 0] + 1j * ch[..., 1]
        planes.append(torch.from_numpy(host).cuda())
    return planes[0].data_ptr(), [p.data_ptr() for p in planes[1:]], planes


def check_plan(wh, want, name):
    got = (wh.fft_len, wh.plan_info()["corr"])
    if got != want:
        sys.exit(f"{name}: the handle reports the plan {got}, the case names {want}")


def last_digests(wh, count):
    import numpy as np
    h = hashlib.sha256()
    for v in range(count):
        ok, w, r, b = wh.read_last(v)
        for a in (np.array([ok], dtype=np.int32), w, r, b):
            h.update(a.tobytes())
    return h.hexdigest()[:24]


def child_bits(name):
    import numpy as np
    import torch

    import blah2_amd as b2
    kind, lag_list, F, form, plan = BIT_CASES[name]
    st = torch.cuda.current_stream().cuda_stream
    lines = []
    n, B, stride = N_BITS, B_BITS, N_BITS + GAP
    blocks, K = 1, 1
    fmts = FMTS
    if kind == "lone":
        B, stride = 1, 0
    if kind == "multi":
        K, fmts = 3, ("FMT_C32", "FMT_I8")
    if kind == "blocks":
        n, B, blocks = 8192, 2, 4
        stride = n + GAP
    if kind == "long":
        n, B, fmts = 40_000, 1, ("FMT_C32",)
        stride = n
    x, ys = scene(n, B, seed=sum(name.encode()), n_surv=K)
    for (dmin, dmax), fmt_name in ((lg, f) for lg in lag_list for f in fmts):
        fmt = getattr(b2, fmt_name)
        wh = b2.WienerHopf(dmin, dmax, n, max_batch=B, blocks=blocks)
        if F:
            wh.set_fft_len(F)
        if form:
            wh.set_corr_form(form)
        if kind == "long":
            assert wh.plan_info()["chunks"] == -(-(dmax - dmin) // 2048), wh.plan_info()
        else:
            check_plan(wh, plan, name)
        px, pys, keep = to_device(torch, b2, fmt, x, ys, stride)
        row = max(stride, n)
        outs = [torch.full((B, row), FILL + 1j * FILL, dtype=torch.complex64, device="cuda") for _ in range(K)]
        ok = torch.full((K * B * blocks + 4,), 7, dtype=torch.int32, device="cuda")  # the four slots behind stay 7
        if kind == "multi":
            wh.process_multi_dev(fmt, px, pys, B, stride, [o.data_ptr() for o in outs], stride, ok.data_ptr(), st)
        else:
            wh.process_dev_fmt(fmt, px, pys[0], B, stride, outs[0].data_ptr(), stride, ok.data_ptr(), st)
        torch.cuda.synchronize()
        okh = ok.cpu().numpy()
        if not (okh[:-4] == 1).all():
            sys.exit(f"{name} {fmt_name}: a solve failed on the crafted scene, ok = {okh.tolist()}")
        d = {"ok": sha(okh), "last": last_digests(wh, K * B * blocks), "planes": sha(np.stack([o.cpu().numpy() for o in outs]))}
        if kind in ("single", "lone"):
            ok.fill_(7)
            wh.estimate_dev_fmt(fmt, px, pys[0], B, stride, ok.data_ptr(), st)
            torch.cuda.synchronize()
            d["estimate_ok"] = sha(ok.cpu().numpy())
            d["estimate_last"] = last_digests(wh, B)
        lines.append({"lags": [dmin, dmax], "format": fmt_name, "fft_len": wh.fft_len, "corr": wh.plan_info()["corr"], **d})
        wh.close()
        del keep, outs
    print("RESULT " + json.dumps(lines), flush=True)


def child_speed(name, steps, warmup):
    import torch

    import blah2_amd as b2
    dmin, dmax, F, plan = SPEED_CASES[name]
    st = torch.cuda.current_stream().cuda_stream
    n, B = N_SPEED, B_SPEED
    res = {}
    for fmt_name in FMTS:
        fmt = getattr(b2, fmt_name)
        torch.manual_seed(len(name) + fmt)
        x = (30.0 * torch.randn((B, n, 2), dtype=torch.float32, device="cuda")).round().clamp(-128, 127)
        y = (0.1 * 30.0 * torch.randn((B, n, 2), dtype=torch.float32, device="cuda") + 0.8 * x).round().clamp(-128, 127)
        if fmt == b2.FMT_I8:
            x, y = x.to(torch.int8), y.to(torch.int8)
            px, py = x.data_ptr(), y.data_ptr()
        elif fmt == b2.FMT_I16:
            x = torch.cat([x, y], dim=2).to(torch.int16)
            y = None
            px, py = x.data_ptr(), 0
        else:
            px, py = x.data_ptr(), y.data_ptr()
        out = torch.empty((B, n), dtype=torch.complex64, device="cuda")
        ok = torch.zeros((B,), dtype=torch.int32, device="cuda")
        wh = b2.WienerHopf(dmin, dmax, n, max_batch=B)
        if F:
            wh.set_fft_len(F)
        check_plan(wh, plan, name)
        for _ in range(warmup):
            wh.process_dev_fmt(fmt, px, py, B, n, out.data_ptr(), n, ok.data_ptr(), st)
        torch.cuda.synchronize()
        wh.set_timing(True)
        wh.get_timing()
        for _ in range(steps):
            wh.process_dev_fmt(fmt, px, py, B, n, out.data_ptr(), n, ok.data_ptr(), st)
        torch.cuda.synchronize()
        ms, brackets = wh.get_timing()["clutter_corr"]
        wh.set_timing(False)
        assert brackets == steps, (brackets, steps)
        res[fmt_name] = {"corr_ms_per_step": ms / steps, "ok": int(ok.sum().item())}
        wh.close()
        del x, y, out
    res["device"] = torch.cuda.get_device_name(0)
    res["arch"] = torch.cuda.get_device_properties(0).gcnArchName
    print("RESULT " + json.dumps(res), flush=True)


def run_child(args, lib, limit):
    """One child under its own time limit; any non-zero status ends the whole run."""
    env = dict(os.environ)
    env.pop("BLAH2HIP_LIBRARY", None)
    if lib:
        env["BLAH2HIP_LIBRARY"] = lib
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), *args]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:  # a fault, an abort, a time limit, a wrong plan: nothing more is started on the GPU
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit(f"{' '.join(args)} ({lib or 'the product library'}): exit status {r.returncode}; stopping")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def bits(a, lib_a, lib_b):
    bad = []
    for name in (a.cases.split(",") if a.cases else BIT_CASES):
        ra = run_child(["--child", "bits", name], lib_a, a.step_timeout)
        rb = run_child(["--child", "bits", name], lib_b, a.step_timeout)
        same = ra == rb
        print(f"{name:28s} {'equal' if same else 'DIFFERENT'}  " + " ".join(f"{r['lags'][0]}..{r['lags'][1]}/{r['format'][4:]}:{r['fft_len']},{r['corr']}" for r in rb), flush=True)
        if not same:
            bad.append(name)
            print("  A " + json.dumps(ra) + "\n  B " + json.dumps(rb), flush=True)
    if bad:
        sys.exit(f"digests differ in {len(bad)} case(s): {', '.join(bad)}")
    print("every digest of B equals A's")


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def speed(a, lib_a, lib_b):
    out = {"what": "BLAH2HIP_CK_CORR slot of blah2hip_clutter_process_dev_fmt, ms per step of 32 CPIs of 2 000 000 samples",
           "libraries": {"A": "the parent commit (tools/build_variant.sh, BLAH2HIP_LIBRARY)", "B": a.lib_b or "this tree's product library"},
           "pairs": a.pairs, "steps_per_leg": a.steps, "warmup_per_leg": a.warmup,
           "rule": "as fast: every pair's B / A at most 1 + the larger same-library spread ((max - min) / median over the legs)",
           "cases": []}
    if os.path.exists(a.out) and a.cases:  # a run in several visits: keep what the earlier ones measured
        out = json.load(open(a.out))
    slower = []
    for name in (a.cases.split(",") if a.cases else SPEED_CASES):
        legs = {"A": [], "B": []}
        for _ in range(a.pairs):
            for which, lib in (("A", lib_a), ("B", lib_b)):
                legs[which].append(run_child(["--child", "speed", name, "--steps", str(a.steps), "--warmup", str(a.warmup)], lib, a.step_timeout))
        out["device"], out["arch"] = legs["B"][0]["device"], legs["B"][0]["arch"]
        for fmt in FMTS:
            ta = [leg[fmt]["corr_ms_per_step"] for leg in legs["A"]]
            tb = [leg[fmt]["corr_ms_per_step"] for leg in legs["B"]]
            s = max(spread(ta), spread(tb))
            ratios = [q / p for p, q in zip(ta, tb)]
            case = {"case": name, "format": fmt, "fft_len": SPEED_CASES[name][3][0], "corr": SPEED_CASES[name][3][1],
                    "A_ms_per_step": ta, "B_ms_per_step": tb, "B_over_A": ratios, "same_library_spread": {"A": spread(ta), "B": spread(tb)},
                    "as_fast": all(r <= 1.0 + s for r in ratios)}
            print(json.dumps(case), flush=True)
            if not case["as_fast"]:
                slower.append(f"{name} {fmt}")
            out["cases"] = [c for c in out["cases"] if (c["case"], c["format"]) != (name, fmt)] + [case]  # a re-run replaces
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)  # after every case: a later stop keeps what was measured
    if slower:
        sys.exit("slower beyond the spread: " + ", ".join(slower))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", action="store_true")
    ap.add_argument("--speed", action="store_true")
    ap.add_argument("--lib-a", default=os.path.join(ROOT, "tools", "ab", "libblah2hip_parent.so"))
    ap.add_argument("--lib-b", default="", help="B from a file too (a copy of A's file: the control, one code object against itself)")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds a child process may take")
    ap.add_argument("--cases", default="", help="comma-separated case names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_clutter_corr_unify.json"))
    ap.add_argument("--child", nargs=2, metavar=("KIND", "CASE"))
    a = ap.parse_args()
    if a.child:
        return child_bits(a.child[1]) if a.child[0] == "bits" else child_speed(a.child[1], a.steps, a.warmup)
    lib_a = os.path.abspath(a.lib_a)
    if not os.path.exists(lib_a):
        sys.exit(f"{lib_a} is missing: build the parent commit's library with tools/build_variant.sh parent")
    lib_b = os.path.abspath(a.lib_b) if a.lib_b else None
    if a.pairs < 3:
        sys.exit("at least three pairs")
    if a.bits:
        bits(a, lib_a, lib_b)
    if a.speed:
        speed(a, lib_a, lib_b)


if __name__ == "__main__":
    main()
