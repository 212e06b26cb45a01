"""Times the clutter filter with taps per block (blah2hip_clutter_create_ex) against one tap set per CPI, stage by stage.

    python tools/gpu_clutter_blocks_time.py [--cpis 256] [--rounds 5] [--solve-e E] [--out FILE.json]

BASELINE configs[1] geometry: CPIs of 2 000 000 samples, 410 taps (lags -10 ... 399), 256 CPIs per step, the .rspduo int16
words read directly.  One handle per B in {1, 4, 8, 16}; B = 1 takes the code path and the kernels the filter had before
blocks existed, so it is the yardstick (never an earlier run of the block kernel).  Method: every handle runs once untimed,
then the variants ALTERNATE inside one process for --rounds rounds; per variant the per-stage device times come from the
handle's own brackets (BLAH2HIP_CK_CORR / _REDUCE / _SOLVE / _FIR, device events around each stage) and the call time from
device events around the whole call.  Reported per call of --cpis CPIs: the median over the rounds, and min ... max.

What to expect from the arithmetic: correlations and FIR stay one pass over the samples whatever B is; the solve does B times
the systems.  A FIR stage above 1.15 x the B = 1 FIR, or a correlation stage that grows with B, wants an explanation.
The samples are seeded pseudo-random words made on the device (surveillance = 0.8 x reference + noise): the kernels' time does
not depend on the values, and every flag is checked to be 1.  --solve-e E (2, 3, 6 or 12) fixes the slice width of the look-ahead
solve on the handles WITH blocks (BLAH2HIP_CLUTTER_OPT_SOLVE_E; B = 1 keeps the planner's choice): beyond one system per CU the
planner takes the widest slices, and the solve is the one stage that grows with B.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, DMIN, DMAX = 2_000_000, -10, 400
BLOCKS = (1, 4, 8, 16)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cpis", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--solve-e", type=int, default=0, help="indices per lane of the look-ahead solve on the handles with blocks (0 = planner)")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    a = ap.parse_args(argv)
    import numpy as np
    import torch

    import blah2_amd as b2
    if b2.device_count() == 0:
        raise SystemExit("no GPU visible: nothing to time")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(20240925)
    C = a.cpis
    iq = torch.empty((C, N, 4), dtype=torch.int16, device=dev)
    for c in range(C):  # CPI by CPI: the generator's temporaries stay small
        ref = torch.randint(-300, 301, (N, 2), generator=g, device=dev, dtype=torch.int32)
        noise = torch.randint(-30, 31, (N, 2), generator=g, device=dev, dtype=torch.int32)
        iq[c, :, :2] = ref.to(torch.int16)
        iq[c, :, 2:] = ((ref * 4) // 5 + noise).to(torch.int16)
    yf = torch.empty((C, N), dtype=torch.complex64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    handles, oks = {}, {}
    for B in BLOCKS:
        handles[B] = b2.WienerHopf(DMIN, DMAX, N, max_batch=C, blocks=B)
        oks[B] = torch.zeros(C * B, dtype=torch.int32, device=dev)
        if B > 1 and a.solve_e:
            handles[B].set_solve_form("auto", a.solve_e)

    def call(B):
        handles[B].process_dev_fmt(b2.FMT_I16, iq.data_ptr(), None, C, N, yf.data_ptr(), N, oks[B].data_ptr(), st)

    for B in BLOCKS:  # untimed: code objects, lazily built state
        call(B)
        torch.cuda.synchronize()
        assert bool(oks[B].all().item()), f"B = {B}: a block's matrix was not positive definite"
        handles[B].set_timing(True)
    names = list(b2._lib.CLUTTER_KERNEL_NAMES.values())
    samples = {B: {k: [] for k in names + ["call"]} for B in BLOCKS}
    for _ in range(a.rounds):
        for B in BLOCKS:
            handles[B].get_timing()  # (collect clears the brackets: what follows is this call's)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(B)
            e1.record()
            torch.cuda.synchronize()
            after = handles[B].get_timing()
            for k in names:
                samples[B][k].append(after[k][0])
            samples[B]["call"].append(e0.elapsed_time(e1))
    res = {"geometry": {"n_samples": N, "delayMin": DMIN, "delayMax": DMAX, "cpis_per_call": C, "fmt": "i16"},
           "rounds": a.rounds, "solve_e_with_blocks": a.solve_e, "unit": "ms per call", "blocks": {}}
    for B in BLOCKS:
        h = handles[B]
        res["blocks"][str(B)] = {"fft_len": h.fft_len, "seg_len": h.seg_len, "corr": h.plan_info()["corr"], "solve": h.solve_info(),
                                 **{k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
                                    for k, v in samples[B].items()}}
    fir1 = res["blocks"]["1"]["clutter_fir"]["median"]
    for B in BLOCKS:
        res["blocks"][str(B)]["fir_over_b1"] = res["blocks"][str(B)]["clutter_fir"]["median"] / fir1
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
