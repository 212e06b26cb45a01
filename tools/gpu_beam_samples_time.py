#!/usr/bin/env python3
"""Time per call of the sample-domain covariance and beam planes against the memory system, and of the adaptive beam
formed in the sample domain against the one formed in the map domain, all in one process.

    python tools/gpu_beam_samples_time.py [--launches 100] [--warmup 50] [--out profiles/r13_beam_samples_time.json]

configs[1] geometry (2 000 000 samples per CPI, 513 x 411 cells), K = 4 and 8 channels, int8 and fp32 planes, n_cpi = 16
and 1; the covariance over the whole CPI, beam planes for 1 and 2 beams.

(a) Each kernel against the memory system.  The kernels' times are blah2hip_amb_set_timing's BLAH2HIP_K_COV
(sample_cov_kernel + cov_fold_kernel) and BLAH2HIP_K_BEAM (beam_samples_kernel), read after every call: the median of
`--launches` calls behind `--warmup` untimed ones.  The covariance reads K * n * s_in bytes per CPI (s_in = 2 for int8
pairs, 8 for fp32 pairs); the beams read that and write n_beams * n * 8.  The yardsticks, bracketed by an event pair per
launch, median of as many launches: blah2hip_stream_read_dev over the SAME planes (the bytes the kernels read), and for the
beams also a device-to-device copy of (read + written) / 2 bytes, which moves read + written bytes in all.  A kernel's
rate is reported as a fraction of those rates; it is never compared with its own earlier runs.

(b) One adaptive beam from K = 4 int8 channels, n_cpi = 16, each sequence bracketed by an event pair per call, the two
alternating call by call:
  sample domain   sample_covariance_dev, mvdr_weights_dev, beam_samples_wdev, process_dev(FMT_I8X_C32Y)
  map domain      process_multi_dev(FMT_I8), covariance_dev, mvdr_weights_dev, beamform_wdev
The two differ in where the covariance is estimated -- over the samples of the CPI, or over the cells of the channel maps
-- so their weights, and their beams, are not the same numbers; what is compared is the cost of one adaptive beam map.

One process; run it under a time limit."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_beam_samples_time.json"))
    a = ap.parse_args()
    if a.launches < 50:
        sys.exit("at least 50 launches")
    import torch

    import blah2_amd as b2
    L = b2.load()
    amb = b2.Ambiguity(*CFG2, True, max_batch=8 * 16)
    n = amb.get_n_samples()
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    st = torch.cuda.current_stream().cuda_stream
    res = {"geometry": f"configs[1]: {n} samples, {nD} x {nC}", "window": "the whole CPI", "loading": 1e-3, "launches": a.launches,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "kernels": [], "adaptive_beam": None}

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

    def slot_us(enqueue, slot):
        for _ in range(a.warmup):
            enqueue()
        torch.cuda.synchronize()
        amb.set_timing(True)
        amb.get_timing()
        us = []
        for _ in range(a.launches):
            enqueue()
            ms, cnt = amb.get_timing()[slot]  # synchronises
            assert cnt == 1
            us.append(ms * 1e3)
        amb.set_timing(False)
        return statistics.median(us), min(us)

    def planes(fmt_i8, K, n_cpi):
        """K planes in one allocation (so one stream_read covers them): (tensor, pointers, bytes)"""
        if fmt_i8:
            t = torch.randint(-100, 101, (K, n_cpi * n, 2), dtype=torch.int8, device="cuda")
        else:
            t = torch.randn((K, n_cpi * n, 2), dtype=torch.float32, device="cuda")
        return t, [t[k].data_ptr() for k in range(K)], t.numel() * t.element_size()

    # ---- (a) the kernels against the memory system ----
    for K in (4, 8):
        for fmt_i8 in (True, False):
            fmt = b2.FMT_I8 if fmt_i8 else b2.FMT_C32
            for n_cpi in (16, 1):
                t, ptrs, in_bytes = planes(fmt_i8, K, n_cpi)
                cov = torch.empty((n_cpi, K, K, 2), dtype=torch.float64, device="cuda")
                cov_us, cov_min = slot_us(lambda: amb.sample_covariance_dev(fmt, ptrs, n_cpi, n, cov.data_ptr(), None, st), "cov")
                read_us, read_min = median_us(lambda: b2._lib.check(L.blah2hip_stream_read_dev(t.data_ptr(), in_bytes, None, st)))
                case = {"kernel": "sample_cov_kernel + cov_fold_kernel", "fmt": "int8" if fmt_i8 else "fp32", "n_surv": K, "n_cpi": n_cpi,
                        "bytes": in_bytes, "us_median": cov_us, "us_min": cov_min, "gbs": in_bytes / cov_us / 1e3,
                        "read_kernel": "blah2hip_stream_read_dev", "read_us_median": read_us, "read_us_min": read_min,
                        "read_gbs": in_bytes / read_us / 1e3}
                case["over_read_rate"] = case["gbs"] / case["read_gbs"]
                print(json.dumps(case), flush=True)
                res["kernels"].append(case)
                for nb in (1, 2):
                    out = torch.empty((nb, n_cpi * n, 2), dtype=torch.float32, device="cuda")
                    outs = [out[b].data_ptr() for b in range(nb)]
                    w = b2.ula_weights(K, 0.5, [20.0, -35.0][:nb])
                    out_bytes = out.numel() * 4
                    beam_us, beam_min = slot_us(lambda: amb.beam_samples_dev(fmt, ptrs, n_cpi, n, w, outs, n, st), "beam")
                    half = (in_bytes + out_bytes) // 2
                    src = torch.empty((half,), dtype=torch.int8, device="cuda")
                    dst = torch.empty((half,), dtype=torch.int8, device="cuda")
                    copy_us, copy_min = median_us(lambda: dst.copy_(src))
                    case = {"kernel": "beam_samples_kernel", "fmt": "int8" if fmt_i8 else "fp32", "n_surv": K, "n_beams": nb, "n_cpi": n_cpi,
                            "bytes_read": in_bytes, "bytes_written": out_bytes, "us_median": beam_us, "us_min": beam_min,
                            "gbs": (in_bytes + out_bytes) / beam_us / 1e3, "read_us_median": read_us,
                            "read_gbs": in_bytes / read_us / 1e3, "copy": "device-to-device copy of (read + written) / 2 bytes",
                            "copy_us_median": copy_us, "copy_us_min": copy_min, "copy_gbs": 2 * half / copy_us / 1e3}
                    case["over_copy_rate"] = case["gbs"] / case["copy_gbs"]
                    case["over_read_rate"] = case["gbs"] / case["read_gbs"]
                    print(json.dumps(case), flush=True)
                    res["kernels"].append(case)
                    del out, src, dst
                del t, cov

    # ---- (b) one adaptive beam from K = 4 int8 channels, n_cpi = 16 ----
    K, n_cpi = 4, 16
    t, ptrs, _ = planes(True, K, n_cpi)
    x = torch.randint(-100, 101, (n_cpi * n, 2), dtype=torch.int8, device="cuda")
    steer = b2.ula_steering(K, 0.5, [20.0])
    cov = torch.empty((n_cpi, K, K, 2), dtype=torch.float64, device="cuda")
    w = torch.empty((n_cpi, 1, K, 2), dtype=torch.float32, device="cuda")
    ok = torch.empty((n_cpi,), dtype=torch.int32, device="cuda")
    beam = torch.empty((n_cpi * n, 2), dtype=torch.float32, device="cuda")
    bmap = torch.empty((n_cpi, nD, nC, 2), dtype=torch.float32, device="cuda")
    bmet = torch.empty((n_cpi, 2), dtype=torch.float64, device="cuda")
    cmaps = torch.empty((K, n_cpi, nD, nC, 2), dtype=torch.float32, device="cuda")
    cmet = torch.empty((K, n_cpi, 2), dtype=torch.float64, device="cuda")

    def sample_domain():
        amb.adaptive_beam_samples_dev(b2.FMT_I8, ptrs, n_cpi, n, steer, 1e-3, cov.data_ptr(), w.data_ptr(), ok.data_ptr(), [beam.data_ptr()],
                                      n, None, st)
        amb.process_dev(b2.FMT_I8X_C32Y, x.data_ptr(), beam.data_ptr(), n_cpi, n, bmap.data_ptr(), bmet.data_ptr(), st)

    def map_domain():
        amb.process_multi_dev(b2.FMT_I8, x.data_ptr(), ptrs, n_cpi, n, cmaps.data_ptr(), cmet.data_ptr(), st)
        amb.adaptive_beamform_dev(cmaps.data_ptr(), K, n_cpi, steer, 1e-3, cov.data_ptr(), w.data_ptr(), ok.data_ptr(), bmap.data_ptr(),
                                  bmet.data_ptr(), None, st)

    # the two sequences alternate call by call, so that whatever else the machine does meets both alike
    for _ in range(a.warmup):
        sample_domain()
        map_domain()
    torch.cuda.synchronize()
    us = {sample_domain: [], map_domain: []}
    for _ in range(a.launches):
        for seq in (sample_domain, map_domain):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            seq()
            e1.record()
            e1.synchronize()
            us[seq].append(e0.elapsed_time(e1) * 1e3)
            assert bool((ok == 1).all())
    s_us, s_min = statistics.median(us[sample_domain]), min(us[sample_domain])
    m_us, m_min = statistics.median(us[map_domain]), min(us[map_domain])
    res["adaptive_beam"] = {
        "n_surv": K, "n_cpi": n_cpi, "n_beams": 1, "fmt": "int8",
        "sample_domain": "sample_covariance_dev, mvdr_weights_dev, beam_samples_wdev, process_dev(FMT_I8X_C32Y)",
        "sample_domain_us_median": s_us, "sample_domain_us_min": s_min,
        "map_domain": "process_multi_dev(FMT_I8), covariance_dev, mvdr_weights_dev, beamform_wdev",
        "map_domain_us_median": m_us, "map_domain_us_min": m_min, "map_over_sample": m_us / s_us,
        "note": "the covariance is estimated over the CPI's samples in the first sequence and over the channel maps' cells in the "
                "second: the weights differ, the cost of one adaptive beam map is what is compared"}
    print(json.dumps(res["adaptive_beam"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
