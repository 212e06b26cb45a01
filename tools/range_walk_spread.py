#!/usr/bin/env python3
"""Exit-time spread of rangew1k_kernel's waves from a -DRANGEW_TRACE run (csrc/trace.hpp):

    bash tools/build_trace.sh
    BLAH2HIP_TRACE_EXITS=$PWD/exits.txt BLAH2HIP_LIBRARY=$PWD/tools/ab/lib_rangew_trace.so \\
        python bench.py --gpus 1 --steps 12 --warmup 3
    python tools/range_walk_spread.py exits.txt

Prints one JSON object: per traced launch (the last eight of the run) and as the median over them, how far behind the
launch's FIRST exit the waves leave (minimum, median, 99th percentile, maximum, in microseconds), the same split by
blockIdx.x & 7, the launch time (first start to last exit), the pulse time (launch time / most pulses of any wave) and
how many waves ran how many pulses.  The question it answers: a ticketed walk ends about half a pulse behind the mean
wave, so it can only pay where the last exit lies more than a pulse behind the median one.
"""
import json
import statistics
import sys


def quantiles(v):
    v = sorted(v)
    n = len(v)
    return {"min": round(v[0], 2), "median": round(v[n // 2], 2), "p99": round(v[min(n - 1, (99 * n) // 100)], 2), "max": round(v[-1], 2)}


def main():
    path = sys.argv[1]
    khz, slots = 100000, {}
    for line in open(path):
        if line.startswith("#"):
            f = line.split()
            khz = int(f[f.index("wall_clock_khz") + 1]) or khz
            continue
        slot, waves, wave, xcd, pulses, start, end = (int(x) for x in line.split())
        slots.setdefault(slot, []).append((wave, xcd, pulses, start, end))
    us = 1e3 / khz
    launches = []
    for slot in sorted(slots):
        rec = slots[slot]
        ran = [r for r in rec if r[2] > 0]
        if not ran:
            continue
        first = min(r[4] for r in ran)
        t0 = min(r[3] for r in rec)
        launch_us = (max(r[4] for r in ran) - t0) * us
        most = max(r[2] for r in ran)
        counts = {}
        for r in ran:
            counts[r[2]] = counts.get(r[2], 0) + 1
        d = {"slot": slot, "waves": len(rec), "waves_with_pulses": len(ran), "launch_us": round(launch_us, 1),
             "pulse_us": round(launch_us / most, 2), "waves_by_pulse_count": {str(k): counts[k] for k in sorted(counts)},
             "exit_behind_first_us": quantiles([(r[4] - first) * us for r in ran]),
             "start_spread_us": round((max(r[3] for r in rec) - t0) * us, 2),
             "by_xcd": {str(x): quantiles([(r[4] - first) * us for r in ran if r[1] == x]) for x in sorted({r[1] for r in ran})}}
        q = d["exit_behind_first_us"]
        d["max_behind_median_us"] = round(q["max"] - q["median"], 2)
        d["max_behind_median_pulses"] = round((q["max"] - q["median"]) / d["pulse_us"], 3)
        # by pulse count: where the waves of the short and the full share leave
        d["by_pulse_count"] = {str(k): quantiles([(r[4] - first) * us for r in ran if r[2] == k]) for k in sorted(counts)}
        launches.append(d)
    # the steady launches of one run share a shape: those with the most waves
    big = max(l["waves"] for l in launches)
    same = [l for l in launches if l["waves"] == big]
    out = {"wall_clock_khz": khz, "launches": launches,
           "median_over_launches": {k: round(statistics.median(l[k] for l in same), 3)
                                    for k in ("launch_us", "pulse_us", "max_behind_median_us", "max_behind_median_pulses")}}
    for k in ("min", "median", "p99", "max"):
        out["median_over_launches"]["exit_behind_first_us_" + k] = round(statistics.median(l["exit_behind_first_us"][k] for l in same), 2)
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
