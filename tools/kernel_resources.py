#!/usr/bin/env python3
"""Register / scratch / LDS / occupancy table of every kernel in a .hip file
(hipcc -Rpass-analysis=kernel-resource-usage; cross-compiles, no GPU needed).

    python tools/kernel_resources.py blah2_amd/csrc/capi.hip [filter]
    python tools/kernel_resources.py --json profiles/r26_clutter_resources_new.json blah2_amd/csrc/clutter.hip blah2_amd/csrc/clutter_solve.hip

One unit a call: the library is several .hip files (capi.hip holds the range and Doppler kernels, clutter.hip the clutter
filter's correlation and FIR kernels and clutter_solve.hip every instantiation of its Toeplitz solve, spectrum.hip the
spectrum analyser's, array.hip the beam kernels, detect.hip the detectors', integrate.hip, taper.hip and walk.hip a family
each), so the whole library is a loop over blah2_amd/csrc/*.hip.  Host-only headers such as cfar_alpha.hpp hold no kernel and
do not show up.

--json: the tables of several units in one file, for comparing two arrangements of the same kernels: {"kernels": {name:
figures}, "instantiated_twice": [names that more than one of the units holds]}, the names without namespaces, return type
and argument list (a kernel that moves between units or namespaces keeps its name).

(SGPRs: this compiler prints the count as `TotalSGPRs`, older ones as `SGPRs`; both are read.)
"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
        return dict(zip(names, out))
    except FileNotFoundError:
        return {n: n for n in names}


def table(src, extra=()):
    """{demangled kernel name: figures} of one unit"""
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "blah2_amd", "csrc"), "-c", src, "-o", "/dev/null",
           "-Rpass-analysis=kernel-resource-usage", *extra]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    rec, name = {}, None
    keys = {"VGPRs": r"\bVGPRs: (\d+)", "AGPRs": r"AGPRs: (\d+)", "scratch": r"ScratchSize \[bytes/lane\]: (\d+)",
            "occ": r"Occupancy \[waves/SIMD\]: (\d+)", "vspill": r"VGPRs Spill: (\d+)", "lds": r"LDS Size \[bytes/block\]: (\d+)",
            "SGPRs": r"\b(?:Total)?SGPRs: (\d+)"}
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            rec[name] = {}
            continue
        for k, pat in keys.items():
            m = re.search(pat, line)
            if m and name:
                rec[name][k] = int(m.group(1))
    dm = demangle(list(rec))
    return {dm[n]: r for n, r in rec.items()}


def plain_name(d):
    d = re.sub(r"\(anonymous namespace\)::|\b[a-z0-9_]+::", "", d)
    return re.sub(r"\(.*\)$", "", re.sub(r"^void ", "", d))


def main():
    if sys.argv[1] == "--json":
        kernels, twice = {}, []
        for src in sys.argv[3:]:
            for d, r in table(src).items():
                n = plain_name(d)
                if n in kernels:
                    twice.append(n)
                kernels[n] = r
        with open(sys.argv[2], "w") as f:
            json.dump({"kernels": dict(sorted(kernels.items())), "instantiated_twice": twice}, f, indent=1)
        print(f"{len(kernels)} kernels, {len(twice)} in more than one unit")
        return
    flt = sys.argv[2] if len(sys.argv) > 2 else ""
    for d, r in table(sys.argv[1], sys.argv[3:]).items():
        if flt and flt not in d:
            continue
        print(f"{d[:100]:100s} " + " ".join(f"{k}={v}" for k, v in r.items()))


if __name__ == "__main__":
    main()
