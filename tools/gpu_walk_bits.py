#!/usr/bin/env python3
"""SHA-256 of everything the two walk-sum entry points write, for comparing two builds of the library bit for bit.

    python tools/gpu_walk_bits.py [--out profiles/r21_walk_bits.json]
    BLAH2HIP_LIBRARY=/path/to/another/libblah2hip.so python tools/gpu_walk_bits.py --out profiles/r21_walk_bits_parent.json

On the five geometries off the grid of 32 pulses (tests/migrate_scenes.py EDGE_GEOMS: 21 x 64, 48 x 65, 81 x 200, 95 x 64,
7 x 64), three impulse-reference CPIs through process_dev, then
  * migrate_dev with the tables physical, limit and jagged;
  * rate_bank_dev with the banks {0}, -2 .. 2 and -8 .. 7, each with those tables and with none, with and without the index plane;
each for n_maps 1 and 3, in place and out of place (a bank that set_rates refuses -- -8 .. 7 at 7 Doppler bins -- is recorded
with the error's text).  Every launch starts from the same maps and from output buffers filled
with 0xff bytes.  "entries" of the JSON file maps a case, one a line, to one SHA-256 over the output maps, index plane and
metrics pairs of its four launches (n_maps 1 and 3, out of place and in place): two builds compute the same bits exactly when their "entries" are equal.  Only the public Python API is used, so the file runs on any tree
that has the two entry points.  One process; run it under a time limit."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TABLES = ("physical", "limit", "jagged")
N_CPI = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_walk_bits.json"))
    a = ap.parse_args()
    import numpy as np
    import torch

    import blah2_amd as b2
    import migrate_scenes as MS
    st = torch.cuda.current_stream().cuda_stream
    banks = {"zero": np.zeros(1), "m2to2": np.arange(-2.0, 3.0), "m8to7": np.arange(-8.0, 8.0)}
    entries = {}

    def feed(h, t, n):
        h.update(t[:n].cpu().numpy().tobytes())

    for geom in MS.EDGE_GEOMS:
        dims = MS.dims_of(geom)
        limits, bins = MS.GEOMS[geom]
        amb = b2.Ambiguity(*limits, True, max_batch=N_CPI, n_doppler_bins=bins)
        amb.set_hot_columns(0)
        amb.set_leak_compensation(0)
        nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
        x, y, stride = MS.impulse_cpis(dims, N_CPI, seed=21)
        dx = torch.from_numpy(x.view(np.float32).copy()).cuda()
        dy = torch.from_numpy(y.view(np.float32).copy()).cuda()
        maps = torch.empty((N_CPI, nD, nC), dtype=torch.complex64, device="cuda")
        met = torch.empty((N_CPI, 2), dtype=torch.float64, device="cuda")
        amb.process_dev(b2.FMT_C32, dx.data_ptr(), dy.data_ptr(), N_CPI, stride, maps.data_ptr(), met.data_ptr(), st)
        torch.cuda.synchronize()
        h = hashlib.sha256()
        feed(h, maps, N_CPI)
        feed(h, met, N_CPI)
        entries[f"{geom} process"] = h.hexdigest()
        work = torch.empty_like(maps)
        out = torch.empty_like(maps)
        index = torch.empty((N_CPI, nD, nC), dtype=torch.uint8, device="cuda")
        tabs = MS.tables(dims, MS.CELLS[geom])

        def run(tag, launch, with_index):
            h = hashlib.sha256()  # of the case's four launches, in this order: maps, index plane, metrics of each
            for n_maps in (1, N_CPI):
                for in_place in (False, True):
                    work.copy_(maps)
                    for t in (out, index, met):
                        t.view(torch.uint8).fill_(0xff)
                    dst = work if in_place else out
                    launch(n_maps, dst)
                    torch.cuda.synchronize()
                    feed(h, dst, n_maps)
                    if with_index:
                        feed(h, index, n_maps)
                    feed(h, met, n_maps)
                    if not in_place:
                        assert torch.equal(work.view(torch.float32), maps.view(torch.float32)), "the input maps were written"
            entries[f"{geom} {tag}"] = h.hexdigest()

        for table in TABLES + ("none",):
            amb.set_migration(None if table == "none" else tabs[table])
            if table != "none":
                run(f"migrate table={table}",
                    lambda n_maps, dst: amb.migrate_dev(work.data_ptr(), n_maps, dst.data_ptr(), met.data_ptr(), st), False)
            for bank, q in banks.items():
                try:
                    amb.set_rates(q)
                except b2.Blah2HipError as e:  # -8 .. 7 on the 7 x 64 map: a rate beyond n_doppler bins
                    entries[f"{geom} rate bank={bank} table={table}"] = {"refused": str(e)}
                    continue
                for with_index in (False, True):
                    run(f"rate bank={bank} table={table} index={'yes' if with_index else 'no'}",
                        lambda n_maps, dst: amb.rate_bank_dev(work.data_ptr(), n_maps, dst.data_ptr(),
                                                              index.data_ptr() if with_index else None, met.data_ptr(), st),
                        with_index)
        amb.close()
    head = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
            "n_launches": 4 * sum(isinstance(v, str) and not k.endswith(" process") for k, v in entries.items())}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:  # one case a line
        f.write(json.dumps(head)[:-1] + ', "entries": {\n')
        f.write(",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in entries.items()) + "\n}}\n")
    json.load(open(a.out))
    print(json.dumps({"out": os.path.relpath(a.out, ROOT), **head,
                      "sha256_of_entries": hashlib.sha256(json.dumps(entries, sort_keys=True).encode()).hexdigest()}))


if __name__ == "__main__":
    main()
