#!/usr/bin/env python3
"""SHA-256 of everything the clutter filter's entry points write, for comparing two builds of the library bit for bit.

    python tools/clutter_parity.py --out profiles/r26_clutter_parity_new.json
    BLAH2HIP_LIBRARY=/path/to/another/libblah2hip.so python tools/clutter_parity.py --out profiles/r26_clutter_parity_parent.json

Builds nothing.  A fixed table of small cases on seeded inputs (a reference of white noise, surveillance channels that
hold a few delayed copies of it plus noise of their own) through every launch path of csrc/clutter.hip and
csrc/clutter_solve.hip:
  * plain filter: fp32 planes, int16 words and int8 planes; the transform length forced to 1024, 2048 and 4096; the
    correlation form forced to window and to half; batches of 1 and of 3 with cpi_stride > N; 33 taps on 6 011 samples
    (first lag +5) and 410 taps on 19 997; the FIR carry on and off where the planner carries it (1 000 taps at F = 2048);
    estimate_dev_fmt (no output plane); a forced correlation grid of 8;
  * solve: the look-ahead form at 2, 3, 6 and 12 indices per lane and the stepwise form at 1, 2 and 4 indices per thread,
    through solve() and solve_dev() on a fixed r, b; a system that is not positive definite;
  * several channels: K = 1, 2, 3 and 5 on fp32 and int8 planes, with and without output planes, then a single-channel
    call on the same handle (read_last and taps_dev switch back);
  * blocks: four blocks a CPI shorter than two filter lengths (direct correlations) and longer (transforms), CPIs back
    to back and with a stride, estimate only, and process() through the host entry point;
  * long filter: 4 610 taps on 60 000 samples (tests/golden's long_filter), a lone CPI with stride 0, a batch of 2, and
    the multi entry point with K = 2.
Every launch starts from output planes and flags filled with 0xff bytes, and the whole buffers are hashed, stride gaps
included.  "entries" of the JSON file maps a case, one a line, to {"sha256": over the flags, the output planes and
read_last's (ok, w, r, b) of every virtual CPI, "info": what get_info reports behind the call}: two builds compute the same
bits exactly when their "entries" are equal.  Only the public Python API is used.  One process, a few seconds; run it
under a time limit."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_clutter_parity.json"))
    a = ap.parse_args()
    import numpy as np
    import torch

    import blah2_amd as b2
    from blah2_amd import _lib
    L = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    entries = {}

    def scene(seed, n, n_cpi, stride, K, amp=20.0):
        """x [n_cpi][stride], ys K x [n_cpi][stride] complex64: small integers (exact in every format) plus, for y, three echoes"""
        rng = np.random.default_rng(seed)
        def noise(shape, s):
            return np.round(rng.normal(0, s, shape)) + 1j * np.round(rng.normal(0, s, shape))
        x = noise((n_cpi, stride), amp)
        ys = []
        for k in range(K):
            y = noise((n_cpi, stride), 3.0)
            for d, g in ((0, 1.0), (2 + k, 0.5), (7, -0.25)):
                y[:, :n] += np.round(g * np.roll(x[:, :n], d, axis=1))
            ys.append(np.clip(y.real, -120, 120) + 1j * np.clip(y.imag, -120, 120))
        x = np.clip(x.real, -120, 120) + 1j * np.clip(x.imag, -120, 120)
        return x.astype(np.complex64), [y.astype(np.complex64) for y in ys]

    def dev(fmt, x, y):
        """device buffers of one reference / surveillance pair in format fmt: (d_x, d_y, keep-alive tensors)"""
        if fmt == b2.FMT_C32:
            tx, ty = (torch.from_numpy(v.view(np.float32).copy()).cuda() for v in (x, y))
            return tx.data_ptr(), ty.data_ptr(), (tx, ty)
        if fmt == b2.FMT_I8:
            tx, ty = (torch.from_numpy(v.view(np.float32).astype(np.int8)).cuda() for v in (x, y))
            return tx.data_ptr(), ty.data_ptr(), (tx, ty)
        w = np.concatenate([x.view(np.float32).reshape(*x.shape, 2), y.view(np.float32).reshape(*y.shape, 2)], axis=-1)
        t = torch.from_numpy(w.astype(np.int16)).cuda()  # the .rspduo words: (xI, xQ, yI, yQ) per sample
        return t.data_ptr(), None, (t,)

    def info(wh):
        s, p = wh.solve_info(), wh.plan_info()
        return {"solve": [s["form"], s["E"], s["G"]], "corr": p["corr"], "corr_grid": wh.last_corr_grid(), "carry": p["carry"],
                "chunks": p["chunks"], "fft_len": wh.fft_len, "seg_len": wh.seg_len}

    def peek_taps(wh, rows):
        p, nb, _ = wh.taps_dev()
        host = np.empty((rows, nb), dtype=np.complex64)
        ctx = ctypes.c_void_p()
        assert L.blah2hip_ctx_create(0, ctypes.byref(ctx)) == 0
        assert L.blah2hip_ctx_d2h(ctx, host.ctypes.data, p, host.nbytes) == 0 and L.blah2hip_ctx_sync(ctx) == 0
        L.blah2hip_ctx_destroy(ctx)
        return host

    def record(name, wh, n_virtual, tensors):
        """the case's digest: the given device tensors whole, the taps through taps_dev, read_last of every virtual CPI"""
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.cpu().numpy().tobytes())
        h.update(peek_taps(wh, n_virtual).tobytes())
        for v in range(n_virtual):
            ok, w, r, b = wh.read_last(v)
            h.update(bytes([ok]) + w.tobytes() + r.tobytes() + b.tobytes())
        assert name not in entries, name
        entries[name] = {"sha256": h.hexdigest(), "info": info(wh)}

    def fresh(shape, dtype):
        t = torch.empty(shape, dtype=dtype, device="cuda")
        t.view(torch.uint8).fill_(0xff)
        return t

    def single(name, wh, fmt, x, y, n_cpi, stride, estimate=False, per_cpi=1):
        dx, dy, keep = dev(fmt, x[:n_cpi], y[:n_cpi])
        ok = fresh((n_cpi * per_cpi,), torch.int32)
        if estimate:
            wh.estimate_dev_fmt(fmt, dx, dy, n_cpi, stride, ok.data_ptr(), st)
            record(name, wh, n_cpi * per_cpi, [ok])
        else:
            ostride = max(stride, wh.nSamples) + 5  # (a lone CPI takes any cpi_stride, 0 included: the plane holds nSamples all the same)
            out = fresh((n_cpi, ostride), torch.complex64)
            wh.process_dev_fmt(fmt, dx, dy, n_cpi, stride, out.data_ptr(), ostride, ok.data_ptr(), st)
            record(name, wh, n_cpi * per_cpi, [ok, out])
        del keep

    FMTS = (("c32", b2.FMT_C32), ("i16", b2.FMT_I16), ("i8", b2.FMT_I8))

    # ---- plain filter
    for n_bins, dmin, n in ((33, 5, 6011), (410, -10, 19997)):
        stride = n + 37
        x, (y,) = scene(100 + n_bins, n, 3, stride, 1)
        wh = b2.WienerHopf(dmin, dmin + n_bins, n, max_batch=3)
        for fname, fmt in FMTS:
            for F in (1024, 2048, 4096):
                wh.set_fft_len(F)
                for corr in ("window", "half"):
                    wh.set_corr_form(corr)
                    for n_cpi in (1, 3):
                        single(f"plain taps={n_bins} {fname} F={F} corr={corr} n_cpi={n_cpi}", wh, fmt, x, y, n_cpi, stride)
        wh.set_fft_len(0)
        wh.set_corr_form("auto")
        for fname, fmt in FMTS:
            single(f"plain taps={n_bins} {fname} planner estimate n_cpi=3", wh, fmt, x, y, 3, stride, estimate=True)
        wh.set_corr_grid(8)
        single(f"plain taps={n_bins} c32 planner corr_grid=8 n_cpi=3", wh, b2.FMT_C32, x, y, 3, stride)
        single(f"plain taps={n_bins} c32 planner corr_grid=8 n_cpi=1", wh, b2.FMT_C32, x, y, 1, stride)
        wh.close()
    n_bins, dmin, n = 1000, -4, 12003  # segLen = F - nBins + 1 = 1049 in [F/2, F/2 + F/64] at F = 2048: the planner carries
    x, (y,) = scene(7, n, 2, n + 11, 1)
    wh = b2.WienerHopf(dmin, dmin + n_bins, n, max_batch=2)
    wh.set_fft_len(2048)
    for carry in (1, 0):
        wh.set_fir_carry(carry)
        wh.set_fft_len(2048)  # (reads the plan's dims back: the carry changes seg_len)
        for fname, fmt in (FMTS[0], FMTS[2]):
            single(f"carry={carry} taps={n_bins} {fname} n_cpi=2", wh, fmt, x, y, 2, n + 11)
    wh.close()

    # ---- solve alone
    n_bins = 410
    x, (y,) = scene(11, 19997, 3, 19997, 1)
    wh = b2.WienerHopf(-10, 400, 19997, max_batch=3)
    dx, dy, keep = dev(b2.FMT_C32, x, y)
    wh.estimate_dev_fmt(b2.FMT_C32, dx, dy, 3, 19997, None, st)
    torch.cuda.synchronize()
    rb = [wh.read_last(c)[2:] for c in range(3)]
    r, b = np.stack([p[0] for p in rb]), np.stack([p[1] for p in rb])
    r_bad = r.copy()
    r_bad[0, 1] = 2.0 * r_bad[0, 0]  # |r[1]| > r[0]: not positive definite, ok = 0 for that system alone
    forms = [("lookahead", E, 0) for E in (2, 3, 6, 12)] + [("stepwise", 0, K) for K in (1, 2, 4)] + [("auto", 0, 0)]
    for form, E, K in forms:
        wh.set_solve_form(form, E)
        wh.set_solve_indices_per_thread(K)
        for tag, rr in (("pd", r), ("not_pd", r_bad)):
            for n_sys in (1, 3):
                ok, w = wh.solve(rr[:n_sys], b[:n_sys])
                h = hashlib.sha256(ok.tobytes() + w.tobytes())
                d_rb = torch.from_numpy(np.ascontiguousarray(np.stack([rr[:n_sys], b[:n_sys]], axis=1)).view(np.float64)).cuda()
                d_w, d_ok = fresh((n_sys, n_bins), torch.complex64), fresh((n_sys,), torch.int32)
                wh.solve_dev(d_rb.data_ptr(), n_sys, d_w.data_ptr(), d_ok.data_ptr(), st)
                torch.cuda.synchronize()
                h.update(d_w.cpu().numpy().tobytes() + d_ok.cpu().numpy().tobytes())
                h.update(bytes([wh.read_last(n_sys - 1)[0]]))  # the flag read_last reports: solve_dev's d_ok
                entries[f"solve form={form} E={E} K={K} {tag} n={n_sys}"] = {"sha256": h.hexdigest(), "info": info(wh)}
    wh.close()
    del keep

    # ---- several surveillance channels on one reference
    n_bins, dmin, n, n_cpi = 410, -10, 19997, 2
    stride = n + 13
    x, ys = scene(21, n, n_cpi, stride, 5)
    for fname, fmt in (FMTS[0], FMTS[2]):
        wh = b2.WienerHopf(dmin, dmin + n_bins, n, max_batch=n_cpi)
        for K in (1, 2, 3, 5):
            planes = [dev(fmt, x, y) for y in ys[:K]]
            for with_out in (True, False):
                ok = fresh((K, n_cpi), torch.int32)
                outs = [fresh((n_cpi, stride), torch.complex64) for _ in range(K)] if with_out else None
                wh.process_multi_dev(fmt, planes[0][0], [p[1] for p in planes], n_cpi, stride,
                                     [o.data_ptr() for o in outs] if outs else None, stride, ok.data_ptr(), st)
                record(f"multi {fname} K={K} out={'yes' if with_out else 'no'}", wh, K * n_cpi, [ok] + (outs or []))
            del planes
        single(f"multi {fname} then single", wh, fmt, x, ys[0], n_cpi, stride)
        wh.close()

    # ---- taps per block
    for tag, n_bins, n in (("direct", 300, 4 * 500), ("transforms", 100, 4 * 1500)):  # L < 2 nBins, L >= 2 nBins
        x, (y,) = scene(31 + n_bins, n, 2, n + 24, 1)
        wh = b2.WienerHopf(-2, n_bins - 2, n, max_batch=2, blocks=4)
        xb = np.ascontiguousarray(x[:, :n]), np.ascontiguousarray(y[:, :n])
        for fname, fmt in FMTS:
            single(f"blocks {tag} {fname} back to back", wh, fmt, xb[0], xb[1], 2, n, per_cpi=4)
            single(f"blocks {tag} {fname} strided", wh, fmt, x, y, 2, n + 24, per_cpi=4)
        single(f"blocks {tag} c32 estimate strided", wh, b2.FMT_C32, x, y, 2, n + 24, estimate=True, per_cpi=4)
        ok, out = wh.process(xb[0][0], xb[1][0])
        torch.cuda.synchronize()
        h = hashlib.sha256(bytes([ok]) + np.asarray(out).tobytes())
        for v in range(4):
            okv, w, r, b = wh.read_last(v)
            h.update(bytes([okv]) + w.tobytes() + r.tobytes() + b.tobytes())
        entries[f"blocks {tag} process() on the host"] = {"sha256": h.hexdigest(), "info": info(wh)}
        wh.close()

    # ---- long filter (tests/golden long_filter: lags -10 .. 4599 on 60 000 samples)
    n, n_bins = 60_000, 4610
    x, ys = scene(41, n, 2, n + 16, 2)
    wh = b2.WienerHopf(-10, 4600, n, max_batch=2)
    single("long lone CPI stride=0", wh, b2.FMT_C32, x, ys[0], 1, 0)
    single("long n_cpi=2", wh, b2.FMT_C32, x, ys[0], 2, n + 16)
    planes = [dev(b2.FMT_C32, x, y) for y in ys]
    ok = fresh((2, 2), torch.int32)
    outs = [fresh((2, n + 16), torch.complex64) for _ in range(2)]
    wh.process_multi_dev(b2.FMT_C32, planes[0][0], [p[1] for p in planes], 2, n + 16, [o.data_ptr() for o in outs], n + 16,
                         ok.data_ptr(), st)
    record("long multi K=2", wh, 4, [ok] + outs)
    wh.close()

    head = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
            "n_cases": len(entries)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:  # one case a line
        f.write(json.dumps(head)[:-1] + ', "entries": {\n')
        f.write(",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in entries.items()) + "\n}}\n")
    json.load(open(a.out))
    print(json.dumps({"out": os.path.relpath(a.out, ROOT), **head,
                      "sha256_of_entries": hashlib.sha256(json.dumps(entries, sort_keys=True).encode()).hexdigest()}))


if __name__ == "__main__":
    main()
