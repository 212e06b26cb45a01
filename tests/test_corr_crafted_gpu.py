"""GPU: the clutter filter's FFT correlations (clutter_corr_kernel, clutter_corr_half_kernel, csrc/clutter_kernels.hpp) on the pair
census of tests/corr_crafted.py with the correlation grid forced (WienerHopf.set_corr_grid), against r and b of the fp64
oracle (the normal equations of oracle.blah2_oracle.wiener_hopf).

Every geometry of corr_crafted.GEOMS: one handle with the transform length and the correlation form forced and read back
(fft_len, seg_len, nBins, plan_info), estimation only (estimate_dev_fmt with the stepwise solve, process_multi_dev without
output planes), r and b through read_last, at each of the geometry's grids: the per-channel call on FMT_C32, FMT_I16 and
FMT_I8 (half-window: the PAIR instantiation), the shared-reference call on FMT_C32 and FMT_I8 with 1, 2, 3 and 4 channels
(<true, 1>; + <false, 1>; + <false, 2>; + <false, 2> and <false, 1>).  Batches of 2 or 3 distinct CPIs at stride N + 37, the
gaps and a row in front of and behind the planes filled with 77s in every format.  Gates, per CPI and channel:

    max_k |r - r_ref| <= 1e-5 r_ref[0],      max_k |b_c - b_ref| <= 1e-5 sqrt(r_ref[0] sum |y_c|^2)  (Cauchy-Schwarz).

Every planted product is at least 8.1e-3 of its normaliser, and each of thirteen ways to lose, double or misplace one moves
r or some b_c by 4.4e3 gates or more (tests/test_corr_crafted_model.py).  Also asserted: the grid that ran
(WienerHopf.last_corr_grid, BLAH2HIP_CLUTTER_INFO_CORR_GRID) is the forced one (plan_info()['corr_grid']), or the planner's as computed from the device's CU count; through the
restated walks, that some workgroup walked 5 or 6 segments where the geometry is about walking; the formats' r and b are
equal bit for bit; the flags' guard words and the input planes are untouched.  One more case runs on the planner's own path:
64 CPIs of 100 half-window segments, where clutter_grids itself leaves fewer workgroups than segments.

Measured on the MI355X (FIGURES below), worst err / normaliser over this file per kernel form and transform length, r | b:
half-window 4.7e-8 | 5.2e-8 at F = 1024, 1.5e-8 | 1.9e-8 at 2048, 4.7e-8 | 3.1e-8 at 4096; windowed 7.0e-8 | 7.4e-8 at 1024,
2.9e-8 | 2.5e-8 at 2048, 2.7e-8 | 3.4e-8 at 4096; the batch of 64 on the planner's grid of 32 (runs of 4 segments) 2.0e-8 |
1.9e-8.  The worst case is 135 times inside the gate; the three sample formats gave equal bits everywhere.  Nothing was found:
the kernels are unchanged.

Every case prints its worst figures."""
import numpy as np
import pytest

import corr_crafted as CC

pytestmark = pytest.mark.gpu

# worst (err r / r_ref[0], err b / its normaliser) per form and transform length, MI355X; a record of what was measured,
# not a bound: every case is held to 1e-5
FIGURES = {("half", 1024): (4.669e-08, 5.202e-08), ("half", 2048): (1.517e-08, 1.907e-08), ("half", 4096): (4.656e-08, 3.064e-08),
           ("window", 1024): (6.959e-08, 7.370e-08), ("window", 2048): (2.857e-08, 2.500e-08), ("window", 4096): (2.682e-08, 3.354e-08)}

_worst = {}


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


@pytest.fixture(scope="module")
def num_cu(b2):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def guarded(torch, shape, dtype, pad=64):
    words = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size() // 4
    whole = torch.full((words + pad,), int(CC.GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    return whole, whole[:words].view(dtype).view(shape)


def guard_intact(whole, pad=64):
    return bool((whole[-pad:].cpu().numpy().view(np.uint32) == CC.GUARD).all())


class Planes:
    """One format's device planes: pointers of the first CPI of x and of every y_c, and the host copies."""

    def __init__(self, torch, fmt_name, x, ys):
        self.host, self.stride = CC.host_planes(fmt_name, x, ys)
        self.dev = [torch.from_numpy(h).cuda() for h in self.host]
        row = [h.itemsize * (h.size // h.shape[0]) for h in self.host]
        self.px = self.dev[0].data_ptr() + row[0]
        self.pys = [None] if fmt_name == "FMT_I16" else [d.data_ptr() + rb for d, rb in zip(self.dev[1:], row[1:])]

    def untouched(self):
        return all(np.array_equal(d.cpu().numpy(), h) for d, h in zip(self.dev, self.host))


def handle(b2, g, batch=None):
    wh = b2.WienerHopf(g.dmin, g.dmin + g.n_bins, g.N, max_batch=batch or g.B)
    wh.set_fft_len(g.F)
    wh.set_corr_form(g.form)
    wh.set_fir_carry(g.carry)
    wh.set_solve_form("stepwise")
    wh._refresh_dims()
    info = wh.plan_info()
    assert (wh.nBins, wh.fft_len, wh.seg_len) == (g.n_bins, g.F, CC.seg_len_of(g)), g.name
    assert info["corr"] == g.form and info["carry"] == g.carry and info["chunks"] == 0 and info["corr_grid"] == 0
    assert wh.last_corr_grid() == 0
    return wh


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def gate(g, tag, c_ref, ch, r, b):
    """One CPI and channel against the oracle; prints before it asserts.  Returns (err r / r0, err b / normaliser)."""
    r_ref, b_ref = CC.oracle_rb(g, c_ref, ch)
    r0, bn = CC.normalisers(g, c_ref, ch)
    assert np.isfinite(r.view(np.float64)).all() and np.isfinite(b.view(np.float64)).all(), (g.name, tag)
    er, eb = np.max(np.abs(r - r_ref)) / r0, np.max(np.abs(b - b_ref)) / bn
    key = (g.form, g.F)
    w = _worst.setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], er), max(w[1], eb)
    if er > CC.R_TOL or eb > CC.B_TOL:
        print(f"\n[corr census {g.name} {tag} cpi {c_ref} ch {ch}] r {er:.3e} (lag {np.argmax(np.abs(r - r_ref))})  "
              f"b {eb:.3e} (lag {np.argmax(np.abs(b - b_ref))})")
    assert er <= CC.R_TOL, (g.name, tag, c_ref, ch, "r", er)
    assert eb <= CC.B_TOL, (g.name, tag, c_ref, ch, "b", eb)
    return er, eb


def run_single(torch, b2, wh, pl, fmt_name, B):
    wo, ok = guarded(torch, (B,), torch.int32)
    wh.estimate_dev_fmt(getattr(b2, fmt_name), pl.px, pl.pys[0], B, pl.stride, ok.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert guard_intact(wo)
    return wh.last_corr_grid()


def run_multi(torch, b2, wh, pl, fmt_name, B, K):
    wo, ok = guarded(torch, (K, B), torch.int32)
    wh.process_multi_dev(getattr(b2, fmt_name), pl.px, pl.pys[:K], B, pl.stride, None, 0, ok.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert guard_intact(wo)
    return wh.last_corr_grid()


@pytest.mark.parametrize("g", CC.GEOMS, ids=lambda g: g.name)
def test_census(b2, num_cu, g):
    import torch
    cs = CC.census_for(g)
    B = g.B
    wh = handle(b2, g)
    planes = {f: Planes(torch, f, cs.x, cs.ys) for f in ("FMT_C32", "FMT_I16", "FMT_I8")}
    worst = [0.0, 0.0]
    for i, forced in enumerate(g.grids):
        want = forced or CC.planner_grid(g, num_cu, B)
        assert want <= CC.plan_jobs(g, num_cu)
        wh.set_corr_grid(forced)
        assert wh.plan_info()["corr_grid"] == forced
        walks = CC.walks_of(g, want)
        assert sorted(s for w in walks for s in w) == list(range(CC.cdiv(g.N, g.F // 2 if g.form == "half" else CC.seg_len_of(g))))
        if g.walk and i == 0:
            assert max(map(len, walks)) == g.walk >= 3, (g.name, want)
        tag = f"grid {want}{'' if forced else ' (planner)'}"
        # the per-channel call
        single = {}
        for f in ("FMT_C32", "FMT_I16", "FMT_I8"):
            assert run_single(torch, b2, wh, planes[f], f, B) == want, (g.name, tag, f)
            single[f] = [wh.read_last(c) for c in range(B)]
            for c in range(B):
                e = gate(g, f"{tag} single {f}", c, 0, single[f][c][2], single[f][c][3])
                worst = [max(worst[0], e[0]), max(worst[1], e[1])]
        for f in ("FMT_I16", "FMT_I8"):
            for c in range(B):
                for which in (2, 3):
                    assert np.array_equal(bits(single[f][c][which]), bits(single["FMT_C32"][c][which])), (g.name, tag, f, c, "rb"[which - 2])
        # one reference, K channels
        for K in (1, 2, 3, 4):
            multi = {}
            for f in ("FMT_C32", "FMT_I8"):
                assert run_multi(torch, b2, wh, planes[f], f, B, K) == want, (g.name, tag, f, K)
                multi[f] = [[wh.read_last(k * B + c) for c in range(B)] for k in range(K)]
                for k in range(K):
                    for c in range(B):
                        e = gate(g, f"{tag} multi K={K} {f}", c, k, multi[f][k][c][2], multi[f][k][c][3])
                        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
            for k in range(K):
                for c in range(B):
                    for which in (2, 3):
                        assert np.array_equal(bits(multi["FMT_I8"][k][c][which]), bits(multi["FMT_C32"][k][c][which])), (g.name, tag, K, k, c)
    assert all(p.untouched() for p in planes.values()), "an input plane was written"
    wh.close()
    print(f"\n[corr census {g.name}] grids {g.grids}: worst err r / r0 {worst[0]:.3e}, err b / normaliser {worst[1]:.3e}")


def test_planner_shrinks_the_grid_below_the_segments(b2, num_cu):
    """The option off: a batch of 64 CPIs of 100 half-window segments, where clutter_grids leaves fewer workgroups per CPI
    than segments.  The first, the middle and the last CPI are census CPIs 0, 1 and 2 of the geometry and are checked; every
    other CPI is census CPI 3, so a workgroup that reads a neighbour's samples is seen."""
    import torch
    g = CC.BATCH_GEOM
    n_cpi = CC.BATCH_CPIS
    cs = CC.census_for(g)
    which = np.full(n_cpi, 3)
    which[0], which[n_cpi // 2], which[-1] = 0, 1, 2
    wh = handle(b2, g, batch=n_cpi)
    want = CC.planner_grid(g, num_cu, n_cpi)
    per, runs = CC.half_walks(g.N, g.F, want)
    assert want < len([s for r in runs for s in r]) == 100
    x, ys = cs.x[which], cs.ys[which]
    for f, K in (("FMT_C32", 0), ("FMT_I8", 3)):
        pl = Planes(torch, f, x, ys)
        if K:
            assert run_multi(torch, b2, wh, pl, f, n_cpi, K) == want
        else:
            assert run_single(torch, b2, wh, pl, f, n_cpi) == want
        grid = wh.last_corr_grid()
        assert wh.plan_info()["corr_grid"] == 0
        assert max(map(len, CC.half_walks(g.N, g.F, grid)[1])) >= 3, grid
        worst = [0.0, 0.0]
        for c in (0, n_cpi // 2, n_cpi - 1):
            for k in range(max(K, 1)):
                _, _, r, b = wh.read_last(k * n_cpi + c)
                e = gate(g, f"batch {n_cpi} {f} K={K}", int(which[c]), k, r, b)
                worst = [max(worst[0], e[0]), max(worst[1], e[1])]
        assert pl.untouched()
        print(f"\n[corr census {g.name} {f} K={K}] grid {grid}, per {per}: worst err r / r0 {worst[0]:.3e}, err b / normaliser {worst[1]:.3e}")
    wh.close()


def test_grid_option(b2, num_cu):
    """BLAH2HIP_CLUTTER_OPT_CORR_GRID: what it refuses, what it reports, that 0 and the planner's own value forced are the same
    bits, that a forced multi call followed by the option at 0 runs (the partials are sized for both), that a re-plan returns
    to 0, that a handle with blocks forwards it and a long filter refuses it."""
    import torch
    g = CC.BY_NAME["win1024_110taps_40seg"]
    cs = CC.census_for(g)
    jobs = CC.plan_jobs(g, num_cu)
    assert jobs == 40
    wh = handle(b2, g)
    for bad in (-8, 4, 12, jobs + 8, 1 << 40):
        with pytest.raises(b2.Blah2HipError) as e:
            wh.set_corr_grid(bad)
        assert f"from 8 to {jobs}" in str(e.value), str(e.value)
    pl = Planes(torch, "FMT_C32", cs.x, cs.ys)
    natural = CC.planner_grid(g, num_cu, g.B)
    assert run_single(torch, b2, wh, pl, "FMT_C32", g.B) == natural
    ref = [wh.read_last(c) for c in range(g.B)]
    wh.set_corr_grid(natural)
    assert run_single(torch, b2, wh, pl, "FMT_C32", g.B) == natural
    for c in range(g.B):
        for which in (2, 3):
            assert np.array_equal(bits(wh.read_last(c)[which]), bits(ref[c][which]))
    # multi: planner's grid, forced to the plan's whole count (more partials than the planner's launch), back to 0
    assert run_multi(torch, b2, wh, pl, "FMT_C32", g.B, 3) == natural
    mref = [wh.read_last(v) for v in range(3 * g.B)]
    for forced in (8, jobs, 0):
        wh.set_corr_grid(forced)
        assert run_multi(torch, b2, wh, pl, "FMT_C32", g.B, 3) == (forced or natural)
        for v in range(3 * g.B):
            gate(g, f"option multi grid {forced}", v % g.B, v // g.B, *wh.read_last(v)[2:])
    for v in range(3 * g.B):
        for which in (2, 3):
            assert np.array_equal(bits(wh.read_last(v)[which]), bits(mref[v][which]))
    wh.set_corr_grid(8)
    assert wh.plan_info()["corr_grid"] == 8
    wh.set_fft_len(2048)  # re-plans: 19 segments, 24 workgroups
    assert wh.plan_info()["corr_grid"] == 0
    assert run_single(torch, b2, wh, pl, "FMT_C32", g.B) == 24
    wh.close()
    # blocks: the option is the child's (4 blocks of 9990 samples: 11 segments of 915, 16 workgroups per virtual CPI)
    wb = b2.WienerHopf(0, 110, 4 * 9990, max_batch=1, blocks=4)
    wb.set_fft_len(1024)
    with pytest.raises(b2.Blah2HipError) as e:
        wb.set_corr_grid(24)
    assert "from 8 to 16" in str(e.value)
    wb.set_corr_grid(8)
    wb.close()
    wl = b2.WienerHopf(0, 5000, 20_000)
    with pytest.raises(b2.Blah2HipError):
        wl.set_corr_grid(8)
    wl.close()


def test_zz_figures():
    """Prints this run's worst figures per kernel form and transform length; FIGURES has a record for each."""
    for key in sorted(_worst):
        print(f"\n[corr census worst {key[0]} F={key[1]}] err r / r0 {_worst[key][0]:.3e}, err b / normaliser {_worst[key][1]:.3e}")
    assert all(v[0] <= CC.R_TOL and v[1] <= CC.B_TOL for v in _worst.values())
    assert set(FIGURES) >= set(_worst)
