"""GPU: the range kernels on crafted pulses (tests/range_crafted.py) against the fp64 oracle.

Part 1, the range stage.  Every row of range_crafted.GEOMS -- windows that exactly fill the transform, the thresholds of the
kernel variants met with equality and missed by one, 449 lags on segments of 576 samples (REUSE without OUT7) -- and one
window in three lag chunks, through every range kernel of its transform length, forced and asserted: three distinct census
CPIs in one call, planes with gaps of 77s between the CPIs, guarded output buffers, the Doppler kernel forced to the direct
one, hot columns and leak compensation off.  The one-wave kernels run on ONE workgroup, so that a wave walks from a CPI's
last pulse into the next CPI's first.  Gate: max|M - ref| <= 1e-5 max|ref| (PEAK_TOL of tests/test_timed_kernels_gpu.py);
every planted product is at least 1e-3 of the peak (tests/test_range_crafted_model.py), so one lost, extra or misplaced
sample misses the gate by 100 times.  Map::set_metrics is not compared: most cells of a census map are rounding noise in
both implementations (as in tests/test_edge_cases_gpu.py).

Part 2, the Doppler rows.  A census of ONE populated pulse gives every column the same modulus in all nD rows, so the peak
gate holds every row of the strongest columns to 1e-5 of itself; every Doppler kernel that covers the length is forced and
asserted.  Finding (MI355X): every kernel holds 1e-5 on every CPI whose populated pulse is not pulse 0 (worst 6.6e-7).  The
CPI whose ONLY populated pulse is pulse 0 misses it from nD = 512 on, in every kernel alike, in the zero-Doppler row first:
the kernels subtract the first pulse's value r0 from a column before the transform and add nD r0 back to bin 0 (DESIGN.md
section 3), which turns this column into nD - 1 rows of -r0 whose fp32 sum, nD times the size of the result, cancels down
to it -- err / peak = 4.2e-5 at 513, 8.5e-5 at 1025, 1.7e-4 at 2049 for the transforms (0.8e-7 nD), about half that for
the direct kernel's blocked sum (5.2e-4 at 2049 while it was one running sum).  That is the fp32 floor of the form on an input it was not chosen for, not a wrong row:
FIRST_PULSE_MEASURED records the figure of every (nD, kernel) and that one CPI is held to twice it; all other CPIs, and
nD = 65 throughout, stay at 1e-5.

Every case prints its worst err / peak."""
import numpy as np
import pytest

import range_crafted as RC
from oracle import blah2_oracle as O
from test_timed_kernels_gpu import PEAK_TOL

pytestmark = pytest.mark.gpu

assert PEAK_TOL == 1e-5
GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces
B = 3                          # CPIs per call
SEEDS = (11, 12, 13)
_cache = {}


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


def guarded(torch, shape, dtype, pad=64):
    words = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size() // 4
    whole = torch.full((words + pad,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    return whole, whole[:words].view(dtype).view(shape)


def guard_intact(whole, pad=64):
    return bool((whole[-pad:].cpu().numpy().view(np.uint32) == GUARD).all())


def upload(torch, host):
    """(keep-alive tensor, pointer) of a host plane; (None, None) for the plane FMT_I16 does not have."""
    if host is None:
        return None, None
    t = torch.from_numpy(host).cuda()
    return t, t.data_ptr()


def census_case(g):
    """(dims, [x per CPI], [y per CPI], [ref per CPI]) of a table row: three CPIs with seeds of their own."""
    if g.name not in _cache:
        d = RC.dims_of(g)
        xy = [RC.census(d, g.n_seg, g.seg_len, s, extra_cols=RC.extra_cols_of(g)) for s in SEEDS]
        xs, ys = [c[0] for c in xy], [c[1] for c in xy]
        _cache[g.name] = (d, xs, ys, [RC.reference(d, x, y) for x, y in zip(xs, ys)])
    return _cache[g.name]


def multi_case(g, K):
    """One reference and K surveillance channels per CPI, every channel a census of its own amplitudes:
    (dims, xs[c], ys[k][c], refs[k][c])."""
    if ("multi", g.name, K) not in _cache:
        d = RC.dims_of(g)
        xs = [RC.census(d, g.n_seg, g.seg_len, s)[0] for s in SEEDS]
        ys = [[RC.census(d, g.n_seg, g.seg_len, 100 * (k + 1) + s)[1] for s in SEEDS] for k in range(K)]
        refs = [[RC.reference(d, xs[c], ys[k][c]) for c in range(B)] for k in range(K)]
        _cache[("multi", g.name, K)] = (d, xs, ys, refs)
    return _cache[("multi", g.name, K)]


def engine(b2, g, kernel, max_batch=B, hot="off", leak="off"):
    from blah2_amd import _lib
    amb = b2.Ambiguity(*RC.args_of(g), True, max_batch=max_batch)
    amb.set_fft_len(g.fft_len)
    assert (amb.dims.fft_len, amb.dims.n_seg, amb.dims.seg_len) == (g.fft_len, g.n_seg, g.seg_len), g.name
    assert (amb.get_n_doppler_bins(), amb.get_n_corr(), amb.get_n_delay_bins()) == (5, g.n_corr, g.delay_max - g.delay_min + 1)
    if kernel != _lib.RANGE_SHARED:
        amb.set_range_kernel(kernel)
    if kernel in (_lib.RANGE_WAVE1K, _lib.RANGE_WAVE, _lib.RANGE_SHARED):
        amb.set_range_grid(1)  # one workgroup: its waves walk on from a CPI's last pulse into the next CPI
    amb.set_doppler_kernel("direct")
    amb.set_hot_columns(hot)
    amb.set_leak_compensation(leak)
    return amb


def gate(got, refs, tag, tol=PEAK_TOL):
    """The peak gate on every CPI; prints every CPI's err / peak before it asserts and returns the worst."""
    ratios, where = [], []
    for c, ref in enumerate(refs):
        m = got[c].astype(np.complex128)
        assert np.isfinite(m.view(np.float64)).all(), f"{tag} cpi {c}: NaN or Inf in the map"
        err = np.abs(m - ref)
        ratios.append(float(err.max() / np.abs(ref).max()))
        where.append(tuple(int(v) for v in np.unravel_index(np.argmax(err), err.shape)))
    print(f"\n[{tag}] worst err / peak {max(ratios):.3e} (gate {tol:.3e}); per CPI " + " ".join(f"{r:.3e}" for r in ratios))
    for c, r in enumerate(ratios):
        assert r <= tol, f"{tag} cpi {c}: err / peak {r:.3e} > {tol:.3e} at (row, column) {where[c]}"
    return max(ratios)


def run_single(b2, amb, fmt_name, xs, ys, stride):
    import torch
    from blah2_amd import _lib
    hx, hy = RC.host_planes(fmt_name, xs, ys, stride)
    tx, px = upload(torch, hx)
    ty, py = upload(torch, hy)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    whole, out = guarded(torch, (len(xs), nD, nC), torch.complex64)
    wm, met = guarded(torch, (len(xs), 2), torch.float64)
    amb.process_dev(getattr(b2, fmt_name), px, py, len(xs), stride, out.data_ptr(), met.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert guard_intact(whole) and guard_intact(wm)
    return out.cpu().numpy(), met.cpu().numpy(), amb.info(_lib.INFO_LAST_RANGE_KERNEL)


# ---- 1. the range stage -----------------------------------------------------------------------------------------------
KERNELS = {1024: ("RANGE_WAVE1K", "RANGE_PS", "RANGE_E8"), 2048: ("RANGE_WAVE", "RANGE_E16"), 4096: ("RANGE_E16",)}


def range_cases():
    out = []
    for g in RC.GEOMS + (RC.CHUNKED,):
        first = RC.FIRST_ROW[g.fft_len] == g.name
        for k in KERNELS[g.fft_len]:
            for f in RC.FORMATS if first else ("FMT_C32", "FMT_I8"):
                out.append(pytest.param(g.name, k, f, id=f"{g.name}-{k[6:].lower()}-{f[4:].lower()}"))
    return out


@pytest.mark.parametrize("name,kernel,fmt_name", range_cases())
def test_range_kernels_on_the_census(b2, name, kernel, fmt_name):
    from blah2_amd import _lib
    g = RC.GEOM_BY_NAME[name]
    d, xs, ys, refs = census_case(g)
    k = getattr(_lib, kernel)
    amb = engine(b2, g, k)
    got, _, rk = run_single(b2, amb, fmt_name, xs, ys, d.n_samples + RC.GAP)
    assert rk == k and amb.last_doppler_kernel() == "direct"
    gate(got, refs, f"{name} {kernel} {fmt_name} seg_len {amb.dims.seg_len} lags {amb.get_n_delay_bins()}")


def test_hot_columns_and_leak_compensation_on_a_sparse_map(b2):
    """The first row with both features forced on: the same map gate, and no NaN in map or metrics."""
    from blah2_amd import _lib
    g = RC.GEOM_BY_NAME[RC.FIRST_ROW[1024]]
    d, xs, ys, refs = census_case(g)
    for fmt_name in ("FMT_C32", "FMT_I8"):
        amb = engine(b2, g, _lib.RANGE_WAVE1K, hot="always", leak="always")
        got, met, rk = run_single(b2, amb, fmt_name, xs, ys, d.n_samples + RC.GAP)
        assert rk == _lib.RANGE_WAVE1K and amb.last_doppler_kernel() == "direct"
        print(f"\n[hot + leak always, {fmt_name}] metrics {met.tolist()}, hot columns {amb.hot_columns()}, leak {amb.leak_info()}")
        assert not np.isnan(met).any()
        gate(got, refs, f"{g.name} hot + leak always {fmt_name}")


F1K = [g.name for g in RC.GEOMS if g.fft_len == 1024]


@pytest.mark.parametrize("fmt_name", ["FMT_C32", "FMT_I8"])
@pytest.mark.parametrize("name", F1K)
def test_shared_reference_kernel_on_the_census(b2, name, fmt_name):
    """K = 3 channels, each with a census of its own, through process_multi_dev on the shared-reference kernel: a pair on
    rangew1k_shared_kernel plus the odd channel on rangew1k_kernel, both in the instantiation the geometry selects."""
    import torch
    from blah2_amd import _lib
    K = 3
    g = RC.GEOM_BY_NAME[name]
    d, xs, ys, refs = multi_case(g, K)
    stride = d.n_samples + RC.GAP
    amb = engine(b2, g, _lib.RANGE_SHARED, max_batch=K * B)
    amb.set_multi_surv_range("shared")
    keep = [upload(torch, RC.host_planes(fmt_name, xs, ys[k], stride)[i]) for k in range(K) for i in (0, 1)]
    px, pys = keep[0][1], [keep[2 * k + 1][1] for k in range(K)]
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    whole, out = guarded(torch, (K * B, nD, nC), torch.complex64)
    wm, met = guarded(torch, (K * B, 2), torch.float64)
    amb.process_multi_dev(getattr(b2, fmt_name), px, pys, B, stride, out.data_ptr(), met.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert guard_intact(whole) and guard_intact(wm)
    assert amb.info(_lib.INFO_LAST_RANGE_KERNEL) == _lib.RANGE_SHARED and amb.last_doppler_kernel() == "direct"
    got = out.cpu().numpy()
    for k in range(K):
        gate(got[k * B:(k + 1) * B], refs[k], f"{name} RANGE_SHARED {fmt_name} channel {k} seg_len {amb.dims.seg_len} lags {nC}")


@pytest.mark.parametrize("fmt_name", ["FMT_I16", "FMT_F16", "FMT_I16X_C32Y", "FMT_I8X_C32Y"])
def test_shared_reference_kernel_refuses_the_other_formats(b2, fmt_name):
    """The shared kernel is built for FMT_C32 and FMT_I8: forced, every other format is refused with ERR_UNSUPPORTED and
    the handle stays usable."""
    import torch
    from blah2_amd import _lib
    g = RC.GEOM_BY_NAME[RC.FIRST_ROW[1024]]
    d, xs, ys, refs = multi_case(g, 3)
    stride = d.n_samples + RC.GAP
    amb = engine(b2, g, _lib.RANGE_SHARED, max_batch=2 * B)
    amb.set_multi_surv_range("shared")
    hx, hy = RC.host_planes(fmt_name, xs, ys[0], stride)
    tx, px = upload(torch, hx)
    ty, py = upload(torch, hy if hy is not None else hx)
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(b2.Blah2HipError) as e:
        amb.process_multi_dev(getattr(b2, fmt_name), px, [py, py], B, stride, None, None, st)
    assert e.value.code == _lib.ERR_UNSUPPORTED, str(e.value)
    assert ("FMT_I16" if fmt_name == "FMT_I16" else "FMT_C32 and BLAH2HIP_FMT_I8") in str(e.value)
    got, _, rk = run_single(b2, amb, "FMT_C32", xs, ys[0], stride)
    assert rk not in (0, _lib.RANGE_SHARED)
    gate(got, refs[0], f"{g.name} after the refusal of {fmt_name}")


# ---- 2. the Doppler rows ----------------------------------------------------------------------------------------------
N_CORR, DELAYS = 40, (-3, 36)  # 40 delay bins: ragged for tiles of 8 and of 16 columns
# the engine's coverage rule (capi.hip doppler_kernel_applicable): the chirp-z transform length is the smallest of 1024,
# 2048, 4096 that is >= 2 nD - 2; tile8 / tile8k / tile16 / tile16wg / sub4 run on 1024 (nD <= 513), pfa513 at nD = 513
# alone, tilew on 2048 (nD <= 1025), tilew2 / tilew4 on 4096 (nD <= 2049), tilem on 2048 and 4096, column wherever a
# chirp-z length exists, direct everywhere
SHORT = ("tile8", "tile8k", "tile16", "tile16wg", "sub4", "column", "direct")
DOPPLER_KERNELS = {65: SHORT, 512: SHORT, 513: SHORT + ("pfa513",), 1025: ("tilew", "tilem", "column", "direct"),
                   2049: ("tilem", "tilew2", "tilew4", "column", "direct")}


def doppler_args(nD):
    """(constructor arguments, explicit bin count): fs = n, so the Doppler resolution is 1 Hz and limits -h .. h give
    2 h + 1 bins; the even length goes through n_doppler_bins."""
    n = nD * N_CORR + RC.TAIL
    h = nD // 2
    return (DELAYS[0], DELAYS[1], -h, h, n, n), (nD if nD % 2 == 0 else 0)


def doppler_case(nD):
    """One CPI per populated pulse i0."""
    if ("dop", nD) not in _cache:
        args, bins = doppler_args(nD)
        d = O.ambiguity_dims(*args, True, n_doppler_bins=bins)
        assert (d.n_doppler_bins, d.n_corr, d.n_delay_bins) == (nD, N_CORR, 40)
        i0s = sorted({0, 1, 63, 64, nD // 2, nD - 1})
        xy = [RC.census(d, 1, N_CORR, 500 + i0, pulses=[i0]) for i0 in i0s]
        xs, ys = [c[0] for c in xy], [c[1] for c in xy]
        refs = [RC.reference(d, x, y) for x, y in zip(xs, ys)]
        for ref in refs:  # constant modulus down every column
            mod = np.abs(ref)
            assert np.abs(mod - mod[0:1]).max() <= 1e-12 * mod.max()
        _cache[("dop", nD)] = (d, xs, ys, refs)
    return _cache[("dop", nD)]


# err / peak measured on the MI355X for the CPI whose only populated pulse is pulse 0, the kernels' DC reference (module
# docstring), where it exceeds PEAK_TOL; that CPI's bound is twice the figure (case-to-case spread)
FIRST_PULSE_MEASURED = {
    (512, "tile8"): 4.234e-05, (512, "tile8k"): 4.234e-05, (512, "tile16"): 4.234e-05, (512, "tile16wg"): 4.234e-05,
    (512, "sub4"): 4.234e-05, (512, "column"): 4.234e-05, (512, "direct"): 2.263e-05,
    (513, "tile8"): 4.225e-05, (513, "tile8k"): 2.991e-05, (513, "tile16"): 2.991e-05, (513, "tile16wg"): 4.225e-05,
    (513, "sub4"): 2.991e-05, (513, "column"): 4.225e-05, (513, "direct"): 2.726e-05, (513, "pfa513"): 4.234e-05,
    (1025, "tilew"): 5.854e-05, (1025, "tilem"): 8.472e-05, (1025, "column"): 8.472e-05, (1025, "direct"): 4.491e-05,
    (2049, "tilem"): 1.693e-04, (2049, "tilew2"): 1.693e-04, (2049, "tilew4"): 1.697e-04, (2049, "column"): 1.693e-04,
    (2049, "direct"): 8.505e-05,
}


@pytest.mark.parametrize("nD,kernel", [pytest.param(nD, k, id=f"{nD}-{k}") for nD in sorted(DOPPLER_KERNELS) for k in DOPPLER_KERNELS[nD]])
def test_doppler_kernels_on_one_pulse_census(b2, nD, kernel):
    d, xs, ys, refs = doppler_case(nD)
    args, bins = doppler_args(nD)
    amb = b2.Ambiguity(*args, True, max_batch=len(xs), n_doppler_bins=bins)
    assert (amb.get_n_doppler_bins(), amb.get_n_corr(), amb.get_n_delay_bins()) == (nD, N_CORR, 40)
    amb.set_doppler_kernel(kernel)
    amb.set_hot_columns("off")
    amb.set_leak_compensation("off")
    got, _, rk = run_single(b2, amb, "FMT_C32", xs, ys, d.n_samples + RC.GAP)
    assert amb.last_doppler_kernel() == kernel and rk != 0
    # CPI 0 is the one with pulse 0 populated (doppler_case sorts the pulses)
    first = 2 * FIRST_PULSE_MEASURED[(nD, kernel)] if (nD, kernel) in FIRST_PULSE_MEASURED else PEAK_TOL
    gate(got[:1], refs[:1], f"nD {nD} Doppler kernel {kernel}, pulse 0 populated", tol=first)
    gate(got[1:], refs[1:], f"nD {nD} Doppler kernel {kernel}, the other pulses")
