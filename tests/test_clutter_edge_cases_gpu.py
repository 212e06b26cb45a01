"""GPU: the clutter filter's lag window at its edge geometries, every CPI against the fp64 oracle.

tests/test_edge_cases_gpu.py sweeps the ambiguity engine's geometries; this is the same for the Wiener-Hopf filter, whose
index arithmetic depends on delayMin everywhere: XsMap / xs_index (the reference's uint32 evaluation of
xs[i] = x[(i - delayMin) mod N]: for a positive delayMin the first delayMin samples come from (2^32 - delayMin) mod N, not
from N - delayMin), xs_window_plain (one buffer-descriptor run or the element-by-element window), the wrap-around pairs of
the last correlation job, load_half under the FIR's carried overlap, long_plane_kernel with dmin, and the _multi kernels.

Every case: B distinct int16-valued CPIs with clutter inside the lag window (tests/clutter_crafted.py), the plan forced
and read back from the handle, process_dev_fmt into guarded planes of stride n + 3, then per CPI
    max|r - r_ref| / |r_ref[0]| <= 1e-5,  max|b - b_ref| / max|b_ref| <= 1e-5,  max|yf - y_ref| / max|y_ref| <= 1e-4
(the gates of tests/test_clutter_gpu.py), ok == 1, guards and gaps intact; FMT_I16 equals FMT_C32 bit for bit (int16 ->
fp32 is exact); where marked, the int8 planes equal the int16 words of the same clipped values bit for bit.

What is unreachable by design and asserted as such: the carried FIR overlap exists only where F - nBins + 1 lies in
[F/2, F/2 + F/64], so "carry" is asserted through the plan (segLen = F/2) and rows outside that band do not ask for it;
the long form has one plan and refuses every option.

Measured on an MI355X, worst over the CPIs, formats and plans of a geometry (r, b, yf; gates 1e-5, 1e-5, 1e-4):
    (1, 2, 3001) 6.5e-8 8.5e-8 5.7e-8     (0, 1, 3001) 6.7e-8 9.3e-8 4.5e-7        (-1, 0, 3001) 7.0e-8 7.2e-8 4.2e-8
    (3, 40, 41) 7.6e-8 1.6e-7 1.1e-6      (3, 40, 600) 1.5e-7 1.3e-7 1.4e-7        (3, 40, 16384) 7.8e-8 8.7e-8 9.5e-8
    (3, 40, 20011) 8.1e-8 8.4e-8 1.2e-7   (700, 1000, 20011) 1.1e-7 1.2e-7 1.3e-7  (1500, 2515, 40003) 8.7e-8 8.6e-8 1.1e-7
    (2500, 4547, 30011) 8.6e-8 1.1e-7 1.3e-7   (-3000, -2600, 20011) 7.2e-8 9.1e-8 1.1e-7   (-1500, 547, 60001) 9.0e-8 1.1e-7 1.7e-7
    (4999, 5010, 5000) 7.2e-8 2.2e-7 5.7e-8    (-4999, -4990, 5000) 7.7e-8 9.2e-8 9.2e-8    (5, 4615, 60000) 9.8e-8 1.0e-7 1.6e-7
    K = 2 channels: 7.7e-8 9.7e-8 1.0e-7"""
import numpy as np
import pytest

import clutter_crafted as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


def geometry_case(b2, dmin, dmax, n, B, corr_form, fft_len, carry, i8, tag):
    """FMT_C32 and FMT_I16 (and FMT_I8 on the clipped samples) of one geometry and plan.  Returns the FMT_C32 run."""
    key = (dmin, dmax, n, B, False)
    chans = cc.cpis_for(dmin, dmax, n, B)
    wh = cc.planned(b2, dmin, dmax, n, B, corr_form, fft_len, carry)
    run32 = cc.run_filter(b2, wh, b2.FMT_C32, chans)
    cc.check_oracle(run32, chans, key, dmin, dmax, (tag, "c32"))
    run16 = cc.run_filter(b2, cc.planned(b2, dmin, dmax, n, B, corr_form, fft_len, carry), b2.FMT_I16, chans)
    cc.assert_same_bits(run32, run16, (tag, "i16 == c32"))
    cc.check_oracle(run16, chans, key, dmin, dmax, (tag, "i16"))
    if i8:
        key8 = (dmin, dmax, n, B, True)
        chans8 = cc.cpis_for(dmin, dmax, n, B, i8=True)
        r16 = cc.run_filter(b2, wh, b2.FMT_I16, chans8)
        r8 = cc.run_filter(b2, cc.planned(b2, dmin, dmax, n, B, corr_form, fft_len, carry), b2.FMT_I8, chans8)
        cc.assert_same_bits(r16, r8, (tag, "i8 == i16"))
        cc.check_oracle(r8, chans8, key8, dmin, dmax, (tag, "i8"))
    return run32


# (dmin, dmax, n), B, i8, [(corr_form, fft_len, carry)]; None = the planner's choice
W, H = "window", "half"
ROWS = [
    ((1, 2, 3001), 2, False, [(W, None, None), (H, None, None)]),       # one tap: nBins = 1, no wrap-around product, history 0
    ((0, 1, 3001), 2, False, [(W, None, None), (H, None, None)]),
    ((-1, 0, 3001), 2, False, [(W, None, None), (H, None, None)]),
    ((3, 40, 41), 3, False, [(W, None, None), (H, None, None)]),        # n barely above the taps: almost every pair wraps
    ((3, 40, 600), 3, True, [(W, None, None), (H, None, None), (W, 2048, None)]),  # a CPI shorter than one transform
    ((3, 40, 16384), 3, False, [(W, None, None), (H, None, None)]),     # 2^32 mod N = 0: wrapC is the plain roll
    ((3, 40, 20011), 3, True, [(W, None, None), (H, None, None)]),      # ... beside an N where it is not
    ((700, 1000, 20011), 2, True, [(c, F, None) for F in (1024, 2048, 4096) for c in (W, H)]),  # shift > F/2: whole head windows on the element path
    ((2500, 4547, 30011), 2, False, [(None, 4096, True)]),              # 2047 taps, F = 4096, carry, shift > a block
    ((-3000, -2600, 20011), 2, False, [(W, None, None), (H, None, None)]),  # negative lags only, shift > F: whole tail windows wrap
    ((4999, 5010, 5000), 2, False, [(W, None, None), (H, None, None)]),  # the largest shift the constructor accepts
    ((-4999, -4990, 5000), 2, False, [(W, None, None), (H, None, None)]),
]
CASES = [(g, B, i8, v) for g, B, i8, vs in ROWS for v in vs]


def case_id(c):
    (dmin, dmax, n), B, i8, (corr, F, carry) = c
    return f"{dmin}_{dmax}_{n}-{corr or 'auto'}-F{F or 'auto'}" + ("-carry" if carry else "")


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_geometry_against_the_oracle(b2, case):
    (dmin, dmax, n), B, i8, (corr, F, carry) = case
    geometry_case(b2, dmin, dmax, n, B, corr, F, carry, i8, case_id(case))


# the carried overlap on and off (tests/test_clutter_gpu.py::test_fir_carries_the_window_overlap, and its bounds)
@pytest.mark.parametrize("dmin,dmax,n,F", [(1500, 2515, 40003, 2048),   # 1015 taps: the carried half crosses from element-path windows into plain ones
                                           (-1500, 547, 60001, 4096)],  # 2047 taps with a large negative shift
                         ids=["1500_2515_40003-F2048", "-1500_547_60001-F4096"])
def test_carried_overlap_on_and_off(b2, dmin, dmax, n, F):
    B = 2
    tag = f"{dmin}_{dmax}_{n}"
    on = geometry_case(b2, dmin, dmax, n, B, None, F, True, False, tag + "-carry")
    off = geometry_case(b2, dmin, dmax, n, B, None, F, False, False, tag + "-whole")
    chans = cc.cpis_for(dmin, dmax, n, B)
    for c in range(B):
        y_ref = cc.oracle_for((dmin, dmax, n, B, False), c, chans[c][0], chans[c][1], dmin, dmax)[1]
        w_on, w_off = on[2][c][1], off[2][c][1]
        assert np.max(np.abs(w_on - w_off)) <= 1e-5 * np.max(np.abs(w_off))
        d = cc.as_c128(on[0], n)[c] - cc.as_c128(off[0], n)[c]
        assert np.max(np.abs(d)) / np.max(np.abs(y_ref)) <= 2e-5


def test_long_form_with_a_positive_first_lag(b2):
    """4610 taps from lag 5: three chunks on child handles, long_plane_kernel<1> / <2> with dmin > 0.  fp32 planes only,
    one plan: every option is refused."""
    dmin, dmax, n, B = 5, 4615, 60000, 1
    chans = cc.cpis_for(dmin, dmax, n, B)
    wh = b2.WienerHopf(dmin, dmax, n, max_batch=B)
    assert wh.plan_info()["chunks"] == 3 and wh.fft_len == 4096 and wh.nBins == 4610
    with pytest.raises(b2.Blah2HipError) as e:
        wh.set_corr_form("half")
    assert e.value.code == b2._lib.ERR_UNSUPPORTED
    run = cc.run_filter(b2, wh, b2.FMT_C32, chans)
    cc.check_oracle(run, chans, (dmin, dmax, n, B, False), dmin, dmax, "5_4615_60000-long")
    wh.close()


def test_refusals_write_nothing(b2):
    import torch
    whole, out = cc.guarded(torch, (2, 1003), torch.complex64)
    for args in ((5000, 5010, 5000), (-5000, -4990, 5000),  # |delayMin| == n
                 (7, 7, 5000), (7, 3, 5000),                # delayMax <= delayMin
                 (0, 42, 41), (-3, 600, 600)):              # more taps than samples
        with pytest.raises(b2.Blah2HipError) as e:
            b2.WienerHopf(*args)
        assert e.value.code == b2._lib.ERR_INVALID, (args, str(e.value))
    torch.cuda.synchronize()
    assert (whole.cpu().numpy().view(np.uint32) == cc.GUARD).all()
    del out


def channel_sets(dmin, dmax, n, B):
    """K = 2 surveillance channels per reference: channel 0 is the harness's y; channel 1 has the same reference (the same
    seed draws the same x) with its own direct-path gain and its own echoes."""
    from oracle import blah2_oracle as O
    base = cc.cpis_for(dmin, dmax, n, B)
    t1 = tuple((d + 1 if abs(d + 1) < n else d, f - 25.0, a * 0.7) for d, f, a in cc.echo_delays(dmin, dmax, n))
    second = []
    for c in range(B):
        x2, y2 = O.synth_iq(n, seed=7000 + 131 * c + n % 97 + (dmax - dmin), fs=cc.FS, targets=t1, direct=-0.5)
        assert np.array_equal(x2, base[c][0])
        second.append((x2, y2))
    return [base, second]


@pytest.mark.parametrize("dmin,dmax,n", [(3, 40, 20011), (700, 1000, 20011), (-3000, -2600, 20011)])
def test_several_channels_share_the_estimate(b2, dmin, dmax, n):
    """process_multi_dev, K = 2, B = 2: each channel is the single-channel call's bits (both handles on the stepwise solve,
    as tests/test_multi_clutter_gpu.py) and passes the oracle gates."""
    import torch
    K, B = 2, 2
    sets = channel_sets(dmin, dmax, n, B)
    assert not np.array_equal(sets[0][0][1], sets[1][0][1])
    st = torch.cuda.current_stream().cuda_stream
    dx, dy0, stride = cc.device_inputs(torch, b2, b2.FMT_C32, sets[0])
    _, dy1, _ = cc.device_inputs(torch, b2, b2.FMT_C32, sets[1])
    wh = cc.planned(b2, dmin, dmax, n, B, solve="stepwise")
    keep = [cc.guarded(torch, (B, n + cc.GAP), torch.complex64) for _ in range(K)]
    wo, ok = cc.guarded(torch, (K, B), torch.int32)
    wh.process_multi_dev(b2.FMT_C32, dx.data_ptr(), [dy0.data_ptr(), dy1.data_ptr()], B, stride, [o.data_ptr() for _, o in keep],
                         n + cc.GAP, ok.data_ptr(), st)
    torch.cuda.synchronize()
    assert all(cc.guard_intact(w) for w, _ in keep) and cc.guard_intact(wo)
    assert wh.solve_info()["form"] == b2._lib.CLUTTER_SOLVE_STEPWISE
    okv = ok.cpu().numpy()
    assert okv.tolist() == [[1] * B] * K
    reads = [wh.read_last(v) for v in range(K * B)]
    wh1 = cc.planned(b2, dmin, dmax, n, B, solve="stepwise")
    assert (wh1.fft_len, wh1.plan_info()) == (wh.fft_len, wh.plan_info())
    for k in range(K):
        words = keep[k][1].cpu().numpy().view(np.uint32).reshape(B, n + cc.GAP, 2)
        assert (words[:, n:] == cc.GUARD).all()
        multi = (words, okv[k], reads[k * B:(k + 1) * B])
        single = cc.run_filter(b2, wh1, b2.FMT_C32, sets[k])
        cc.assert_same_bits(multi, single, (dmin, dmax, n, "channel", k))
        cc.check_oracle(multi, sets[k], (dmin, dmax, n, B, "channel", k), dmin, dmax, (f"{dmin}_{dmax}_{n}-multi", k))
    assert not np.array_equal(cc.bits(reads[0][1]), cc.bits(reads[B][1]))  # the channels' taps differ


def test_a_failed_cpi_inside_a_shifted_batch(b2):
    """(700, 1000, 20011), B = 3, the reference of CPI 1 all zero: ok = [1, 0, 1]; process_dev_fmt passes the surveillance
    channel of the failed CPI through (WienerHopf.cpp:111-115); its neighbours pass the oracle gates."""
    dmin, dmax, n, B = 700, 1000, 20011, 3
    chans = cc.cpis_for(dmin, dmax, n, B, zero_ref=(1,))
    key = (dmin, dmax, n, B, "zero-ref-1")
    runs = {}
    for name, fmt in (("c32", b2.FMT_C32), ("i16", b2.FMT_I16)):
        run = cc.run_filter(b2, cc.planned(b2, dmin, dmax, n, B), fmt, chans)
        assert run[1].tolist() == [1, 0, 1], name
        assert not run[2][1][0]
        assert np.array_equal(cc.as_c128(run[0], n)[1], chans[1][1]), name
        cc.check_oracle(run, chans, key, dmin, dmax, ("700_1000_20011-failed-cpi", name), cpis=(0, 2))
        runs[name] = run
    cc.assert_same_bits(runs["c32"], runs["i16"], "failed CPI: i16 == c32")


def test_relaunch_leaves_no_state(b2):
    """(1500, 2515, 40003) three times on one handle: the carry registers and the partial buffers leak nothing."""
    dmin, dmax, n, B = 1500, 2515, 40003, 2
    chans = cc.cpis_for(dmin, dmax, n, B)
    wh = cc.planned(b2, dmin, dmax, n, B, None, 2048, True)
    runs = cc.run_filter(b2, wh, b2.FMT_C32, chans, reps=3)
    cc.check_oracle(runs[0], chans, (dmin, dmax, n, B, False), dmin, dmax, "1500_2515_40003-relaunch")
    for again in runs[1:]:
        cc.assert_same_bits(runs[0], again, "relaunch")
