"""GPU: the fp64 transform of the delay columns under the map's tallest peaks (BLAH2HIP_OPT_HOT_COLUMNS, csrc/capi.hip).

The fp32 Doppler transform leaves up to 1.2e-7 of a column's peak in the other rows of that column; under a peak 1000x the
map's mean level -- a strong echo behind the clutter filter -- that is beyond north_star's 1e-4 on a mean-level cell
(tools/gpu_chain_split_diag.py).  The engine transforms such columns again in fp64.  Checked against the oracle
(Ambiguity.cpp:152-169 in fp64): the column's error with and without it, that no other cell moves, which columns are
picked, every Doppler kernel family, batches whose CPIs differ, echoes at the Dopplers where a sparse look at the range map is
blind (whole multiples of 8 bins, the zeros of earlier rules, the worst Doppler of today's rule from tests/test_hot_columns_model.py),
and what is left out when more columns qualify than the kernel rewrites (BLAH2HIP_INFO_HOT_COLUMNS_MISSED).
"""
import numpy as np
import pytest

from gates import map_cell_gate
from oracle import blah2_oracle as O
from test_hot_columns_model import worst_k

HOT_RATIO = 250.0

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


def echo_cpi(n, fs, seed, delay, doppler, amp=1.0, noise=0.02, direct=0.0):
    """x white; y = direct x + amp x(t - delay) e^{2 pi i doppler t} + noise: one echo far above the floor."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 200.0
    t = np.arange(n) / fs
    xd = np.roll(x, delay)
    xd[:delay] = 0
    y = direct * x + amp * xd * np.exp(2j * np.pi * doppler * t) + noise * 200.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64), y.astype(np.complex64)


def col_err(got, ref, lvl, col, skip_row):
    """Largest error of the column's cells, each relative to itself or to the mean level if it lies below (an echo between two
    Doppler rows fills its column with sidelobes far above the mean level: those cells answer for their own size)."""
    e = np.abs(got[:, col].astype(np.complex128) - ref[:, col]) / np.maximum(np.abs(ref[:, col]), lvl)
    e[skip_row] = 0.0
    return float(e.max())


GEOMETRIES = [
    # (delayMin, delayMax, dopplerMin, dopplerMax, fs, n), echo (delay, doppler)
    ((-10, 400, -256, 256, 2_000_000, 2_000_000), (37, -63.0)),   # nD 513: the headline's geometry
    ((-10, 300, -512, 512, 2_000_000, 1_000_000), (120, 200.0)),  # nD 513 at 0.5 s (2 Hz rows)
    ((-8, 200, -512, 512, 1_000_000, 1_000_000), (50, 101.0)),    # nD 1025
    ((-8, 120, -1024, 1024, 1_000_000, 1_000_000), (9, -700.0)),  # nD 2049
    ((-4, 60, -100, 100, 500_000, 250_000), (20, 33.0)),          # nD 101: short pulses
]


@pytest.mark.parametrize("args,echo", GEOMETRIES)
def test_the_echo_column_is_transformed_in_fp64(b2, args, echo):
    n, fs = args[5], args[4]
    x, y = echo_cpi(n, fs, 11, *echo)
    d = O.ambiguity_dims(*args, True)
    ref = O.ambiguity_process(d, x.astype(np.complex128), y.astype(np.complex128))
    lvl = 10.0 ** (O.map_metrics(ref)[0] / 10.0)
    col = int(np.argmin(np.abs(d.delay - echo[0])))
    row = int(np.argmin(np.abs(d.doppler - echo[1])))
    assert np.abs(ref[row, col]) > 250.0 * lvl                      # the echo stands where the rule looks
    maps, hot = {}, {}
    for mode in ("off", "auto"):
        amb = b2.Ambiguity(*args, True)
        amb.set_hot_columns(mode)
        maps[mode] = amb.process(x, y).data.copy()
        hot[mode] = (amb.hot_columns(), amb.hot_columns_missed())
        kern = amb.last_doppler_kernel()
        amb.close()
    assert hot["off"] == (0, 0) and hot["auto"] == (1, 0), hot
    e_off, e_on = col_err(maps["off"], ref, lvl, col, row), col_err(maps["auto"], ref, lvl, col, row)
    other = np.ones(ref.shape, dtype=bool)
    other[:, col] = False
    floor = float((np.abs(maps["off"].astype(np.complex128) - ref) / np.maximum(np.abs(ref), lvl))[other].max())
    print(f"\n[hot] nD {ref.shape[0]} Doppler kernel {kern}: echo {np.abs(ref[row, col]) / lvl:.0f}x the mean level; its column's "
          f"largest error / mean level {e_off:.2e} -> {e_on:.2e} (other columns {floor:.2e})")
    assert np.array_equal(maps["off"][other], maps["auto"][other])  # no other cell moves
    assert e_on <= 2.0 * floor + 2e-6 and e_on < e_off
    g = map_cell_gate(maps["auto"], ref)
    assert g["ok"] and g["cell_rel_above_mean"] <= 3e-5, g
    # the peak cell itself: fp64 of the fp32 range map
    assert abs(maps["auto"][row, col] - ref[row, col]) <= 2e-6 * abs(ref[row, col])


def test_noise_has_no_hot_column_and_the_map_keeps_its_bits(b2):
    args = (-10, 400, -256, 256, 2_000_000, 2_000_000)
    rng = np.random.default_rng(3)
    x = ((rng.standard_normal(args[5]) + 1j * rng.standard_normal(args[5])) * 100).astype(np.complex64)
    y = ((rng.standard_normal(args[5]) + 1j * rng.standard_normal(args[5])) * 100).astype(np.complex64)
    out = {}
    for mode in ("off", "auto", "always"):
        amb = b2.Ambiguity(*args, True)
        amb.set_hot_columns(mode)
        out[mode] = amb.process(x, y).data.copy()
        assert amb.hot_columns() == 0 and amb.hot_columns_missed() == 0
        amb.close()
    assert np.array_equal(out["off"], out["auto"]) and np.array_equal(out["off"], out["always"])


def test_the_direct_path_column_is_left_to_the_doppler_kernel(b2):
    """y = 0.8 x + noise: the lag-0 column holds a peak 1000x the mean level AT ZERO DOPPLER, which the Doppler kernels take out
    exactly before they transform (the first pulse's value) -- nothing to transform again."""
    args = (-10, 400, -256, 256, 2_000_000, 2_000_000)
    x, y = echo_cpi(args[5], args[4], 9, 37, -63.0, amp=0.02, noise=0.1, direct=0.8)
    d = O.ambiguity_dims(*args, True)
    ref = O.ambiguity_process(d, x.astype(np.complex128), y.astype(np.complex128))
    lvl = 10.0 ** (O.map_metrics(ref)[0] / 10.0)
    c0 = int(np.argmin(np.abs(d.delay)))
    assert np.abs(ref[:, c0]).max() > 800.0 * lvl
    amb = b2.Ambiguity(*args, True)
    m = amb.process(x, y).data.copy()
    assert amb.hot_columns() == 0 and amb.hot_columns_missed() == 0
    amb.close()
    assert map_cell_gate(m, ref)["ok"]


def test_short_cpis_are_left_alone_in_auto_mode(b2):
    """Under 35 000 samples no peak can stand 250x above the mean level: auto mode does not launch the kernel; "always" does."""
    args = (-4, 40, -50, 50, 100_000, 20_000)
    x, y = echo_cpi(args[5], args[4], 5, 10, 7.0, noise=1e-3)
    d = O.ambiguity_dims(*args, True)
    ref = O.ambiguity_process(d, x.astype(np.complex128), y.astype(np.complex128))
    amb = b2.Ambiguity(*args, True)
    m_auto = amb.process(x, y).data.copy()
    assert amb.hot_columns() == 0
    amb.set_hot_columns("always")
    m_always = amb.process(x, y).data.copy()
    lvl = 10.0 ** (O.map_metrics(ref)[0] / 10.0)
    n_hot = amb.hot_columns()
    assert amb.hot_columns_missed() == 0
    amb.close()
    for m in (m_auto, m_always):
        assert np.max(np.abs(m.astype(np.complex128) - ref)) <= 1e-5 * np.abs(ref).max()
    col = int(np.argmin(np.abs(d.delay - 10)))
    if np.abs(ref[:, col]).max() > 250.0 * lvl:
        assert n_hot >= 1


def test_each_cpi_of_a_batch_has_its_own_columns(b2):
    import torch
    args = (-10, 400, -256, 256, 2_000_000, 2_000_000)
    B = 5
    d = O.ambiguity_dims(*args, True)
    echoes = [(37, -63.0), None, (200, 10.0), (37, 100.0), None]
    data = []
    for c, e in enumerate(echoes):
        if e is None:
            rng = np.random.default_rng(40 + c)
            mk = lambda: ((rng.standard_normal(args[5]) + 1j * rng.standard_normal(args[5])) * 100).astype(np.complex64)
            data.append((mk(), mk()))
        else:
            data.append(echo_cpi(args[5], args[4], 40 + c, *e))
    xs = torch.from_numpy(np.stack([v[0] for v in data])).cuda()
    ys = torch.from_numpy(np.stack([v[1] for v in data])).cuda()
    st = torch.cuda.current_stream().cuda_stream
    res = {}
    for mode in ("off", "auto"):
        amb = b2.Ambiguity(*args, True, max_batch=B)
        amb.set_hot_columns(mode)
        out = torch.zeros((B, d.n_doppler_bins, d.n_delay_bins), dtype=torch.complex64, device="cuda")
        met = torch.zeros((B, 2), dtype=torch.float64, device="cuda")
        amb.process_dev(b2.FMT_C32, xs.data_ptr(), ys.data_ptr(), B, args[5], out.data_ptr(), met.data_ptr(), st)
        torch.cuda.synchronize()
        res[mode] = (out.cpu().numpy(), met.cpu().numpy())
        assert amb.hot_columns() == (1 if mode == "auto" else 0)       # of CPI 0
        assert amb.hot_columns_missed() == 0                            # of any CPI
        amb.close()
    assert np.array_equal(res["off"][1], res["auto"][1])               # Map::set_metrics: taken before the rewrite
    for c, e in enumerate(echoes):
        a, b = res["off"][0][c], res["auto"][0][c]
        changed = np.flatnonzero(np.any(a != b, axis=0))
        if e is None:
            assert changed.size == 0, (c, changed)
            continue
        col = int(np.argmin(np.abs(d.delay - e[0])))
        assert list(changed) == [col], (c, changed, col)
    c = 2
    ref = O.ambiguity_process(d, data[c][0].astype(np.complex128), data[c][1].astype(np.complex128))
    g = map_cell_gate(res["auto"][0][c], ref)
    assert g["ok"] and g["cell_rel_above_mean"] <= 3e-5, g
    nz, mx = O.map_metrics(ref)
    assert abs(res["auto"][1][c][0] - nz) < 1e-3 and abs(res["auto"][1][c][1] - mx) < 1e-3


def test_the_strongest_sixteen_of_many(b2):
    """More columns qualify than the kernel rewrites: 16 echoes at amplitude 1.4 and 2 at 1.0, every one of them above
    HOT_RATIO x the mean level, all on Dopplers that are whole multiples of 8 bins.  The estimate reads between HOT_BOUND (0.8)
    and 1 of an echo's amplitude, so 1.4 x 0.8 > 1.0 sets the sixteen apart whatever their Dopplers: exactly their columns
    are rewritten, and the two left with their fp32 values are counted as missed."""
    args = (-10, 400, -256, 256, 2_000_000, 2_000_000)
    n, fs = args[5], args[4]
    d = O.ambiguity_dims(*args, True)
    rng = np.random.default_rng(8)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 200.0
    t = np.arange(n) / fs
    y = 0.01 * 200.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    lags = list(range(20, 20 + 18 * 20, 20))                                   # 18 echoes, 20 lags apart
    bins = [8 * b for b in range(-9, 10) if b != 0]                            # -72 ... 72 bins, zero Doppler left out
    weak = (5, 11)                                                             # amplitude 1.0; the others 1.4
    for i, (lag, b) in enumerate(zip(lags, bins)):
        xd = np.roll(x, lag)
        xd[:lag] = 0
        y = y + (1.0 if i in weak else 1.4) * xd * np.exp(2j * np.pi * (b / d.cpi) * t)
    x, y = x.astype(np.complex64), y.astype(np.complex64)
    ref = O.ambiguity_process(d, x.astype(np.complex128), y.astype(np.complex128))
    lvl = 10.0 ** (O.map_metrics(ref)[0] / 10.0)
    cols = [int(np.argmin(np.abs(d.delay - lag))) for lag in lags]
    peaks = [float(np.abs(ref[:, c]).max() / lvl) for c in cols]
    assert min(peaks) > HOT_RATIO, peaks                                      # every echo qualifies
    out, hot = {}, {}
    for mode in ("off", "auto"):
        amb = b2.Ambiguity(*args, True)
        amb.set_hot_columns(mode)
        out[mode] = amb.process(x, y).data.copy()
        hot[mode] = (amb.hot_columns(), amb.hot_columns_missed())
        amb.close()
    print(f"\n[hot] 18 echoes {min(peaks):.0f}x ... {max(peaks):.0f}x the mean level: (rewritten, missed) {hot}")
    assert hot["off"] == (0, 0) and hot["auto"] == (16, 2), hot
    changed = np.flatnonzero(np.any(out["off"] != out["auto"], axis=0))
    strong = sorted(c for i, c in enumerate(cols) if i not in weak)
    assert list(changed) == strong, (changed, strong)


# Geometries for the blind-Doppler tests: (delayMin, delayMax, dopplerMin, dopplerMax, fs, n), explicit Doppler bin count
BLIND_GEOMETRIES = {
    513: ((-10, 400, -256, 256, 2_000_000, 2_000_000), 0),
    1025: ((-8, 200, -512, 512, 1_000_000, 1_000_000), 0),
    2049: ((-8, 120, -1024, 1024, 1_000_000, 1_000_000), 0),
    4096: ((-4, 60, -2048, 2048, 2_000_000, 2_000_000), 4096),
}


def blind_bins(nD):
    """Dopplers (bins off zero) where a sparse look at the range map reads least: whole multiples of 8 (where the phases of
    pulses nD/8 apart line up), the exact zero of the four-pulse rule of round 6 (64.125 nD / 513), and the worst Doppler of
    today's rule, from the CPU model of tests/test_hot_columns_model.py."""
    return [8.0, 16.0, 64.0, -64.0, 64.125 * nD / 513, worst_k(nD)[0]]


BLIND_CASES = [(nD, k) for nD in BLIND_GEOMETRIES for k in blind_bins(nD)]


@pytest.mark.parametrize("nD,k", BLIND_CASES, ids=[f"nD{nD}-k{k:+.4f}" for nD, k in BLIND_CASES])
def test_an_echo_at_a_blind_doppler_is_transformed_in_fp64(b2, nD, k):
    args, nd_explicit = BLIND_GEOMETRIES[nD]
    d = O.ambiguity_dims(*args, True, n_doppler_bins=nd_explicit)
    assert d.n_doppler_bins == nD
    delay = 9
    x, y = echo_cpi(args[5], args[4], 31, delay, k / d.cpi)                  # k bins = k / cpi Hz
    ref = O.ambiguity_process(d, x.astype(np.complex128), y.astype(np.complex128))
    lvl = 10.0 ** (O.map_metrics(ref)[0] / 10.0)
    col = int(np.argmin(np.abs(d.delay - delay)))
    row = int(np.argmax(np.abs(ref[:, col])))
    assert np.abs(ref[row, col]) > HOT_RATIO * lvl                            # the echo qualifies
    maps, hot = {}, {}
    for mode in ("off", "auto"):
        amb = b2.Ambiguity(*args, True, n_doppler_bins=nd_explicit)
        amb.set_hot_columns(mode)
        maps[mode] = amb.process(x, y).data.copy()
        hot[mode] = (amb.hot_columns(), amb.hot_columns_missed())
        amb.close()
    other = np.ones(ref.shape, dtype=bool)
    other[:, col] = False
    e_off, e_on = col_err(maps["off"], ref, lvl, col, row), col_err(maps["auto"], ref, lvl, col, row)
    floor = float((np.abs(maps["off"].astype(np.complex128) - ref) / np.maximum(np.abs(ref), lvl))[other].max())
    g = map_cell_gate(maps["auto"], ref)
    print(f"\n[hot blind] nD {nD} k {k:+.4f}: echo {np.abs(ref[row, col]) / lvl:.0f}x the mean level; (rewritten, missed) "
          f"{hot['auto']}; its column's error / mean level {e_off:.2e} -> {e_on:.2e} (other columns {floor:.2e}); "
          f"cell gate {g['cell_rel_above_mean']:.2e}")
    assert hot["off"] == (0, 0)
    assert hot["auto"][0] >= 1, hot
    assert np.array_equal(maps["off"][other], maps["auto"][other])           # only the echo column changes
    assert not np.array_equal(maps["off"][:, col], maps["auto"][:, col])
    assert e_on < e_off and e_on <= 2.0 * floor + 2e-6                       # the echo put the floor in reach; fp64 took it out
    # north_star's 1e-4 everywhere; 3e-5 up to nD = 2049.  At nD = 4096 the direct-DFT Doppler kernel's own fp32 floor is
    # ~5e-5 in EVERY column (measured: 4.8e-5 ... 6.2e-5 with the echo's column rewritten, its column 4e-6)
    assert g["ok"] and g["cell_rel_above_mean"] <= (3e-5 if nD <= 2049 else 1e-4), g
    assert abs(maps["auto"][row, col] - ref[row, col]) <= 2e-6 * abs(ref[row, col])
    assert hot["auto"] == (1, 0), hot


def test_every_multiple_of_8_bins_in_one_batch(b2):
    """nD = 513 at 0.5 s: 64 CPIs in one process_dev call, CPI c with one echo at lag 3 + c on Doppler bin 8 (c - 32) (c < 32)
    or 8 (c - 31) -- every whole multiple of 8 bins from -256 to +256.  In every CPI its echo's column is rewritten and no
    other; the oracle checks three of them."""
    import torch
    args = (-10, 120, -512, 512, 2_000_000, 1_000_000)
    n, fs = args[5], args[4]
    d = O.ambiguity_dims(*args, True)
    assert d.n_doppler_bins == 513
    bins = [8 * (c - 32) for c in range(32)] + [8 * (c - 31) for c in range(32, 64)]
    B = len(bins)
    assert B == 64 and 0 not in bins and min(bins) == -256 and max(bins) == 256
    rng = np.random.default_rng(64)
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 200.0).astype(np.complex64)
    t = np.arange(n) / fs
    ys = np.empty((B, n), dtype=np.complex64)
    for c, b in enumerate(bins):
        lag = 3 + c
        xd = np.roll(x, lag)
        xd[:lag] = 0
        ys[c] = xd * np.exp(2j * np.pi * (b / d.cpi) * t) + 4.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    xs = torch.from_numpy(np.broadcast_to(x, (B, n)).copy()).cuda()
    yd = torch.from_numpy(ys).cuda()
    st = torch.cuda.current_stream().cuda_stream
    res, hot = {}, {}
    for mode in ("off", "auto"):
        amb = b2.Ambiguity(*args, True, max_batch=B)
        amb.set_hot_columns(mode)
        out = torch.zeros((B, d.n_doppler_bins, d.n_delay_bins), dtype=torch.complex64, device="cuda")
        met = torch.zeros((B, 2), dtype=torch.float64, device="cuda")
        amb.process_dev(b2.FMT_C32, xs.data_ptr(), yd.data_ptr(), B, n, out.data_ptr(), met.data_ptr(), st)
        torch.cuda.synchronize()
        res[mode] = out.cpu().numpy()
        hot[mode] = (amb.hot_columns(), amb.hot_columns_missed())
        amb.close()
    assert hot["off"] == (0, 0) and hot["auto"] == (1, 0), hot
    wrong = []
    for c in range(B):
        col = int(np.argmin(np.abs(d.delay - (3 + c))))
        changed = list(np.flatnonzero(np.any(res["off"][c] != res["auto"][c], axis=0)))
        if changed != [col]:
            wrong.append((c, bins[c], changed, col))
    assert not wrong, wrong
    for c in (24, 31, 63):                                                    # -64, -8 and +256 bins
        ref = O.ambiguity_process(d, x.astype(np.complex128), ys[c].astype(np.complex128))
        lvl = 10.0 ** (O.map_metrics(ref)[0] / 10.0)
        col = int(np.argmin(np.abs(d.delay - (3 + c))))
        assert np.abs(ref[:, col]).max() > HOT_RATIO * lvl
        g = map_cell_gate(res["auto"][c], ref)
        print(f"\n[hot sweep] CPI {c} ({bins[c]:+d} bins): echo {np.abs(ref[:, col]).max() / lvl:.0f}x the mean level, "
              f"cell gate {g['cell_rel_above_mean']:.2e}")
        assert g["ok"] and g["cell_rel_above_mean"] <= 3e-5, g


def test_a_blind_doppler_behind_the_clutter_filter(b2):
    """BASELINE configs[1] end to end through the clutter filter (410 taps, lags -10 .. 400): a target on Doppler bin 8, which
    the four-pulse rule of round 6 read at 0.056 of its amplitude, ~2000x the cancelled map's mean level.  The map's gates of
    tests/test_full_chain_gpu.py hold, with its column rewritten."""
    import torch
    from test_full_chain_gpu import check_chain_map
    geom = (-10, 400, -256, 256, 2_000_000, 2_000_000)
    n, fs = geom[5], geom[4]
    d = O.ambiguity_dims(*geom, True)
    f = 8.0 / d.cpi
    x, y = O.synth_iq(n, seed=64, fs=fs, targets=((37, f, 0.1),))
    ok_ref, y_ref, w_ref, r_ref, b_ref = O.wiener_hopf(x, y, -10, 400, return_filter=True)
    assert ok_ref
    m_ref = O.ambiguity_process(d, x, y_ref)
    noise_ref, max_ref = O.map_metrics(m_ref)
    col = int(np.argmin(np.abs(d.delay - 37)))
    assert np.abs(m_ref[:, col]).max() > HOT_RATIO * 10.0 ** (noise_ref / 10.0)
    wh = b2.WienerHopf(-10, 400, n)
    amb = b2.Ambiguity(*geom, True)
    dx = torch.from_numpy(x.astype(np.complex64)).cuda()
    dy = torch.from_numpy(y.astype(np.complex64)).cuda()
    okf = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    wh.process_dev(dx.data_ptr(), dy.data_ptr(), 1, n, dy.data_ptr(), okf.data_ptr(), st)  # in place
    amb.process_dev(b2.FMT_C32, dx.data_ptr(), dy.data_ptr(), 1, n, None, None, st)
    torch.cuda.synchronize()
    assert int(okf.item()) == 1
    m = amb.read_last(0)
    hot = (amb.hot_columns(), amb.hot_columns_missed())
    print(f"\n[hot chain] target {np.abs(m_ref[:, col]).max() / 10.0 ** (noise_ref / 10.0):.0f}x the mean level, "
          f"(rewritten, missed) {hot}")
    assert hot == (1, 0), hot
    direct_level = np.max(np.abs(b_ref)) * (d.n_corr * d.n_doppler_bins / n)
    check_chain_map("cfg2 chain, bin 8", m.data.astype(np.complex128), m.noisePower, m_ref, noise_ref, direct_level,
                    d.doppler, d.delay, -10, 400)
    assert abs(m.noisePower - noise_ref) <= 1e-3 and abs(m.maxPower - max_ref) <= 1e-3


@pytest.mark.parametrize("nD", [1025, 2049, 4096])
def test_noise_has_no_hot_column_at_long_doppler_axes(b2, nD):
    """The test is lowered by HOT_BOUND, and noise columns sit closest to it at the longest Doppler axes (a factor
    0.75 x 0.8 x 250 / sqrt(nD) = 2.3 at nD = 4096): white noise in "always" mode finds nothing, and the map keeps its bits."""
    args, nd_explicit = BLIND_GEOMETRIES[nD]
    rng = np.random.default_rng(nD)
    mk = lambda: ((rng.standard_normal(args[5]) + 1j * rng.standard_normal(args[5])) * 100).astype(np.complex64)
    x, y = mk(), mk()
    out = {}
    for mode in ("off", "always"):
        amb = b2.Ambiguity(*args, True, n_doppler_bins=nd_explicit)
        assert amb.get_n_doppler_bins() == nD
        amb.set_hot_columns(mode)
        out[mode] = amb.process(x, y).data.copy()
        assert (amb.hot_columns(), amb.hot_columns_missed()) == (0, 0)
        amb.close()
    assert np.array_equal(out["off"], out["always"])
