"""GPU: adaptive beams -- the array covariance of the channel maps (blah2hip_amb_covariance_dev: array_cov_kernel +
cov_fold_kernel), minimum-variance weights from it (blah2hip_amb_mvdr_weights_dev: mvdr_weights_kernel) and beams with
per-CPI weights read from the device (blah2hip_amb_beamform_wdev: beamform_wdev_kernel).

No reference counterpart; the checks are fp64 NumPy restatements with derived bounds.  As in tests/test_beamform_gpu.py
the kernels read any buffer with the map layout, so the cases feed crafted maps and the handle is only there for its
dimensions.  Every output has guard words behind it.

Bounds
  * covariance: |R_dev - R_fp64| <= 4 * 2^-24 * sum |M_i| |M_j| per entry.  The arithmetic contract allows fp32 products:
    per component two roundings of at most 2^-24 |M_i| |M_j| each, so under 2 sqrt(2) * 2^-24 per cell in magnitude, and
    the fp64 additions add n * 2^-53 of the same sum (n <= 210 843 cells: 2.4e-11, nothing beside 2^-24 = 6e-8).
  * weights: |w_dev - w_ref| <= 2^-23 ||w_ref||inf + 64 K 2^-53 cond(R_l) ||w_ref||inf per entry against mvdr_weights on
    the same fp64 R: fp32 storage, then the Cholesky solve.  The inputs keep cond(R_l) <= 1e5 (asserted), so the first
    term dominates.  Distortionless to K * 2^-23.
  * beamform_wdev: bit-identical to beamform_dev, maps and metrics, where the weights agree; metrics within 1e-3 dB (the
    project's DB_TOL) of fp64 Map::set_metrics of the device's own cells otherwise.
Geometries: 21 x 111 cells (odd count), 21 x 112 (even) and one case at the configs[1] size 513 x 411 with 3 CPIs (many
workgroups, strided walks).
"""
import ctypes as C

import numpy as np
import pytest

import adaptive_crafted as A

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces
PAD = 64
MAX_BATCH = 24
SMALL = (-10, 100, -100, 100, 1_000_000, 100_000)    # 21 x 111
EVEN = (-10, 101, -100, 100, 1_000_000, 100_000)     # 21 x 112
CFG2 = (-10, 400, -256, 256, 2_000_000, 2_000_000)   # configs[1]: 513 x 411
DB_TOL = 1e-3
EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


_handles = {}


def handle(b2, geom):
    if geom not in _handles:
        _handles[geom] = b2.Ambiguity(*geom, True, max_batch=MAX_BATCH)
    return _handles[geom]


def stream(torch):
    return torch.cuda.current_stream().cuda_stream


def guarded(torch, shape, dtype):
    words = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size() // 4
    whole = torch.full((words + PAD,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    return whole, whole[:words].view(dtype).view(shape)


def guard_intact(whole):
    return bool((whole[-PAD:].cpu().numpy().view(np.uint32) == GUARD).all())


def untouched(whole):
    return bool((whole.cpu().numpy().view(np.uint32) == GUARD).all())


def crafted(K, n_cpi, nD, nC, seed, scaled=True):
    """Unit-variance complex normal cells, channel k scaled by 10^k (a dropped or swapped channel shows), no cell zero."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((K, n_cpi, nD, nC)) + 1j * rng.standard_normal((K, n_cpi, nD, nC))) * np.sqrt(0.5)
    if scaled:
        z *= (10.0 ** np.arange(K))[:, None, None, None]
    z = z.astype(np.complex64)
    assert (z != 0).all()
    return z


def with_interferer(K, n_cpi, nD, nC, seed):
    """Unscaled channels plus a 30 dB plane wave from -24 degrees in every cell of three rows: cond(R_l) stays small."""
    z = crafted(K, n_cpi, nD, nC, seed, scaled=False).astype(np.complex128)
    rng = np.random.default_rng(seed + 1)
    a = np.exp(2j * np.pi * 0.5 * np.sin(np.deg2rad(-24.0)) * np.arange(K))
    z[:, :, 9:12, :] += 31.6 * a[:, None, None, None] * np.exp(2j * np.pi * rng.random((n_cpi, 3, nC)))[None]
    return z.astype(np.complex64)


def weights(n_cpi, n_beams, K, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_cpi, n_beams, K)) + 1j * rng.standard_normal((n_cpi, n_beams, K))).astype(np.complex64)


def set_metrics64(z):
    """Map::set_metrics (Map.cpp:187-206) in fp64."""
    db = 10.0 * np.log10(np.abs(z.astype(np.complex128)))
    noise = db.mean()
    return noise, max(0.0, db.max()) - noise


def cov_dev(torch, amb, d_in, K, n_cpi, region=None):
    """One call into a guarded output -> R [n_cpi, K, K] complex128."""
    wc, cov = guarded(torch, (n_cpi, K, K), torch.complex128)
    amb.covariance_dev(d_in.data_ptr(), K, n_cpi, cov.data_ptr(), region, stream(torch))
    torch.cuda.synchronize()
    assert guard_intact(wc)
    return cov.cpu().numpy()


def cov_check(R, maps, region, tag):
    """The derived bound, exact Hermitian symmetry and a diagonal with imaginary parts exactly 0; prints the worst ratio."""
    m = maps.astype(np.complex128)
    if region is not None:
        m = m[:, :, region[0]:region[1], region[2]:region[3]]
    ref = np.einsum("icrq,jcrq->cij", m, np.conj(m))
    bound = 4 * EPS32 * np.einsum("icrq,jcrq->cij", np.abs(m), np.abs(m))
    err = np.abs(R - ref)
    print(f"{tag}: largest error / bound {float((err / bound).max()):.3e}")
    assert np.isfinite(R.view(np.float64)).all(), tag
    assert (err <= bound).all(), (tag, float((err / bound).max()))
    K = R.shape[-1]
    assert np.array_equal(R, np.conj(np.swapaxes(R, -1, -2))), tag
    assert (R[:, np.arange(K), np.arange(K)].imag == 0).all(), tag


# ---- 1. covariance ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cpi", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 8])
def test_covariance_of_the_whole_map(b2, torch, K, n_cpi):
    amb = handle(b2, SMALL)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    assert (nD * nC) % 2 == 1
    maps = crafted(K, n_cpi, nD, nC, seed=2000 + 10 * K + n_cpi)
    d_in = torch.from_numpy(maps).cuda()
    R = cov_dev(torch, amb, d_in, K, n_cpi)
    cov_check(R, maps, None, f"covariance K={K} n_cpi={n_cpi} {nD}x{nC}")
    R2 = cov_dev(torch, amb, d_in, K, n_cpi)
    assert np.array_equal(R.view(np.uint64), R2.view(np.uint64))  # two calls: the same bits


def test_covariance_at_the_large_geometry(b2, torch):
    K, n_cpi = 4, 3
    amb = handle(b2, CFG2)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    assert (nD, nC) == (513, 411)
    maps = crafted(K, n_cpi, nD, nC, seed=2100)
    d_in = torch.from_numpy(maps).cuda()
    R = cov_dev(torch, amb, d_in, K, n_cpi)
    cov_check(R, maps, None, f"covariance K={K} n_cpi={n_cpi} {nD}x{nC}")
    assert np.array_equal(R.view(np.uint64), cov_dev(torch, amb, d_in, K, n_cpi).view(np.uint64))
    region = (100, 413, 7, 400)  # an odd first column and an odd width, many rows
    cov_check(cov_dev(torch, amb, d_in, K, n_cpi, region), maps, region, f"covariance {region} of {nD}x{nC}")


@pytest.mark.parametrize("geom", [SMALL, EVEN], ids=["111cols", "112cols"])
def test_covariance_over_rectangles(b2, torch, geom):
    K, n_cpi = 3, 3
    amb = handle(b2, geom)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    maps = crafted(K, n_cpi, nD, nC, seed=2200 + nC)
    d_in = torch.from_numpy(maps).cuda()
    regions = {"the whole map": (0, nD, 0, nC), "one cell": (5, 6, 17, 18), "one row": (20, 21, 0, nC),
               "one column": (0, nD, nC - 1, nC), "odd col0, odd width": (2, 19, 3, 3 + 77),
               "the bottom-right corner": (nD - 4, nD, nC - 9, nC)}
    for name, region in regions.items():
        R = cov_dev(torch, amb, d_in, K, n_cpi, region)
        cov_check(R, maps, region, f"covariance over {name} of {nD}x{nC}")
        if name == "one cell":  # one product per entry: what the cell holds, exactly (fp32 x fp32 is exact in fp64)
            m = maps[:, :, 5, 17].astype(np.complex128)
            assert np.allclose(R, np.einsum("ic,jc->cij", m, np.conj(m)), rtol=2 * EPS64, atol=0)


def test_a_nan_outside_the_rectangle_is_not_read(b2, torch):
    K, n_cpi = 2, 2
    amb = handle(b2, SMALL)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    maps = crafted(K, n_cpi, nD, nC, seed=2300)
    region = (3, 10, 20, 51)
    for r, q in ((2, 30), (10, 30), (5, 19), (5, 51), (0, 0), (nD - 1, nC - 1)):  # all round the rectangle, and the corners
        maps[:, :, r, q] = np.nan
    R = cov_dev(torch, amb, torch.from_numpy(maps).cuda(), K, n_cpi, region)
    cov_check(R, maps, region, "covariance beside NaN cells")
    # ... and one inside reaches every entry it takes part in
    maps[1, 0, 4, 25] = np.nan
    R = cov_dev(torch, amb, torch.from_numpy(maps).cuda(), K, n_cpi, region)
    assert np.isfinite(R[0, 0, 0]) and np.isnan(R[0, 1, 1].real) and np.isnan(R[0, 0, 1].real) and np.isfinite(R[1].view(np.float64)).all()


def test_covariance_refusals_write_nothing(b2, torch):
    from blah2_amd import _lib
    amb = handle(b2, SMALL)
    L, h = amb._L, amb._h
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    cells = nD * nC
    d_in = torch.from_numpy(crafted(8, 3, nD, nC, seed=5)).cuda()
    wc, cov = guarded(torch, (MAX_BATCH, 8, 8), torch.complex128)
    int_map, int_met = C.c_void_p(), C.c_void_p()
    assert L.blah2hip_amb_result_ptrs(h, C.byref(int_map), C.byref(int_met)) == _lib.OK
    # (d_map, n_surv, n_cpi, row0, row1, col0, col1, d_cov)
    good = [d_in.data_ptr(), 2, 3, 0, nD, 0, nC, cov.data_ptr()]
    bad = {
        "n_surv 0": {1: 0}, "n_surv 9": {1: 9, 2: 1}, "n_cpi 0": {2: 0}, "n_surv * n_cpi above max_batch": {1: 8, 2: 4},
        "NULL output": {7: None}, "row0 == row1": {3: 4, 4: 4}, "row0 > row1": {3: 5, 4: 4}, "row1 > nD": {4: nD + 1},
        "col0 == col1": {5: 9, 6: 9}, "col0 > col1": {5: 10, 6: 9}, "col1 > nDelay": {6: nC + 1},
        "a rectangle far outside": {3: 0xFFFFFFF0, 4: 0xFFFFFFFF},
        "output inside the input": {7: d_in.data_ptr() + 8 * (2 * 3 * cells - 1)},
        "output around the input's start": {0: cov.data_ptr() + 16},
        "output in the handle's own map": {0: None, 7: int_map.value + 8 * cells},
    }
    for name, change in bad.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert L.blah2hip_amb_covariance_dev(h, *args, None) == _lib.ERR_INVALID, name
    assert L.blah2hip_amb_covariance_dev(None, *good, None) == _lib.ERR_INVALID
    torch.cuda.synchronize()
    assert untouched(wc)
    assert L.blah2hip_amb_covariance_dev(h, *good, None) == _lib.OK
    torch.cuda.synchronize()
    assert guard_intact(wc) and not untouched(wc)


# ---- 2. weights ---------------------------------------------------------------------------------------------------------
def mvdr_dev(torch, amb, R, steer, loading):
    """R [n_cpi, K, K] complex128 (host) -> (w [n_cpi, n_beams, K] complex64, ok [n_cpi] int32) through guarded outputs."""
    n_cpi, K = R.shape[0], R.shape[-1]
    d_cov = torch.from_numpy(np.ascontiguousarray(R)).cuda()
    ww, w = guarded(torch, (n_cpi, steer.shape[0], K), torch.complex64)
    wk, ok = guarded(torch, (n_cpi,), torch.int32)
    amb.mvdr_weights_dev(d_cov.data_ptr(), K, n_cpi, steer, loading, w.data_ptr(), ok.data_ptr(), stream(torch))
    torch.cuda.synchronize()
    assert guard_intact(ww) and guard_intact(wk)
    return w.cpu().numpy(), ok.cpu().numpy()


def weights_check(b2, w, ok, R, steer32, loading, tag):
    K = R.shape[-1]
    ref, ok_ref = b2.mvdr_weights(R, steer32, loading)
    assert ok.tolist() == ok_ref.tolist() == [1] * R.shape[0], tag
    worst = 0.0
    for c in range(R.shape[0]):
        cond = np.linalg.cond(R[c] + loading * (np.trace(R[c]).real / K) * np.eye(K))
        assert cond <= 1e5, (tag, c, cond)
        for b in range(steer32.shape[0]):
            top = np.abs(ref[c, b]).max()
            bound = 2.0 ** -23 * top + 64 * K * EPS64 * cond * top
            err = np.abs(w[c, b].astype(np.complex128) - ref[c, b]).max()
            worst = max(worst, err / bound)
            assert err <= bound, (tag, c, b, err, bound)
            assert abs(w[c, b].astype(np.complex128) @ steer32[b].astype(np.complex128) - 1.0) <= K * 2.0 ** -23, (tag, c, b)
    print(f"{tag}: largest weight error / bound {worst:.3f}")


@pytest.mark.parametrize("K", [2, 4, 8])
def test_weights_from_the_device_covariance(b2, torch, K):
    n_cpi, loading = 3, 1e-3
    amb = handle(b2, SMALL)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    maps = with_interferer(K, n_cpi, nD, nC, seed=3000 + K)
    steer32 = b2.ula_steering(K, 0.5, [20.0, 0.0, -50.0]).astype(np.complex64)
    st = stream(torch)
    d_in = torch.from_numpy(maps).cuda()
    wc, cov = guarded(torch, (n_cpi, K, K), torch.complex128)
    ww, w = guarded(torch, (n_cpi, 3, K), torch.complex64)
    wk, ok = guarded(torch, (n_cpi,), torch.int32)
    amb.covariance_dev(d_in.data_ptr(), K, n_cpi, cov.data_ptr(), None, st)
    amb.mvdr_weights_dev(cov.data_ptr(), K, n_cpi, steer32, loading, w.data_ptr(), ok.data_ptr(), st)
    torch.cuda.synchronize()
    assert guard_intact(wc) and guard_intact(ww) and guard_intact(wk)
    weights_check(b2, w.cpu().numpy(), ok.cpu().numpy(), cov.cpu().numpy(), steer32, loading, f"weights from the device's R, K={K}")


def sample_covariance(K, n, seed, n_cpi):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n_cpi, K, n)) + 1j * rng.standard_normal((n_cpi, K, n))) * np.sqrt(0.5)
    x = x + 30.0 * np.exp(2j * np.pi * 0.21 * np.arange(K))[:, None] * (rng.standard_normal((n_cpi, 1, n)) + 0j)
    R = x @ np.conj(np.swapaxes(x, -1, -2))
    return 0.5 * (R + np.conj(np.swapaxes(R, -1, -2)))


@pytest.mark.parametrize("K", [1, 3, 5, 8])
def test_weights_from_crafted_hermitian_matrices(b2, torch, K):
    amb = handle(b2, SMALL)
    R = sample_covariance(K, 300, seed=3100 + K, n_cpi=2)
    steer32 = b2.ula_steering(K, 0.5, [20.0, -35.0]).astype(np.complex64)
    for loading in (1e-3, 0.5):
        w, ok = mvdr_dev(torch, amb, R, steer32, loading)
        weights_check(b2, w, ok, R, steer32, loading, f"weights from a crafted R, K={K} loading={loading}")
    # NULL d_ok is allowed
    ww, w2 = guarded(torch, (2, 2, K), torch.complex64)
    d_cov = torch.from_numpy(R).cuda()
    amb.mvdr_weights_dev(d_cov.data_ptr(), K, 2, steer32, 0.5, w2.data_ptr(), None, stream(torch))
    torch.cuda.synchronize()
    assert guard_intact(ww) and np.array_equal(w2.cpu().numpy().view(np.uint32), w.view(np.uint32))


@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_identity_covariance_gives_ula_weights(b2, torch, K):
    """Angles whose phase steps are multiples of a quarter turn and element counts that are powers of two: the steering
    vectors survive the rounding to fp32 and the division by K is exact, so the result is ula_weights rounded to fp32, bit
    for bit."""
    amb = handle(b2, SMALL)
    angles = [0.0, 30.0, -30.0, 90.0]
    R = np.broadcast_to(np.eye(K, dtype=np.complex128), (2, K, K)).copy()
    w, ok = mvdr_dev(torch, amb, R, b2.ula_steering(K, 0.5, angles), 0.0)
    assert ok.tolist() == [1, 1]
    want = b2.ula_weights(K, 0.5, angles).astype(np.complex64)
    assert np.array_equal(w[0], want) and np.array_equal(w[1], want)


def test_a_zero_cpi_falls_back_and_leaves_its_neighbours_alone(b2, torch):
    K, loading = 4, 1e-3
    amb = handle(b2, SMALL)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    maps = with_interferer(K, 3, nD, nC, seed=3200)
    maps[:, 1] = 0
    steer = b2.ula_steering(K, 0.5, [20.0, 0.0])
    steer[1] *= 3.0  # not unit modulus: the fallback divides by a^H a
    steer32 = steer.astype(np.complex64)
    R = cov_dev(torch, amb, torch.from_numpy(maps).cuda(), K, 3)
    assert (R[1] == 0).all()
    w, ok = mvdr_dev(torch, amb, R, steer32, loading)
    assert ok.tolist() == [1, 0, 1]
    a = steer32.astype(np.complex128)
    conventional = np.conj(a) / (np.abs(a) ** 2).sum(axis=1)[:, None]
    assert np.abs(w[1] - conventional).max() <= 2.0 ** -23 * np.abs(conventional).max()
    for c in (0, 2):
        w1, ok1 = mvdr_dev(torch, amb, R[c:c + 1], steer32, loading)
        assert ok1.tolist() == [1] and np.array_equal(w1[0].view(np.uint32), w[c].view(np.uint32)), c
    # a NaN in the maps fails its CPI the same way
    maps[2, 2, 7, 7] = np.nan
    R = cov_dev(torch, amb, torch.from_numpy(maps).cuda(), K, 3)
    w3, ok3 = mvdr_dev(torch, amb, R, steer32, loading)
    assert ok3.tolist() == [1, 0, 0] and np.array_equal(w3[2].view(np.uint32), w[1].view(np.uint32))
    assert np.array_equal(w3[0].view(np.uint32), w[0].view(np.uint32))


def test_weights_refusals_write_nothing(b2, torch):
    from blah2_amd import _lib
    amb = handle(b2, SMALL)
    L, h = amb._L, amb._h
    K = 4
    d_cov = torch.from_numpy(sample_covariance(K, 100, seed=6, n_cpi=3)).cuda()
    ww, w = guarded(torch, (3, 8, 8), torch.complex64)
    wk, ok = guarded(torch, (3,), torch.int32)
    steer = np.ascontiguousarray(np.ones((9, 9)), dtype=np.complex64)
    zero = steer.copy()
    zero.reshape(-1)[K:2 * K] = 0  # beam 1 of [n_beams][4]
    sp, zp = C.c_void_p(steer.ctypes.data), C.c_void_p(zero.ctypes.data)
    # (d_cov, n_surv, n_cpi, steer, n_beams, loading, d_w, d_ok)
    good = [d_cov.data_ptr(), K, 3, sp, 2, 1e-3, w.data_ptr(), ok.data_ptr()]
    bad = {"NULL covariance": {0: None}, "NULL steer": {3: None}, "NULL weights": {6: None}, "n_surv 0": {1: 0}, "n_surv 9": {1: 9},
           "n_beams 0": {4: 0}, "n_beams 9": {4: 9}, "n_cpi 0": {2: 0}, "loading < 0": {5: -1e-3}, "loading nan": {5: float("nan")},
           "loading inf": {5: float("inf")}, "a steering vector that is all zero": {3: zp}}
    for name, change in bad.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert L.blah2hip_amb_mvdr_weights_dev(h, *args, None) == _lib.ERR_INVALID, name
    assert L.blah2hip_amb_mvdr_weights_dev(None, *good, None) == _lib.ERR_INVALID
    torch.cuda.synchronize()
    assert untouched(ww) and untouched(wk)
    assert L.blah2hip_amb_mvdr_weights_dev(h, *good, None) == _lib.OK
    torch.cuda.synchronize()
    assert guard_intact(ww) and guard_intact(wk) and ok.cpu().numpy().tolist() == [1, 1, 1]


# ---- 3. beams with weights from the device ------------------------------------------------------------------------------
def beamform_host_w(torch, amb, d_in, K, n_cpi, w):
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    wo, out = guarded(torch, (w.shape[0], n_cpi, nD, nC), torch.complex64)
    wm, met = guarded(torch, (w.shape[0], n_cpi, 2), torch.float64)
    amb.beamform_dev(d_in.data_ptr(), K, n_cpi, w, out.data_ptr(), met.data_ptr(), stream(torch))
    torch.cuda.synchronize()
    assert guard_intact(wo) and guard_intact(wm)
    return out.cpu().numpy(), met.cpu().numpy()


def beamform_dev_w(torch, amb, d_in, K, n_cpi, w):
    """w [n_cpi, n_beams, K] complex64, uploaded -> (beam maps [n_beams, n_cpi, nD, nC], metrics [n_beams, n_cpi, 2])."""
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    nb = w.shape[1]
    d_w = torch.from_numpy(np.ascontiguousarray(w)).cuda()
    wo, out = guarded(torch, (nb, n_cpi, nD, nC), torch.complex64)
    wm, met = guarded(torch, (nb, n_cpi, 2), torch.float64)
    amb.beamform_wdev(d_in.data_ptr(), K, n_cpi, d_w.data_ptr(), nb, out.data_ptr(), met.data_ptr(), stream(torch))
    torch.cuda.synchronize()
    assert guard_intact(wo) and guard_intact(wm)
    return out.cpu().numpy(), met.cpu().numpy()


# (geometry, K, n_beams, n_cpi)
WDEV_CASES = [(SMALL, 2, 1, 1), (SMALL, 4, 4, 2), (SMALL, 8, 8, 3), (SMALL, 4, 3, 3), (EVEN, 2, 2, 3), (EVEN, 4, 5, 1),
              (EVEN, 8, 3, 2), (CFG2, 4, 4, 3)]
WDEV_IDS = [f"{g[1] - g[0] + 1}cols-K{k}-b{b}-cpi{c}" for g, k, b, c in WDEV_CASES]


@pytest.mark.parametrize("case", WDEV_CASES, ids=WDEV_IDS)
def test_replicated_weights_give_the_bits_of_beamform_dev(b2, torch, case):
    geom, K, nb, n_cpi = case
    amb = handle(b2, geom)
    maps = crafted(K, n_cpi, amb.get_n_doppler_bins(), amb.get_n_delay_bins(), seed=4000 + 100 * K + 10 * nb + n_cpi)
    d_in = torch.from_numpy(maps).cuda()
    w = weights(1, nb, K, seed=11 + K + nb)
    out_h, met_h = beamform_host_w(torch, amb, d_in, K, n_cpi, w[0])
    out_d, met_d = beamform_dev_w(torch, amb, d_in, K, n_cpi, np.repeat(w, n_cpi, axis=0))
    assert np.array_equal(out_d.view(np.uint32), out_h.view(np.uint32))
    assert np.array_equal(met_d.view(np.uint64), met_h.view(np.uint64))


@pytest.mark.parametrize("case", [WDEV_CASES[1], WDEV_CASES[2], WDEV_CASES[4], WDEV_CASES[7]],
                         ids=[WDEV_IDS[1], WDEV_IDS[2], WDEV_IDS[4], WDEV_IDS[7]])
def test_weights_per_cpi_give_the_bits_of_one_call_per_cpi(b2, torch, case):
    geom, K, nb, n_cpi = case
    amb = handle(b2, geom)
    maps = crafted(K, n_cpi, amb.get_n_doppler_bins(), amb.get_n_delay_bins(), seed=4500 + 100 * K + 10 * nb + n_cpi)
    w = weights(n_cpi, nb, K, seed=17 + K + nb)
    out, met = beamform_dev_w(torch, amb, torch.from_numpy(maps).cuda(), K, n_cpi, w)
    worst = 0.0
    for c in range(n_cpi):
        one, _ = beamform_host_w(torch, amb, torch.from_numpy(np.ascontiguousarray(maps[:, c:c + 1])).cuda(), K, 1, w[c])
        assert np.array_equal(out[:, c].view(np.uint32), one[:, 0].view(np.uint32)), c
        for b in range(nb):
            noise, peak = set_metrics64(out[b, c])
            worst = max(worst, abs(met[b, c, 0] - noise), abs(met[b, c, 1] - peak))
            assert abs(met[b, c, 0] - noise) <= DB_TOL and abs(met[b, c, 1] - peak) <= DB_TOL, (b, c)
    print(f"beamform_wdev metrics K={K} beams={nb} n_cpi={n_cpi}: largest difference {worst:.3e} dB")


def test_beamform_wdev_refusals_write_nothing(b2, torch):
    from blah2_amd import _lib
    amb = handle(b2, SMALL)
    L, h = amb._L, amb._h
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    cells = nD * nC
    d_in = torch.from_numpy(crafted(8, 3, nD, nC, seed=5)).cuda()
    wo, out = guarded(torch, (MAX_BATCH, nD, nC), torch.complex64)
    wm, met = guarded(torch, (MAX_BATCH, 2), torch.float64)
    d_w = torch.from_numpy(weights(MAX_BATCH, 8, 8, seed=3)).cuda()
    int_map, int_met = C.c_void_p(), C.c_void_p()
    assert L.blah2hip_amb_result_ptrs(h, C.byref(int_map), C.byref(int_met)) == _lib.OK
    # (d_map, n_surv, n_cpi, d_w, n_beams, d_beam_map, d_beam_metrics)
    good = [d_in.data_ptr(), 2, 3, d_w.data_ptr(), 2, out.data_ptr(), met.data_ptr()]
    bad = {
        "n_surv 0": {1: 0}, "n_surv 9": {1: 9, 2: 1}, "n_beams 0": {4: 0}, "n_beams 9": {4: 9, 2: 1}, "n_cpi 0": {2: 0},
        "n_surv * n_cpi above max_batch": {1: 8, 2: 4, 4: 1}, "n_beams * n_cpi above max_batch": {1: 1, 2: 4, 4: 8},
        "NULL d_w": {3: None}, "NULL beam map": {5: None}, "NULL beam metrics": {6: None},
        "beam map inside the input": {5: d_in.data_ptr() + 8 * (2 * 3 * cells - 1)},
        "beam map around the input's start": {0: out.data_ptr() + 8 * cells},
        "beam metrics inside the input": {6: d_in.data_ptr() + 16},
        "beam map in the handle's own map": {0: None, 5: int_map.value + 8 * cells},
    }
    for name, change in bad.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert L.blah2hip_amb_beamform_wdev(h, *args, None) == _lib.ERR_INVALID, name
    assert L.blah2hip_amb_beamform_wdev(None, *good, None) == _lib.ERR_INVALID
    torch.cuda.synchronize()
    assert untouched(wo) and untouched(wm)
    assert L.blah2hip_amb_beamform_wdev(h, *good, None) == _lib.OK
    torch.cuda.synchronize()
    assert guard_intact(wo) and guard_intact(wm) and not untouched(wo) and not untouched(wm)


# ---- 4. end to end ------------------------------------------------------------------------------------------------------
def test_adaptive_beams_null_the_interferer_and_keep_the_target(b2, torch):
    """The scenario of tests/adaptive_crafted.py through adaptive_beamform_dev and the 1-D detector.  Expected difference
    of the interferer-row mean power between the device's MVDR beam and the fp64 pipeline on the same maps: a weight error
    near 1e-7 against an interferer amplitude of 100 is 1e-5 of a noise-level residual, about 1e-4 dB; the bound of
    0.01 dB leaves a hundredfold margin.  Measured on an MI355X: -3.9e-7 dB."""
    K, nb = A.K, len(A.BEAMS_DEG)
    amb = handle(b2, SMALL)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    assert (nD, nC) == (A.ND, A.NC)
    maps = A.scene()
    _, w_ref, ok_ref, mv_ref = A.pipeline64(maps)
    conv = A.conventional64(maps)
    st = stream(torch)
    steer = b2.ula_steering(K, A.SPACING, A.BEAMS_DEG)
    d_in = torch.from_numpy(maps).cuda()
    wc, cov = guarded(torch, (1, K, K), torch.complex128)
    ww, w = guarded(torch, (1, nb, K), torch.complex64)
    wk, ok = guarded(torch, (1,), torch.int32)
    wo, beams = guarded(torch, (nb, 1, nD, nC), torch.complex64)
    wm, met = guarded(torch, (nb, 1, 2), torch.float64)
    amb.adaptive_beamform_dev(d_in.data_ptr(), K, 1, steer, A.LOADING, cov.data_ptr(), w.data_ptr(), ok.data_ptr(),
                              beams.data_ptr(), met.data_ptr(), None, st)
    cap = nD * nC
    d_hits = torch.zeros((nb, cap, 2), dtype=torch.float64, device="cuda")
    d_cnt = torch.zeros(nb, dtype=torch.int32, device="cuda")
    b2.CfarDetector1D(1e-5, 2, 6, 5, 15.0).process_dev(amb, nb, d_hits.data_ptr(), cap, d_cnt.data_ptr(), beams.data_ptr(),
                                                       met.data_ptr(), st)
    torch.cuda.synchronize()
    for whole in (wc, ww, wk, wo, wm):
        assert guard_intact(whole)
    assert ok.cpu().numpy().tolist() == ok_ref.tolist() == [1]
    out = beams.cpu().numpy()
    i_dev, i_ref, i_conv = A.interferer_db(out[0, 0]), A.interferer_db(mv_ref[0, 0]), A.interferer_db(conv[0, 0])
    print(f"interferer rows of the 20 degree beam: conventional {i_conv:.3f} dB, MVDR fp64 {i_ref:.5f} dB, MVDR device {i_dev:.5f} dB, "
          f"difference {i_dev - i_ref:+.3e} dB; target cell {A.target_db(out[0, 0]):.3f} dB")
    assert abs(i_dev - i_ref) <= 0.01
    assert i_conv - i_dev >= 20.0 and abs(A.target_db(out[0, 0]) - A.TARGET_DB) <= 0.5
    for b in range(nb):
        noise, peak = set_metrics64(out[b, 0])
        assert abs(met.cpu().numpy()[b, 0, 0] - noise) <= DB_TOL and abs(met.cpu().numpy()[b, 0, 1] - peak) <= DB_TOL, b
    # the target is among the detections of the 20 degree beam (virtual CPI 0)
    counts = d_cnt.cpu().numpy()
    assert 0 < counts[0] <= cap
    hits = d_hits.cpu().numpy().view(b2.HIT_DTYPE).reshape(nb, cap)[0, :counts[0]]
    assert ((hits["row"] == A.TARGET_CELL[0]) & (hits["col"] == A.TARGET_CELL[1])).any()
