"""Strong-echo cancellation on the device (blah2hip_clean_*) against the fp64 restatements of blah2_amd.process.

Gates (the issue's): |dG| <= 1e-5 max_p G[p][p] and |db[p]| <= 1e-5 sqrt(G[p][p] sum |y|^2) -- the project's gate for the
clutter correlations on their Cauchy-Schwarz scale -- with exact conjugate symmetry and a real diagonal; amplitudes
||da|| <= 2e-5 kappa(G_l) ||a|| (first-order perturbation of the two gates above; every scene has kappa <= 1e3, asserted);
the subtraction, with the device's own amplitudes, |y_out - (y - S a)| <= 1e-5 (max |y| + sum_p |a_p| max |x|).  Each test
prints its worst error over its gate; measured on an MI355X, worst over all tests: 4.4e-8 (G), 2.2e-8 (b), 2.1e-8 (amplitudes,
in units of kappa ||a||), 6.4e-8 (subtraction).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import clean_scenes as S

FS = 8192.0
WORST = {}


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    if blah2_amd.device_count() == 0:
        pytest.fail("no GPU visible: the HIP path has no fallback")
    return blah2_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def planes(rng, B, N, stride, snr_atoms, fs=FS):
    """x, y [B][stride] complex64 with canaries (-77 - 77j) in the stride gap; y = noise + the given atoms' replicas."""
    import blah2_amd
    x = np.full((B, stride), -77 - 77j, dtype=np.complex64)
    y = np.full((B, stride), -77 - 77j, dtype=np.complex64)
    for c in range(B):
        x[c, :N] = S.band_limited(rng, max(N, 64))[:N]
        yy = (rng.standard_normal(N) + 1j * rng.standard_normal(N)) / np.sqrt(2)
        for k, at in enumerate(snr_atoms[c]):
            yy = yy + (2.0 + k) * np.exp(1j * k) * blah2_amd.clean_replicas(x[c, :N], [at], fs)[0]
        y[c, :N] = yy
    return x, y


def atom_table(b2, atoms, cap):
    t = np.zeros((len(atoms), cap), dtype=b2.ATOM_DTYPE)
    for c, lst in enumerate(atoms):
        for k, (d, f) in enumerate(lst[:cap]):
            t[c, k] = (d, 0, f)
    return t


class Run:
    """One batch through fit and subtract; everything read back."""

    def __init__(self, b2, torch, ec, fmt, x_raw, x_c, y, N, atoms, counts, cap, loading, in_place=False, out_stride=None):
        B, stride = y.shape
        self.d_x, self.d_y = dev(torch, x_raw), dev(torch, y)
        self.d_at, self.d_cnt = dev(torch, atom_table(b2, atoms, cap)), dev(torch, np.asarray(counts, dtype=np.uint32))
        self.d_amp = dev(torch, np.full((B, cap), 9 + 9j, dtype=np.complex128))
        self.d_ok = dev(torch, np.full(B, 7, dtype=np.int32))
        out_stride = stride if out_stride is None else out_stride
        self.d_out = self.d_y if in_place else dev(torch, np.full((B, out_stride), 5 + 5j, dtype=np.complex64))
        ec.fit_dev(fmt, self.d_x.data_ptr(), self.d_y.data_ptr(), B, stride, self.d_at.data_ptr(), cap, self.d_cnt.data_ptr(), loading,
                   self.d_amp.data_ptr(), self.d_ok.data_ptr())
        ec.subtract_dev(fmt, self.d_x.data_ptr(), self.d_y.data_ptr(), B, stride, self.d_at.data_ptr(), cap, self.d_cnt.data_ptr(),
                        self.d_amp.data_ptr(), self.d_ok.data_ptr(), self.d_out.data_ptr(), out_stride)
        torch.cuda.synchronize()
        self.amp = host(self.d_amp, np.complex128).reshape(B, cap)
        self.ok = host(self.d_ok, np.int32)
        self.out = host(self.d_out, np.complex64).reshape(B, out_stride)
        self.last = [ec.read_last(c) for c in range(B)]


def gate(b2, name, r, x_c, y, N, atoms, counts, cap, loading, fs=FS, kappa_max=1e3):
    """The four gates for every CPI of a run against the restatement."""
    worst = WORST.setdefault(name, dict(G=0.0, b=0.0, a=0.0, sub=0.0))
    for c in range(y.shape[0]):
        P = min(counts[c], cap)
        at = atoms[c][:P]
        xc, yc = x_c[c, :N].astype(np.complex128), y[c, :N].astype(np.complex128)
        a, ok, G, b = b2.clean_fit(xc, yc, at, fs, loading)
        Gd, bd, ad, okd = r.last[c]
        assert okd == ok == r.ok[c] == 1, (c, okd, ok)
        assert np.array_equal(ad, r.amp[c])
        assert not Gd[P:, :].any() and not Gd[:, P:].any() and not bd[P:].any() and not ad[P:].any()
        if P == 0:
            assert np.array_equal(r.out[c, :N], y[c, :N])
            continue
        Gd, bd, ad = Gd[:P, :P], bd[:P], ad[:P]
        assert np.array_equal(Gd, np.conj(Gd.T)) and not Gd.diagonal().imag.any()
        gG = np.max(np.abs(Gd - G)) / np.max(G.diagonal().real)
        gb = np.max(np.abs(bd - b) / np.sqrt(G.diagonal().real * np.sum(np.abs(yc) ** 2)))
        Gl = G + loading * (np.trace(G).real / P) * np.eye(P)
        kappa = np.linalg.cond(Gl)
        assert kappa <= kappa_max, (c, kappa)
        ga = np.linalg.norm(ad - a) / (kappa * np.linalg.norm(a))
        ref = b2.clean_subtract(xc, yc, at, ad, fs)
        gs = np.max(np.abs(r.out[c, :N] - ref)) / (np.max(np.abs(yc)) + np.sum(np.abs(ad)) * np.max(np.abs(xc)))
        for k, v, lim in (("G", gG, 1e-5), ("b", gb, 1e-5), ("a", ga, 2e-5), ("sub", gs, 1e-5)):
            worst[k] = max(worst[k], float(v))
            assert v <= lim, (name, c, k, v)
    print(name, {k: f"{v:.2e}" for k, v in worst.items()})


def scene_atoms(N):
    """Per-CPI atom lists for a batch of three: a three-delay cluster with a far atom, one atom, well-separated atoms."""
    if N < 64:
        return [[(0, 300.0), (7, -1100.0)], [(3, 50.5)], [(-2, 700.0), (9, -2000.25), (4, 2999.0)]]
    return [[(19, 37.3), (20, 37.3), (21, 37.3), (-5, -800.0)], [(40, 1234.5)], [(-5, 10.0), (0, -20.5), (11, 333.0), (30, -4000.0), (40, 4095.9)]]


@pytest.mark.parametrize("N", [41, 4096, 20011, 32768])
def test_fit_and_subtract_against_the_restatement(b2, torch, N):
    rng = np.random.default_rng(100 + N)
    atoms = scene_atoms(N)
    B, cap, stride = 3, 8, N + 3  # an odd stride: CPI 1 starts off 16 bytes (single samples), CPIs 0 and 2 on them
    x, y = planes(rng, B, N, stride, atoms)
    ec = b2.EchoCanceller(N, FS, -5, 40, max_batch=B)
    counts = [len(a) for a in atoms]
    r = Run(b2, torch, ec, b2.FMT_C32, x, x, y, N, atoms, counts, cap, 0.0)
    gate(b2, f"N={N}", r, x, y, N, atoms, counts, cap, 0.0)
    assert (r.out[:, N:] == 5 + 5j).all()  # the stride gap is not written
    # in place: the same bits, the gap's canaries untouched
    r2 = Run(b2, torch, ec, b2.FMT_C32, x, x, y, N, atoms, counts, cap, 0.0, in_place=True)
    assert np.array_equal(r2.out[:, :N].view(np.uint32), r.out[:, :N].view(np.uint32)) and (r2.out[:, N:] == -77 - 77j).all()
    assert np.array_equal(host(r2.d_x, np.complex64).reshape(B, stride), x)
    ec.close()


def test_every_atom_count_in_one_batch(b2, torch):
    """P = 1 .. 32 in one batch, then counts of 0 and above cap_atoms (the first cap_atoms are used)."""
    N, cap = 4096, 32
    rng = np.random.default_rng(7)
    full = [(3 * k - 20, float(rng.uniform(-3000, 3000))) for k in range(40)]
    atoms = [full[:p] for p in range(1, 33)] + [[], full]
    counts = list(range(1, 33)) + [0, 40]
    B = len(atoms)
    x, y = planes(rng, B, N, N, [a[:3] for a in atoms])
    ec = b2.EchoCanceller(N, FS, -20, 100, max_batch=B)
    r = Run(b2, torch, ec, b2.FMT_C32, x, x, y, N, atoms, counts, cap, 0.0)
    gate(b2, "P=1..32", r, x, y, N, atoms, counts, cap, 0.0)
    ec.close()


def test_geometry_span_edges_and_a_failed_cpi(b2, torch):
    """Span 4095, atoms at delay_lo and delay_hi (replicas cut at either end of the CPI), and a CPI with duplicate atoms and
    no loading inside the batch: ok = 0, passed through bit for bit, its neighbours cancelled."""
    N, cap, lo, hi = 20011, 4, -2000, 2095
    rng = np.random.default_rng(8)
    atoms = [[(lo, 100.0), (hi, -200.0), (0, 5.0)], [(7, 1.0), (7, 1.0)], [(hi, 0.0), (lo, 0.0)]]
    B, stride = 3, N + 5
    x, y = planes(rng, B, N, stride, atoms)
    with pytest.raises(b2.Blah2HipError) as e:
        b2.EchoCanceller(N, FS, lo, hi + 1)
    assert e.value.code == b2._lib.ERR_UNSUPPORTED
    ec = b2.EchoCanceller(N, FS, lo, hi, max_batch=B)
    counts = [3, 2, 2]
    r = Run(b2, torch, ec, b2.FMT_C32, x, x, y, N, atoms, counts, cap, 0.0, out_stride=N + 1)
    assert r.ok.tolist() == [1, 0, 1] and not r.amp[1].any()
    assert np.array_equal(r.out[1, :N].view(np.uint32), y[1, :N].view(np.uint32))
    assert (r.out[:, N:] == 5 + 5j).all()
    keep = [0, 2]
    r.last, r.ok, r.amp, r.out = [r.last[c] for c in keep], r.ok[keep], r.amp[keep], r.out[keep]
    gate(b2, "span 4095", r, x[keep], y[keep], N, [atoms[c] for c in keep], [counts[c] for c in keep], cap, 0.0)
    # with loading the duplicate pair is fitted: ok = 1
    r = Run(b2, torch, ec, b2.FMT_C32, x, x, y, N, atoms, counts, cap, 1e-6)
    assert r.ok.tolist() == [1, 1, 1]
    # an atom outside the handle's range, a Doppler that is not finite: that CPI's ok = 0 and it passes through
    bad = [[(hi + 1, 0.0)], [(0, float("nan"))], [(0, 1.0)]]
    r = Run(b2, torch, ec, b2.FMT_C32, x, x, y, N, bad, [1, 1, 1], cap, 1e-6)
    assert r.ok.tolist() == [0, 0, 1]
    assert np.array_equal(r.out[:2, :N].view(np.uint32), y[:2, :N].view(np.uint32))
    ec.close()


def test_forced_grids_and_reproducibility(b2, torch):
    N, cap = 20011, 8
    rng = np.random.default_rng(9)
    atoms = scene_atoms(N)
    counts = [len(a) for a in atoms]
    x, y = planes(rng, 3, N, N, atoms)
    ec = b2.EchoCanceller(N, FS, -5, 40, max_batch=3)
    bits = {}
    for grid in (0, 1, 1 << 20):
        ec.set_option(b2._lib.CLEAN_OPT_GRAM_GRID, grid)
        r = Run(b2, torch, ec, b2.FMT_C32, x, x, y, N, atoms, counts, cap, 0.0)
        g = ec.get_info(b2._lib.CLEAN_INFO_GRAM_GRID)
        assert g == 1 if grid == 1 else 1 < g <= (N + 1023) // 1024
        gate(b2, f"grid {grid}", r, x, y, N, atoms, counts, cap, 0.0)
        r2 = Run(b2, torch, ec, b2.FMT_C32, x, x, y, N, atoms, counts, cap, 0.0)
        for c in range(3):
            for u, v in zip(r.last[c][:3], r2.last[c][:3]):
                assert np.array_equal(u.view(np.uint64), v.view(np.uint64))
        assert np.array_equal(r.out.view(np.uint32), r2.out.view(np.uint32))
        bits[grid] = r
    ec.close()


def test_integer_reference_formats(b2, torch):
    N, cap, B = 4096, 8, 2
    rng = np.random.default_rng(10)
    atoms = [[(19, 37.3), (20, 37.3), (21, 37.3)], [(0, -100.0), (33, 2000.5)]]
    counts = [3, 2]
    for fmt, width, scale in ((b2.FMT_I16X_C32Y, 16, 3000.0), (b2.FMT_I8X_C32Y, 8, 30.0)):
        xf = np.stack([S.band_limited(rng, N) for _ in range(B)]) * scale
        lim = 2 ** (width - 1) - 1
        xi = np.clip(np.rint(np.stack([xf.real, xf.imag], axis=-1)), -lim, lim)
        x_c = (xi[..., 0] + 1j * xi[..., 1]).astype(np.complex64)  # the converted reference
        if width == 16:
            raw = np.zeros((B, N, 4), dtype=np.int16)
            raw[..., :2] = xi
            raw[..., 2:] = rng.integers(-3000, 3000, size=(B, N, 2))  # tuner 2: never read
        else:
            raw = xi.astype(np.int8)
        y = np.zeros((B, N), dtype=np.complex64)
        for c in range(B):
            yy = scale * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
            for k, at in enumerate(atoms[c]):
                yy = yy + (1.0 + k) * b2.clean_replicas(x_c[c], [at], FS)[0]
            y[c] = yy
        ec = b2.EchoCanceller(N, FS, -5, 40, max_batch=B)
        r = Run(b2, torch, ec, fmt, raw, x_c, y, N, atoms, counts, cap, 0.0)
        gate(b2, f"fmt {fmt}", r, x_c, y, N, atoms, counts, cap, 0.0)
        ec.close()


def test_phase_at_length(b2, torch):
    """One atom, N = 2^22, f = 9973.7 Hz at fs = 2 MHz, y the fp64 replica rounded to fp32: the amplitude is 1 and the
    residual meets the subtraction's bound (an fp32 product f n would miss it by two orders of magnitude)."""
    N, fs, at = 1 << 22, 2e6, [(17, 9973.7)]
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(N) + 1j * rng.standard_normal(N)).astype(np.complex64)[None, :]
    y = b2.clean_replicas(x[0], at, fs)[0].astype(np.complex64)[None, :]
    ec = b2.EchoCanceller(N, fs, 0, 32)
    r = Run(b2, torch, ec, b2.FMT_C32, x, x, y, N, [at], [1], 1, 0.0)
    a = r.amp[0, 0]
    assert r.ok[0] == 1 and abs(a - 1) <= 2e-5  # (the amplitude gate at kappa = 1)
    ref = b2.clean_subtract(x[0], y[0], at, r.amp[0], fs)
    g = np.max(np.abs(r.out[0] - ref)) / (np.max(np.abs(y)) + abs(a) * np.max(np.abs(x)))
    print(f"phase at length: worst |y_out - (y - S a)| over its scale {g:.2e}")
    assert g <= 1e-5
    # and against the contract directly: the device's replica is within 8 2^-24 |x| of the fp64 one, sample by sample
    s = b2.clean_replicas(x[0], at, fs)[0]
    err = np.abs((y[0].astype(np.complex128) - r.out[0].astype(np.complex128)) / a - s)
    bound = (8 + 3) * 2.0 ** -24 * np.abs(np.roll(x[0], 17)) + 1e-12  # + y's own rounding, the amplitude's and the chain's two
    assert (err <= bound).all(), float(np.max(err / bound))
    ec.close()


def test_refusals_leave_the_outputs_alone(b2, torch):
    N, cap = 4096, 4
    rng = np.random.default_rng(12)
    atoms = [[(1, 2.0)], [(3, 4.0)]]
    x, y = planes(rng, 2, N, N, atoms)
    ec = b2.EchoCanceller(N, FS, -5, 40, max_batch=2)
    d_x, d_y = dev(torch, x), dev(torch, y)
    d_at, d_cnt = dev(torch, atom_table(b2, atoms, cap)), dev(torch, np.array([1, 1], dtype=np.uint32))
    d_amp, d_ok = dev(torch, np.full((2, cap), 9 + 9j, dtype=np.complex128)), dev(torch, np.full(2, 7, dtype=np.int32))
    d_out = dev(torch, np.full((2, N), 5 + 5j, dtype=np.complex64))
    L = b2._lib
    px, py, pa, pc, pm, po, pout = (t.data_ptr() for t in (d_x, d_y, d_at, d_cnt, d_amp, d_ok, d_out))

    def fit(fmt=b2.FMT_C32, x=px, y=py, n_cpi=2, stride=N, at=pa, cap_=cap, cnt=pc, loading=0.0, amp=pm, ok=po):
        return ec.fit_dev(fmt, x, y, n_cpi, stride, at, cap_, cnt, loading, amp, ok)

    def sub(fmt=b2.FMT_C32, x=px, y=py, n_cpi=2, stride=N, at=pa, cap_=cap, cnt=pc, amp=pm, ok=po, out=pout, ostride=N):
        return ec.subtract_dev(fmt, x, y, n_cpi, stride, at, cap_, cnt, amp, ok, out, ostride)

    cases = [(fit, dict(fmt=b2.FMT_I16), L.ERR_UNSUPPORTED), (fit, dict(fmt=b2.FMT_F16), L.ERR_UNSUPPORTED), (fit, dict(fmt=99), L.ERR_UNSUPPORTED),
             (fit, dict(x=None), L.ERR_INVALID), (fit, dict(amp=None), L.ERR_INVALID), (fit, dict(n_cpi=0), L.ERR_INVALID),
             (fit, dict(n_cpi=3), L.ERR_INVALID), (fit, dict(cap_=0), L.ERR_INVALID), (fit, dict(cap_=33), L.ERR_INVALID),
             (fit, dict(stride=N - 1), L.ERR_INVALID), (fit, dict(y=py + 4), L.ERR_INVALID), (fit, dict(loading=-1.0), L.ERR_INVALID),
             (fit, dict(loading=float("nan")), L.ERR_INVALID), (fit, dict(amp=py), L.ERR_INVALID), (fit, dict(ok=pm), L.ERR_INVALID),
             (sub, dict(fmt=b2.FMT_I8), L.ERR_UNSUPPORTED), (sub, dict(out=None), L.ERR_INVALID), (sub, dict(ostride=N - 1), L.ERR_INVALID),
             (sub, dict(out=px), L.ERR_INVALID), (sub, dict(out=py + 8), L.ERR_INVALID), (sub, dict(out=pout + 4), L.ERR_INVALID),
             (sub, dict(out=py, ostride=N + 1, stride=N), L.ERR_INVALID)]
    for fn, kw, code in cases:
        with pytest.raises(b2.Blah2HipError) as e:
            fn(**kw)
        assert e.value.code == code, (kw, e.value.code)
    torch.cuda.synchronize()
    assert (host(d_amp, np.complex128) == 9 + 9j).all() and (host(d_ok, np.int32) == 7).all()
    assert (host(d_out, np.complex64) == 5 + 5j).all() and np.array_equal(host(d_y, np.complex64).reshape(2, N), y)
    with pytest.raises(b2.Blah2HipError):
        ec.read_last(0)  # no fit yet
    ec.close()


def test_atoms_dev_against_the_restatement(b2, torch):
    fs, n = 8192, 8192
    amb = b2.Ambiguity(-10, 40, -32, 32, fs, n, max_batch=3)
    cpi = amb.dims.cpi
    nD, nDelay = amb.dims.n_doppler_bins, amb.dims.n_delay_bins
    rng = np.random.default_rng(13)
    cap, cap_atoms, B = 12, 16, 3
    d = np.zeros((B, cap), dtype=b2.DET_DTYPE)
    # CPI 0: ties on snr (rows and columns at the map's edges decide), delays at and beyond the range's ends
    d[0, :6] = [(nD - 1, nDelay - 1, 40.2, 3.0, 20.0), (0, nDelay - 1, 39.6, -7.0, 20.0), (0, 0, -10.4, -7.5, 20.0),
                (nD - 1, 0, -9.5, 1.0, 20.0), (7, 7, 20.5, 2.0, 25.0), (3, 3, 21.5, 2.0, 9.0)]
    # CPI 1: more records than cap (the count says 30: the first cap are the list), random
    d[1]["row"], d[1]["col"] = rng.integers(0, nD, cap), rng.integers(0, nDelay, cap)
    d[1]["delay"], d[1]["doppler"], d[1]["snr"] = rng.uniform(-10, 40, cap), rng.uniform(-30, 30, cap), rng.integers(8, 14, cap)
    # CPI 2: empty
    counts = np.array([6, 30, 0], dtype=np.uint32)
    for trial, (snr_min, echoes, sd, sf) in enumerate(((10.0, 8, 1, 0), (10.0, 3, 2, 1), (0.0, 32, 0, 0), (12.0, 2, 0, 1))):
        perm = [rng.permutation(6), rng.permutation(cap), np.arange(0)]
        ds = d.copy()
        ds[0, :6], ds[1] = d[0, perm[0]], d[1, perm[1]]
        ec = b2.EchoCanceller(n, fs, -10, 40, max_batch=B)
        d_d, d_c = dev(torch, ds), dev(torch, counts)
        d_at = dev(torch, np.zeros((B, cap_atoms), dtype=b2.ATOM_DTYPE))
        d_n, d_u = dev(torch, np.full(B, 99, dtype=np.uint32)), dev(torch, np.full((B, cap_atoms), 99, dtype=np.int32))
        ec.atoms_dev(amb, d_d.data_ptr(), cap, d_c.data_ptr(), B, snr_min, echoes, sd, sf, d_at.data_ptr(), cap_atoms, d_n.data_ptr(),
                     d_u.data_ptr())
        torch.cuda.synchronize()
        at, cnt, used = host(d_at, b2.ATOM_DTYPE).reshape(B, cap_atoms), host(d_n, np.uint32), host(d_u, np.int32).reshape(B, cap_atoms)
        for c in range(B):
            ra, ru = b2.clean_atoms(ds[c], counts[c], snr_min, echoes, sd, sf, -10, 40, cpi, cap_atoms)
            assert cnt[c] == len(ra), (trial, c)
            assert np.array_equal(at[c, :len(ra)], ra) and used[c, :len(ru)].tolist() == ru.tolist() and (used[c, len(ru):] == -1).all()
            # the list's order does not matter: the same atoms as from the unshuffled list
            r0 = b2.clean_atoms(d[c], counts[c], snr_min, echoes, sd, sf, -10, 40, cpi, cap_atoms)[0]
            assert np.array_equal(ra, r0)
        ec.close()
    amb.close()
